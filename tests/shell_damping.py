"""Hinge damping of the shell model (mpm_set_shell_damping; drake_amd/csrc/mpm_shell.h, HINGE DAMPING) on the CPU: the
model restated in numpy float64 from its definition -- psidot = cos(theta / 2) grad theta . v with theta by arctan2 --,
a float32 restatement of shell_hinge_core's damped modes operation by operation, the velocity states of the tests, the
guard, and the bound.  Meshes, states, hinges, grad_theta64 and kappas are tests/shell_bending.py's, the layout strips
tests/creases.py's.

The model.  Per hinge, w_j = v_j - v_0:  thetadot = sum_j G_j . v_j = G1 . w1 + G2 . w2 + G3 . w3 (sum_j G_j = 0),
psidot = cos(theta / 2) thetadot,  m_d = -bkc psidot cos(theta / 2),  f_j = m_d G_j,  power = bkc psidot^2.

The bound.  D_hj = |bkc| dpsi |G_hj| V (kappa_A + kappa_B),  V = |G2| (|w2| + (|a| / |e|) |w1|) + |G3| (|w3| +
(|b| / |e|) |w1|).  The damping part of a record lies within R_SHELL_DAMP 2^-24 D of the float64 one: 62.5, counted in
mpm_shell.h (thetadot 21.25, psidot 7.5, m_d 8, the sum with m_el 0.5, G and the record 24.5, second order 0.75); a row
of n_i records adds n_i.  A damped hinge's full record: (R_SHELL + 0.5) T + R_SHELL_DAMP D.  psidot within 29 V
(kappa_A + kappa_B) 2^-24.  The numbers are counts, not fits: tests/test_shell_damping.py pushes the float32 restatement
and the host compile through them on every case, and profiles/shell_damping.txt holds the worst shares."""
import math

import numpy as np

from tests import shell_bending as sb

U = sb.U
F = np.float32
R_SHELL_DAMP = 62.5
R_PSIDOT = 29.0
BETA = 2e-3                      # s, the damping time of the tests


# ---- velocity states: float32 (n_verts, 3) from float32 positions -------------------------------------------------------------
def _zero(x, H, seed):
    return np.zeros_like(x, F)


def _common(x, H, seed):
    return np.broadcast_to(np.array([3.0, -1.5, 0.75], F), x.shape).copy()


def _rotation(x, H, seed):
    """a rigid rotation about a random axis through the mesh's centre, 5 rad/s, on a common velocity"""
    return rotation64(x, seed).astype(F)


def rotation64(x, seed=11):
    """... before it is rounded to float32"""
    r = np.random.default_rng(seed)
    w = r.normal(size=3)
    w *= 5.0 / np.linalg.norm(w)
    X = np.asarray(x, np.float64)
    return np.cross(w, X - X.mean(axis=0)) + np.array([0.5, 0.25, -0.5])


def _random(x, H, seed):
    return np.random.default_rng(seed).normal(size=x.shape).astype(F)


def _opening(x, H, seed):
    """every vertex along the sum of its hinges' G_j: all hinges open"""
    v = np.zeros((len(x), 3))
    if len(H):
        with np.errstate(divide="ignore", invalid="ignore"):
            G = np.nan_to_num(sb.grad_theta64(np.asarray(x, np.float64), H), posinf=0.0, neginf=0.0)
        for j in range(4):
            np.add.at(v, H[:, j], G[:, j])
        s = np.abs(v).max()
        v = v / s if s > 0 else v
    return v.astype(F)


def _cancel(x, H, seed):
    """relative motion of order 1e-3 on a common velocity of order 10: what the differences against corner 0 are for"""
    r = np.random.default_rng(seed)
    return (np.array([10.0, -7.0, 12.0]) + 1e-3 * r.normal(size=x.shape)).astype(F)


VELOCITIES = {"zero": _zero, "common": _common, "rotation": _rotation, "random": _random, "opening": _opening, "cancel": _cancel}
CASES = [(m, s, v) for (m, s) in sb.CASES for v in VELOCITIES]


def velocity(name, st, kind, seed=11):
    x = sb.state(name, st)
    H = sb.hinges(sb.mesh(name)[1])
    return VELOCITIES[kind](x, H, seed)


def case(name, st, kind, beta=BETA):
    """(x32, v32, H, kc, psibar, bkc): the state, the velocities and the rest table's numbers; bkc = float(beta k cbar)"""
    H, kc, psibar = sb.rest_table(name)
    return sb.state(name, st), velocity(name, st, kind), H, kc, psibar, bkc_of(name, beta)


def bkc_of(name, beta, k=sb.K):
    """float(beta k cbar), the product formed in double from the floats beta and k and rounded once"""
    X, T, _ = sb.mesh(name)
    H = sb.hinges(T)
    if len(H) == 0:
        return np.zeros(0, F)
    return (float(F(beta)) * float(F(k)) * sb.cbar64(sb.rest_shape(name).astype(np.float64), H)).astype(F)


# ---- the model in float64 --------------------------------------------------------------------------------------------------
def _w(v, H):
    v = np.asarray(v, np.float64)
    return [v[H[:, j]] - v[H[:, 0]] for j in range(4)]


def psidot64(x, v, H):
    """cos(theta / 2) grad theta . v, theta by arctan2; the velocities as differences against corner 0 (sum_j G_j = 0)"""
    if len(H) == 0:
        return np.zeros(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        G = sb.grad_theta64(x, H)
        w = _w(v, H)
        thetadot = sum((G[:, j] * w[j]).sum(axis=1) for j in range(1, 4))
        return np.cos(0.5 * sb.theta64(x, H)) * thetadot


def records64(x, v, H, bkc, act=None, wrong=None):
    """the damping part's corner records (n, 4, 3), psidot (n,) and the power terms (n,); `wrong`: one of the three wrong
    models of tests/test_shell_damping.py"""
    if len(H) == 0:
        return np.zeros((0, 4, 3)), np.zeros(0), np.zeros(0)
    b = np.asarray(bkc, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        G = sb.grad_theta64(x, H)
        c = np.cos(0.5 * sb.theta64(x, H))
        w = _w(v, H)
        if wrong == "edge corners ignored":
            w[1] = np.zeros_like(w[1])
            vv = np.asarray(v, np.float64)
            thetadot = (G[:, 2] * vv[H[:, 2]]).sum(axis=1) + (G[:, 3] * vv[H[:, 3]]).sum(axis=1)
        else:
            thetadot = sum((G[:, j] * w[j]).sum(axis=1) for j in range(1, 4))
        pd = c * thetadot
        m = -b * pd * c
        if wrong == "no dpsi^2":
            m = -b * thetadot
        elif wrong == "sign":
            m = -m
        rec = m[:, None, None] * G
        power = b * pd * pd
    if act is not None:
        rec[~act], pd[~act], power[~act] = 0.0, 0.0, 0.0
    return rec, pd, power


def force64(x, v, H, bkc, act=None):
    rec, _, _ = records64(x, v, H, bkc, act)
    f = np.zeros((len(x), 3))
    for j in range(4):
        np.add.at(f, H[:, j], rec[:, j])
    return f


def scales(x, v, H, bkc, act=None):
    """(D (n, 4) the unit of every record's damping part, V (kappa_A + kappa_B) (n,) psidot's unit)"""
    if len(H) == 0:
        return np.zeros((0, 4)), np.zeros(0)
    x = np.asarray(x, np.float64)
    n = lambda q: np.linalg.norm(q, axis=1)   # noqa: E731
    with np.errstate(divide="ignore", invalid="ignore"):
        kA, kB = sb.kappas(x, H)
        G = np.linalg.norm(sb.grad_theta64(x, H), axis=2)
        e, a, b = x[H[:, 1]] - x[H[:, 0]], x[H[:, 2]] - x[H[:, 0]], x[H[:, 3]] - x[H[:, 0]]
        w = _w(v, H)
        V = G[:, 2] * (n(w[2]) + n(a) / n(e) * n(w[1])) + G[:, 3] * (n(w[3]) + n(b) / n(e) * n(w[1]))
        dpsi = np.abs(np.cos(0.5 * sb.theta64(x, H)))
        pu = V * (kA + kB)
        D = (np.abs(np.asarray(bkc, np.float64)) * dpsi * pu)[:, None] * G
    if act is not None:
        D[~act], pu[~act] = 0.0, 0.0
    return D, pu


def row_bounds(x, v, H, bkc, act=None):
    """(B_D (n_verts,) the rows' sums of D, N (n_verts,) the records per row)"""
    B, N = np.zeros(len(x)), np.zeros(len(x))
    if len(H):
        D, _ = scales(x, v, H, bkc, act)
        for j in range(4):
            np.add.at(B, H[:, j], D[:, j])
            np.add.at(N, H[:, j], 1.0)
    return B, N


def power_bound(x, v, H, bkc, act=None):
    """per hinge: the float term (bkc psidot) psidot against float64 -- psidot's error d = 29 V (kappa_A + kappa_B) 2^-24
    enters as |bkc| (2 |psidot| d + d^2), and the two products round the term itself: 2 2^-24 of it (3 allowed)"""
    if len(H) == 0:
        return np.zeros(0)
    _, pu = scales(x, v, H, bkc, act)
    _, pd, power = records64(x, v, H, bkc, act)
    d = R_PSIDOT * U * pu
    return np.abs(np.asarray(bkc, np.float64)) * (2 * np.abs(pd) * d + d * d) + 3 * U * power


def share(err, unit, R):
    """the worst |err| / (R 2^-24 unit) (0 where the error vanishes)"""
    e, b = np.abs(np.asarray(err, np.float64)), R * U * np.asarray(unit, np.float64)
    while e.ndim > b.ndim:
        e = e.max(axis=-1)
    w = np.where(e == 0, 0.0, e / np.maximum(b, 1e-300))
    return float(w.max()) if w.size else 0.0


# ---- shell_hinge_core's damped modes restated in float32 ------------------------------------------------------------------------
def hinges32(x32, v32, H, kc, psibar, bkc, elastic=True):
    """shell_hinge_core<1> (elastic) / <2> on every hinge, operation by operation in float32: (records (n, 4, 3), psi,
    psidot, power (n,) float32, acts (n,) bool)"""
    x, v = np.asarray(x32, F), np.asarray(v32, F)
    kc, psibar, bkc = np.asarray(kc, F), np.asarray(psibar, F), np.asarray(bkc, F)
    if len(H) == 0:
        z = np.zeros(0, F)
        return np.zeros((0, 4, 3), F), z, z, z, np.zeros(0, bool)
    c32, d32 = sb._cross32, sb._dot32
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        e, a, b = x[H[:, 1]] - x[H[:, 0]], x[H[:, 2]] - x[H[:, 0]], x[H[:, 3]] - x[H[:, 0]]
        nA, nB = c32(e, a), c32(b, e)
        ee, AA, BB = d32(e, e), d32(nA, nA), d32(nB, nB)
        on = (ee >= F(sb.GATE)) & (AA >= F(sb.GATE)) & (BB >= F(sb.GATE))
        le, lA, lB = np.sqrt(ee), np.sqrt(AA), np.sqrt(BB)
        rA, rB = F(1) / lA, F(1) / lB
        hA, hB = nA * rA[:, None], nB * rB[:, None]
        d, s = hA - hB, hA + hB
        t = d32(e, c32(nA, nB))
        mag = np.sqrt(d32(d, d))
        psi = np.where(t >= 0, mag, -mag).astype(F)
        dpsi = F(0.5) * np.sqrt(d32(s, s))
        m_el = -(kc * (psi - psibar)) * dpsi
        gA, gB = le / AA, le / BB
        re = F(1) / ee
        wA, wB = d32(a, e) * re, d32(b, e) * re
        uA, uB = F(1) - wA, F(1) - wB
        w1, w2, w3 = v[H[:, 1]] - v[H[:, 0]], v[H[:, 2]] - v[H[:, 0]], v[H[:, 3]] - v[H[:, 0]]
        p2, p3 = w2 - wA[:, None] * w1, w3 - wB[:, None] * w1
        sA, sB = d32(nA, p2), d32(nB, p3)
        thetadot = -(gA * sA + gB * sB)
        psidot = dpsi * thetadot
        bp = bkc * psidot
        m_d = -bp * dpsi
        damped = bkc != 0
        m = np.where(damped, m_el + m_d, m_el) if elastic else np.where(damped, m_d, F(0))
        m = m.astype(F)
        power = np.where(damped, bp * psidot, F(0)).astype(F)
        f2 = m[:, None] * -(gA[:, None] * nA)
        f3 = m[:, None] * -(gB[:, None] * nB)
        f1 = -(wA[:, None] * f2 + wB[:, None] * f3)
        f0 = -(uA[:, None] * f2 + uB[:, None] * f3)
    rec = np.stack([f0, f1, f2, f3], axis=1).astype(F)
    psidot = psidot.astype(F)
    rec[~on], psi[~on], psidot[~on], power[~on] = 0, 0, 0, 0
    return rec, psi, psidot, power, on


# ---- the guard ---------------------------------------------------------------------------------------------------------------
def link_limit(W, G):
    """mpm_links.h's link_limit restated: the float not above the positive root of W dt^2 + 2 G dt = 4"""
    if not (W > 0.0) and not (G > 0.0):
        return np.inf
    if not (math.isfinite(W) and math.isfinite(G)):
        return 0.0
    lim = 4.0 / (G + math.sqrt(G * G + 4.0 * W))
    dt = F(lim)
    while dt > 0 and (float(dt) > lim or W * float(dt) * float(dt) + 2.0 * G * float(dt) > 4.0):
        dt = np.nextafter(dt, F(0))
    return float(dt)


def elastic_limit(W):
    """stable_dt_limit(sqrt(W)): the float not above 2 / sqrt(W)"""
    if not W > 0.0:
        return np.inf
    lim = 2.0 / math.sqrt(W)
    dt = F(lim)
    if float(dt) > lim:
        dt = np.nextafter(dt, F(0))
    return float(dt)


def row_rates(X_rest, H, kc, mass, flat=False):
    """per vertex: (1 / m_i) sum_h kc cos^2(thetabar / 2) |G_hi| sum_j |G_hj| at the rest shape, in float64"""
    S = np.zeros(len(X_rest))
    if len(H):
        X = np.asarray(X_rest, np.float64)
        G = np.linalg.norm(sb.grad_theta64(X, H), axis=2)
        c2 = np.ones(len(H)) if flat else np.cos(0.5 * sb.theta64(X, H)) ** 2
        for j in range(4):
            np.add.at(S, H[:, j], np.asarray(kc, np.float64) * c2 * G[:, j] * G.sum(axis=1))
    return S / np.asarray(mass, np.float64)


def max_stable_dt(rates, beta_of_row):
    """the guard from the rows' rates and their cloths' beta: link_limit(W, G), the elastic expression while G = 0"""
    rates, beta = np.asarray(rates, np.float64), np.asarray(beta_of_row, np.float64)
    W = float(rates.max()) if len(rates) else 0.0
    G = float((rates * beta).max()) if len(rates) else 0.0
    return link_limit(W, G) if G > 0.0 else elastic_limit(W)
