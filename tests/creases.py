"""Creases: plastic shell hinges (mpm_set_creases; drake_amd/csrc/mpm_shell.h) on the CPU: the yield rule restated in
numpy float64 from its definition on top of tests/shell_bending.py's meshes, states, hinges, theta64, psi64 and kappas; a
float32 restatement of shell_angle and crease_return, operation by operation; the rounding bounds; the layout scenes.

The model.  Per hinge with its cloth's y = float(2 sin(yield_angle / 2)), eta, P = float(2 sin(max_angle / 2)):
    t = |psi - psibar| cos(theta / 2);  the hinge yields where it acts and t > y;  then
    psibar' = clamp(psi - sign(psi - psibar) (y / cos(theta / 2) + eta (|psi - psibar| - y / cos(theta / 2))), -P, P),
otherwise psibar' = psibar.  The float64 values are those of the FLOAT positions and the float y, eta, P, psibar.

The bounds, counted in mpm_shell.h (CREASES: "Roundings"), first order, in units of 2^-24 of
    W = (kappa_A + kappa_B) (1 + |psi| + |psibar|):
    |t - t64| <= R_T W 2^-24, R_T = 22 (psi 13, the subtraction 0.5, dpsi's absolute error 7, the product 0.5, second order 1);
    |psibar' - psibar'64| <= R_PB W / cos(theta / 2) 2^-24 on a hinge that yields, R_PB = 24 (psi 13, the subtraction
    0.5, dpsi through the division 7, the division 0.5, the hardening line 1.5, the final subtraction 0.5, second order 1).
A hinge is UNDECIDED where |t64 - y| <= R_T W 2^-24; only decided hinges are compared with float64.  Counts, not fits:
tests/test_creases.py pushes the float32 restatement below through the same bounds on every case; its worst share is
0.043 of t's bound (the jittered sheet, rigid) and 0.026 of psibar's (icosphere2, perturbed, yield angle 0.05)."""
import numpy as np

from tests import shell_bending as sb

U = sb.U
F = np.float32
R_T, R_PB = 22.0, 24.0
YIELD_ANGLES = (0.05, 0.3)      # rad
CAP = 0.02                      # at most this share of the active hinges of a case may be undecided


def chord(angle):
    """y and P as the host forms them: (float)(2 sin(angle / 2)) in double from the float angle, rounded once"""
    return (2.0 * np.sin(0.5 * np.asarray(angle, F).astype(np.float64))).astype(F)


# ---- the model in float64 --------------------------------------------------------------------------------------------------
def values64(x32, H, psibar):
    """(psi, dpsi = cos(theta / 2), t, W) per hinge in float64 from float positions and float psibar"""
    x = np.asarray(x32, np.float64)
    pb = np.asarray(psibar, F).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        th = sb.theta64(x, H)
        psi, dpsi = 2.0 * np.sin(0.5 * th), np.cos(0.5 * th)
        kA, kB = sb.kappas(x, H)
        W = (kA + kB) * (1.0 + np.abs(psi) + np.abs(pb))
    return psi, dpsi, np.abs(psi - pb) * dpsi, W


def verdict64(x32, H, psibar, y, act):
    """(yields (n,) bool, decided (n,) bool): the exact verdict t64 > y on the hinges that act, and where the float
    verdict must agree: |t64 - y| above the bound of t.  An inactive hinge never yields and is decided; so is y = 0."""
    _, _, t, W = values64(x32, H, psibar)
    y = np.broadcast_to(np.asarray(y, F).astype(np.float64), t.shape)
    act = np.asarray(act, bool)
    with np.errstate(invalid="ignore"):
        yields = act & (y > 0) & (t > y)
        decided = ~act | (y == 0) | (np.abs(t - y) > R_T * U * W)
    return yields, decided


def return64(x32, H, psibar, y, eta, P, act):
    """the exact psibar' per hinge, and its bound R_PB W / dpsi 2^-24 (0 where the hinge does not yield)"""
    psi, dpsi, t, W = values64(x32, H, psibar)
    pb = np.asarray(psibar, F).astype(np.float64)
    y, eta, P = (np.broadcast_to(np.asarray(a, F).astype(np.float64), t.shape) for a in (y, eta, P))
    yields, _ = verdict64(x32, H, psibar, y, act)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = psi - pb
        dy = y / dpsi
        pn = psi - np.copysign(dy + eta * (np.abs(d) - dy), d)
        bound = R_PB * U * W / dpsi
    out = np.where(yields, np.clip(pn, -P, P), pb)
    return out, np.where(yields, bound, 0.0)


# ---- the engine's arithmetic restated in float32 ---------------------------------------------------------------------------
def angle32(x32, H):
    """shell_angle on every hinge, operation by operation in float32: (psi, dpsi, acts)"""
    x = np.asarray(x32, F)
    if len(H) == 0:
        return np.zeros(0, F), np.zeros(0, F), np.zeros(0, bool)
    c32, d32 = sb._cross32, sb._dot32
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        e, a, b = x[H[:, 1]] - x[H[:, 0]], x[H[:, 2]] - x[H[:, 0]], x[H[:, 3]] - x[H[:, 0]]
        nA, nB = c32(e, a), c32(b, e)
        ee, AA, BB = d32(e, e), d32(nA, nA), d32(nB, nB)
        on = (ee >= F(sb.GATE)) & (AA >= F(sb.GATE)) & (BB >= F(sb.GATE))
        lA, lB = np.sqrt(AA), np.sqrt(BB)
        rA, rB = F(1) / lA, F(1) / lB
        hA, hB = nA * rA[:, None], nB * rB[:, None]
        d, s = hA - hB, hA + hB
        t = d32(e, c32(nA, nB))
        mag = np.sqrt(d32(d, d))
        psi = np.where(t >= 0, mag, -mag).astype(F)
        dpsi = (F(0.5) * np.sqrt(d32(s, s))).astype(F)
    psi[~on], dpsi[~on] = 0, 0
    return psi, dpsi, on


def return32(psi, dpsi, on, psibar, y, eta, P):
    """crease_return, operation by operation in float32: (psibar', yields, t)"""
    psi, dpsi = np.asarray(psi, F), np.asarray(dpsi, F)
    psibar, y, eta, P = (np.broadcast_to(np.asarray(a, F), psi.shape) for a in (psibar, y, eta, P))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        d = psi - psibar
        ad = np.abs(d)
        t = ad * dpsi
        yields = np.asarray(on, bool) & (y > 0) & (t > y)
        dy = y / dpsi
        dn = dy + eta * (ad - dy)
        pn = psi - np.copysign(dn, d)
        out = np.where(yields, np.minimum(np.maximum(pn, -P), P), psibar).astype(F)
    return out, yields, t.astype(F)


# ---- cases ------------------------------------------------------------------------------------------------------------------
CASES = sb.CASES
SWEEP = (-3.1, -1.0, -0.4, -0.1, -0.051, -0.049, -0.01, 0.0, 0.01, 0.049, 0.051, 0.1, 0.4, 1.0, 3.1)   # the strip's hinge, rad


def case(name, st):
    """(x32 the state, H, psibar the rest table's)"""
    H, _, psibar = sb.rest_table(name)
    return sb.state(name, st), H, psibar


def sweep_state(theta):
    return sb.folded(sb.rest_shape("strip"), theta).astype(F)


# ---- layout scenes -----------------------------------------------------------------------------------------------------------
def strip(n_faces, h=None, origin=(0.2, 0.45, 0.5), seed=0):
    """a triangle strip of n_faces faces along x (n_faces + 2 vertices, n_faces - 1 hinges), and a bent state of it: every
    vertex lifted by a random height of up to 0.3 h, so that hinges lie on both sides of the yield angles"""
    h = sb.H0 / 4 if h is None else h
    n = n_faces + 2
    i = np.arange(n)
    X = np.stack([origin[0] + 0.5 * h * i, origin[1] + h * (i % 2), np.full(n, origin[2])], axis=1)
    T = np.array([(k, k + 1, k + 2) if k % 2 == 0 else (k + 1, k, k + 2) for k in range(n_faces)], np.int32)
    r = np.random.default_rng(seed + n_faces)
    x = X.copy()
    x[:, 2] += 0.3 * h * r.uniform(-1.0, 1.0, n)
    assert X.min() > 0.1 and X.max() < 0.9
    return X.astype(F), T, x.astype(F)


STRIPS = (64, 65, 66, 256, 257, 258)    # faces: 63, 64, 65 hinges around a wave; 255, 256, 257 around a block


def three_cloths(angle=2.6):
    """three 7 x 7 sheets side by side along y: [(X, T)], the crease table's rows (yield_angle, hardening, max_angle) --
    plastic with eta = 0, elastic (shell bending on, yield_angle 0) between the two, plastic with eta = 0.5 and max_angle
    1.0 so that the clamp acts -- and a state of all vertices: every sheet folded by `angle` about its middle line"""
    from tests import bending as bd
    X, T = bd.sheet(7, 7)
    cloths, xs = [], []
    for c in range(3):
        Xc = (X.astype(np.float64) + np.array([0.0, (c - 1) * 8 * sb.H0, 0.0])).astype(F)
        cloths.append((Xc, T))
        xs.append(fold_state(Xc, angle, seed=c))
    rows = [(0.05, 0.0, 0.0), (0.0, 0.0, 0.0), (0.05, 0.5, 1.0)]
    return cloths, rows, np.concatenate(xs).astype(F)


def fold_state(X, angle, seed=0, jitter=0.02):
    """the sheet folded by `angle` about its middle line (shell_bending.fold) with a random lift of every vertex"""
    x = sb.fold(X, angle)
    x[:, 2] += jitter * sb.H0 * np.random.default_rng(seed).uniform(-1.0, 1.0, len(x))
    return x.astype(F)


def hinge_records(H_cloth, rows):
    """(y, eta, P) per hinge from the table's rows and the cloth of every hinge"""
    rows = np.asarray(rows, F).reshape(-1, 3)
    y = np.where(rows[:, 0] == 0, F(0), chord(rows[:, 0])).astype(F)
    P = np.where(rows[:, 2] == 0, F(2), chord(rows[:, 2])).astype(F)
    c = np.asarray(H_cloth, int)
    return y[c], rows[c, 1], P[c]
