"""Every dt guard of the engine against the float64 spectrum of the force the engine holds (tests/guards.py).

1. The engine's guard is below the true limit of the operators K = -df/dx, D = -df/dv assembled in float64 from the
   engine's own numbers: MPM_ARR_MASSES through PIDS, DM_INVERSES and the rest volumes, the shell's kc and psibar, the
   weave's axes, the link and anchor tables as set.  Among the cases a multi-material pair (masses and moduli per cloth)
   and a cloth with mpm_set_rest_shape (rest records from another shape than the mesh as added).
   guard <= true limit (1 + 1e-6): the engine rounds its guard towards zero; 1e-6 is the restatement tests' tolerance.
2. The device force has that spectrum.  phi: the top eigenvector of the float64 operator, scaled to max |phi_i| = 1.  The
   state X +- a phi (or the rest positions with v = +- a phi) is uploaded, the feature's *_forces() read, and
   q_dev = -phi . (f+ - f-) / (2 a phi^T M phi) compared with the same secant of the float64 reference at the identical
   float32 states.  The central secant serves the linear forces too: it removes whatever does not depend on the varied
   state (the elastic part of a link's force while its velocities vary).  a is the largest power of two times H0, chosen
   on the CPU, at which the float64 secant is within 1 % of lambda_max and the feature's rounding bound, carried through
   sum |phi| bound / (2 a phi^T M phi), is below 1 % of it; every feature has one (asserted).  Asserted: |q_dev / q_ref
   - 1| within the carried bound, and guard <= 2 / sqrt(q_dev) (2 / q_dev for a damping operator) with that margin.
   Links and anchors are tested on tables whose springs sit at l == L in the uploaded state (that is where the guard is
   stated); the scenes' own tables, with stretched springs and cords, are in 1.
3. Composition on the engine: composed_limit of the engine's guards passes the spectral-radius condition on the sum of
   the operators, with the engine's masses -- the fan with both bending models, and a 9 x 9 patch of cloth 1 of
   tests/feature_paths.py with that scene's features on it, each at 0.499 of its guard.  true limit / min(guard) is
   recorded.

Every guard / true-limit ratio goes through helpers.MARGINS into the suite's report."""
import functools
import math

import numpy as np
import pytest

from tests import anchors as an
from tests import bending as bd
from tests import damping as dp
from tests import guards as gd
from tests import harness as hs
from tests import links as lk
from tests import shell_bending as sb
from tests import shell_damping as sd
from tests import weave as wv

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
F = np.float32
H0 = bd.H0
UP = np.array([0.0, 0.0, 0.05], np.float32)
MATS = (dict(youngs_modulus=2.5e5, poisson_ratio=0.25), dict(youngs_modulus=6e5, density=1300.0))


_engine = functools.partial(hs.engine, material=dict(gravity=0.0))
_by_id = functools.partial(hs.by_id, split=True)


def _margin(what, ratio):
    print(f"guards [engine]: {what}: {ratio:.4f}")
    hs.record(what, ratio, prefix="guards: ")


def _masses(g):
    return _by_id(g, hs.ARR().MASSES)[1].astype(np.float64)


def _rest_records(g):
    """(dm (nf, 3), vol (nf,)) float32 in original face order, of a SINGLE-material engine (whose MPM_ARR_VOLUMES is the
    record the face kernels read)"""
    return g.download(hs.ARR().DM_INVERSES).reshape(g.n_faces, 4)[:, [0, 1, 3]].copy(), _by_id(g, hs.ARR().VOLUMES)[0].copy()


def _lame32(E, nu):
    """the engine's float Lame parameters (lame, mpm_cloth_host.h): float32 arithmetic throughout"""
    E, nu, one, two = (F(a) for a in (E, nu, 1.0, 2.0))
    return E / (two * (one + nu)), E * nu / ((one + nu) * (one - two * nu))


def _joined(cloths):
    first = np.cumsum([0] + [len(X) for X, _ in cloths])
    X = np.concatenate([X for X, _ in cloths])
    T = np.concatenate([T + o for (_, T), o in zip(cloths, first)])
    cof = np.concatenate([np.full(len(T), c) for c, (_, T) in enumerate(cloths)])
    return X, T, cof, first


def _pair():
    return [(bd.mesh("jittered")[0], bd.mesh("jittered")[1]), ((bd.mesh("fan")[0] + UP).astype(np.float32), bd.mesh("fan")[1])]


def _cloths(scene):
    """(cloths as added, per-cloth materials or None, rest positions of all vertices or None)"""
    if scene == "pair_multi":
        return _pair(), MATS, None
    if scene == "reshaped":      # the jittered sheet with a rest shape 10 % longer along x and 5 % shorter along y
        X, T = bd.mesh("jittered")
        rest = ((X.astype(np.float64) - bd.CENTER) * np.array([1.1, 0.95, 1.0]) + bd.CENTER).astype(np.float32)
        return [(X, T)], None, rest
    X, T = bd.mesh(scene)
    return [(X, T)], None, None


class Rig:
    """one feature on one engine: the operators in float64 from the engine's numbers, the guard, the device force, and the
    float64 reference force with its rounding bound at given float32 states"""

    def __init__(self, g, x0, m, K=None, D=None, guard=None, forces=None, ref=None):
        self.g, self.x0, self.m, self.K, self.D = g, np.asarray(x0, np.float32), m, K, D
        self.guard, self.forces, self.ref = guard, forces, ref


def _scene_engine(scene):
    cloths, mats, rest = _cloths(scene)
    g = _engine(cloths, mats=mats)
    if rest is not None:
        g.set_rest_shape(rest)
    X, T, cof, first = _joined(cloths)
    Xr = X if rest is None else rest
    return g, cloths, mats, Xr, T, cof, first


def _face_records(scene):
    """the rest records of the scene from a single-material twin (Finalize's geometry does not depend on the material)"""
    cloths, _, rest = _cloths(scene)
    twin = _engine(cloths)
    if rest is not None:
        twin.set_rest_shape(rest)
    out = _rest_records(twin)
    twin.destroy()
    return out


# ---- the features ---------------------------------------------------------------------------------------------------------
def bending_rig(scene):
    g, cloths, mats, Xr, T, cof, first = _scene_engine(scene)
    ks = [float(F(1e-6 * (1 + c))) for c in range(len(cloths))]
    g.set_bending(ks)
    n = len(Xr)
    K = np.zeros((3 * n, 3 * n))
    Hs = []
    for c, (Xc, Tc) in enumerate(cloths):
        a, b = first[c], first[c + 1]
        Kc, H = gd.bending_K(ks[c], Xr[a:b], Tc)
        K[3 * a:3 * b, 3 * a:3 * b] = Kc
        Hs.append((H, bd.q_dense(b - a, H)[1]))

    def ref(x32, v32):
        f, bnd = np.zeros((n, 3)), np.zeros((n, 3))
        for c in range(len(cloths)):
            a, b = first[c], first[c + 1]
            H, P = Hs[c]
            f[a:b] = bd.force64(ks[c], H, x32[a:b])
            bnd[a:b] = (U * bd.rounding_count(P) * bd.bound(ks[c], H, x32[a:b]))[:, None]
        return f, bnd

    return Rig(g, Xr, _masses(g), K=gd.sanity(K, "bending"), guard=g.bending_max_stable_dt, forces=g.bending_forces, ref=ref)


def shell_rig(name, beta=None):
    """tests/shell_bending.py's mesh `name` about its rest shape; beta: with the hinge damper, the stiffness sized so that
    the elastic guard is 2 beta_0 = 2 BETA (tests/test_guards.py)"""
    X, T, rest = sb.mesh(name)
    g = _engine([(X, T)])
    g.set_shell_bending([sb.K], rest)
    k = sb.K
    if beta is not None:
        k = float(F(sb.K * (g.shell_max_stable_dt() / (2.0 * sd.BETA)) ** 2))
        g.set_shell_bending([k], rest)
        g.set_shell_damping([beta])
    ids, kc, psibar = g.shell_hinges()
    H = ids.astype(np.int64)
    assert np.array_equal(H, sb.hinges(T)) and len(H)
    Xr = sb.rest_shape(name)
    K = gd.sanity(gd.shell_K(Xr.astype(np.float64), H, kc, psibar), f"shell {name}")
    D, bkc = None, None
    if beta is not None:
        bkc = (float(F(beta)) * float(F(k)) * sb.cbar64(Xr.astype(np.float64), H)).astype(F)
        D = gd.sanity(gd.shell_D(Xr.astype(np.float64), H, bkc), f"shell damper {name}")

    def ref(x32, v32):
        x = x32.astype(np.float64)
        on = sb.active(x32, H)
        if beta is None or not np.any(v32):
            B, N, _ = sb.bound(x, H, kc, psibar, on)
            return sb.force64(x, H, kc, psibar, on), (U * (sb.R_SHELL + N) * B)[:, None] * np.ones(3)
        v = v32.astype(np.float64)
        B, N = sd.row_bounds(x, v, H, bkc, on)
        # (one more unit: bkc here is the double product rounded once, the engine's may differ from it by a rounding)
        return sd.force64(x, v, H, bkc, on), (U * (sd.R_SHELL_DAMP + N + 1.0) * B)[:, None] * np.ones(3)

    forces = g.shell_forces if beta is None else None
    rig = Rig(g, Xr, _masses(g), K=K, D=D, guard=g.shell_max_stable_dt, forces=forces, ref=ref)
    rig.forces_K, rig.forces_D = g.shell_forces, g.shell_damping_forces
    return rig


def weave_rig(scene, material=wv.TWILL, angle="30"):
    g, cloths, mats, Xr, T, cof, first = _scene_engine(scene)
    ang = np.deg2rad(wv.ANGLES[angle])
    d = (np.cos(ang), np.sin(ang), 0.0)
    rows = [tuple(q * (1.0 + 0.5 * c) for q in material[:2]) + material[2:] + d for c in range(len(cloths))]
    g.set_weave(np.array(rows, np.float32))
    coef_f = np.stack([wv.coefficients(*rows[c][:4]) for c in range(len(cloths))])[cof]
    cs = g.weave_axes()
    dm, vol = _face_records(scene)
    n = len(Xr)
    K = gd.sanity(gd.weave_K(Xr.astype(np.float64), T, dm, vol, coef_f, cs), f"weave {scene}")
    R, val = wv.rounding_count(), wv.valence(T, n)

    def ref(x32, v32):
        xc = wv.corners(T, x32)
        f = wv.vertex_sum(T, n, wv.records64(dm, vol, coef_f, cs, xc))
        return f, U * (R + val)[:, None] * -wv.vertex_sum(T, n, wv.record_bound(dm, vol, coef_f, cs, xc))

    return Rig(g, Xr, _masses(g), K=K, guard=g.weave_max_stable_dt, forces=g.weave_forces, ref=ref)


def damping_rig(scene):
    """membrane damping and hinge damping (on a bending stiffness), the hinge part sized to the membrane part's guard"""
    from drake_amd import GpuMpm
    g, cloths, mats, Xr, T, cof, first = _scene_engine(scene)
    nc, n = len(cloths), len(Xr)
    base = GpuMpm.default_material()
    lame = []
    for c in range(nc):
        q = dict(youngs_modulus=base.youngs_modulus, poisson_ratio=base.poisson_ratio)
        q.update({k: v for k, v in (mats[c] if mats else {}).items() if k in q})
        lame.append(_lame32(q["youngs_modulus"], q["poisson_ratio"]))
    ks = [float(F(1e-6 * (1 + c))) for c in range(nc)]
    g.set_bending(ks)
    g.set_damping([(1e-4, 0.0)] * nc)
    gm = g.damping_max_stable_dt()
    g.set_damping([(0.0, 1.0)] * nc)
    gb = g.damping_max_stable_dt()
    betas = np.array([(1e-4 * (1 + 0.5 * c), gb / gm) for c in range(nc)], np.float32)
    g.set_damping(betas)
    dm, vol = _face_records(scene)
    mu = np.array([lame[c][0] for c in cof], np.float32)
    lam = np.array([lame[c][1] for c in cof], np.float32)
    bm = np.array([betas[c][0] for c in cof], np.float32)
    D = gd.membrane_D(Xr.astype(np.float64), T, dm, vol, mu, lam, bm)
    Hs = []
    for c, (Xc, Tc) in enumerate(cloths):
        a, b = first[c], first[c + 1]
        H = bd.hinges(Xr[a:b], Tc)
        Q, P = bd.q_dense(b - a, H)
        Hs.append((H, P))
        D[3 * a:3 * b, 3 * a:3 * b] += gd.kron3(float(betas[c][1]) * ks[c] * Q)
    R = dp.rounding_count()
    x0 = Xr

    def ref(x32, v32):
        f, Bm = dp.forces64(Xr, T, x32, v32, (mu, lam), bm, rest=(dm, vol))
        tol = U * R * Bm
        for c in range(nc):
            a, b = first[c], first[c + 1]
            H, P = Hs[c]
            kb = float(betas[c][1]) * ks[c]
            f[a:b] += bd.force64(kb, H, v32[a:b])
            tol[a:b] += (U * (bd.rounding_count(P) + 2.0) * bd.bound(kb, H, v32[a:b]))[:, None]
        return f, tol

    return Rig(g, x0, _masses(g), D=gd.sanity(D, f"damping {scene}"), guard=g.damping_max_stable_dt, forces=g.damping_forces, ref=ref)


def _at_rest_table(n_a, X, seed, kinds="links"):
    """40 seams and springs between the two sheets of tests/links.py's `mixed` scene, every spring with L = its float
    length in X (l == L within a rounding), stiffness and damping unrelated; a hub of 9 links at vertex 0"""
    r = np.random.default_rng(seed)
    rows = []
    for i in range(40):
        a = 0 if i < 9 else int(r.integers(0, n_a))
        b = n_a + int(r.integers(0, n_a))
        seam = i % 3 == 0
        L = 0.0 if seam else float(lk._l32((X[b] - X[a]).astype(np.float32)[None])[1][0])
        rows.append((a, b, float(r.uniform(10, 80)), L, float(r.uniform(0.005, 0.06)), 0))
    return lk.make_links(rows)


def links_rig(table):
    cloths, scene_links, X = lk.scene("mixed")
    g = _engine(cloths)
    x0 = lk.state("rest", "mixed", X)[0]
    links = scene_links if table == "mixed" else _at_rest_table(len(cloths[0][0]), X, 23)
    if table != "mixed":
        x0 = X
    g.set_links(links)
    n = len(X)
    K, D = gd.link_operators(links, x0, n)

    def ref(x32, v32):
        f, bnd, _ = lk.vertex_forces64(links, x32, v32, n)
        return f, bnd[:, None] * np.ones(3)

    return Rig(g, x0, _masses(g), K=gd.sanity(K, "links"), D=gd.sanity(D, "links damping"), guard=g.links_max_stable_dt,
               forces=g.link_forces, ref=ref)


def _at_rest_anchors():
    """(cloths, anchors, motions, X): 40 seams and springs at l == L from the lower sheet of tests/anchors.py's `mixed`
    scene to points of a body that stands still, a hub of 5 at vertex 0, stiffness and damping unrelated"""
    cloths, _, _, X = an.scene("mixed")
    r = np.random.default_rng(29)
    p_WB = np.array([0.5, 0.5, 0.6], np.float32)
    motions = {0: an.motion32(p_WB, np.eye(3), (0, 0, 0), (0, 0, 0))}
    rows = []
    for i in range(40):
        v = 0 if i < 5 else int(r.integers(0, an.N * an.N))
        y = (X[v].astype(np.float64) + an.GAP * np.array([0.3 * r.normal(), 0.3 * r.normal(), 1.0])).astype(np.float32)
        p_BQ = (y - p_WB).astype(np.float32)
        y32 = (p_WB + p_BQ).astype(np.float32)
        L = 0.0 if i % 3 == 0 else float(lk._l32((y32 - X[v]).astype(np.float32)[None])[1][0])
        rows.append((v, 0, p_BQ, float(r.uniform(10, 80)), L, float(r.uniform(0.005, 0.06)), 0))
    return cloths, an.make_anchors(rows), motions, X


def anchors_rig(table):
    """`hung`, `mixed`: the scenes' tables as set, the bodies' clocks at zero; `at_rest`: seams and springs at l == L from
    the lower sheet of `mixed` to points of a body that stands still"""
    from drake_amd import BodyMotion
    cloths, anchors, motions, X = _at_rest_anchors() if table == "at_rest" else an.scene(table)
    g = _engine(cloths, bodies=an.N_BODIES)
    g.set_body_motions([BodyMotion(b, q[0], q[1].ravel(), q[2], q[3]) for b, q in motions.items()])
    g.set_anchors(anchors)
    x0 = X
    hs.upload(g, x0)
    y32 = g.anchor_state()["point"]
    vq32 = an.points(anchors, motions, 0.0)[3]
    n = len(X)
    K, D = gd.anchor_operators(anchors, x0, y32, n)
    k, c = anchors["stiffness"].astype(np.float64), anchors["damping"].astype(np.float64)

    def ref(x32, v32):
        f, S, _, on = an.anchor_forces64(anchors, x32, v32, y32, vq32)
        far = (k * np.linalg.norm(y32.astype(np.float64), axis=1) + c * np.linalg.norm(vq32.astype(np.float64), axis=1)) * on
        Fv, SS, cnt, E = np.zeros((n, 3)), np.zeros(n), np.zeros(n), np.zeros(n)
        np.add.at(Fv, anchors["vertex"], f)
        np.add.at(SS, anchors["vertex"], S)
        np.add.at(cnt, anchors["vertex"], 1.0)
        np.add.at(E, anchors["vertex"], far)
        return Fv, (U * ((lk.R_LINK + cnt) * SS + E))[:, None] * np.ones(3)

    return Rig(g, x0, _masses(g), K=gd.sanity(K, "anchors"), D=gd.sanity(D, "anchors damping") if np.any(D) else None,
               guard=g.anchors_max_stable_dt, forces=g.anchor_forces, ref=ref)


RIGS = {
    "bending fan": lambda: bending_rig("fan"),
    "bending jittered": lambda: bending_rig("jittered"),
    "bending pair_multi": lambda: bending_rig("pair_multi"),
    "bending reshaped": lambda: bending_rig("reshaped"),
    "shell fan": lambda: shell_rig("fan"),
    "shell icosphere1": lambda: shell_rig("icosphere1"),
    "shell book": lambda: shell_rig("book"),
    "shell damped jittered": lambda: shell_rig("jittered", sd.BETA),
    "shell damped tube 4": lambda: shell_rig("tube", 4 * sd.BETA),
    "weave fan": lambda: weave_rig("fan"),
    "weave pair_multi": lambda: weave_rig("pair_multi", wv.DENIM, "130"),
    "weave reshaped": lambda: weave_rig("reshaped", wv.DENIM, "30"),
    "damping jittered": lambda: damping_rig("jittered"),
    "damping pair_multi": lambda: damping_rig("pair_multi"),
    "damping reshaped": lambda: damping_rig("reshaped"),
    "links mixed": lambda: links_rig("mixed"),
    "links at_rest": lambda: links_rig("at_rest"),
    "anchors hung": lambda: anchors_rig("hung"),
    "anchors mixed": lambda: anchors_rig("mixed"),
    "anchors at_rest": lambda: anchors_rig("at_rest"),
}


# ---- 1 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(RIGS))
def test_the_engines_guard_is_below_the_true_limit(name):
    rig = RIGS[name]()
    guard = rig.guard()
    assert math.isfinite(guard) and guard > 0
    limit = gd.true_limit(rig.K, rig.D, rig.m, start=guard)
    _margin(f"guard / true limit, {name}", guard / limit)
    assert guard <= limit * (1.0 + 1e-6), (name, guard, limit)
    if rig.K is not None and rig.D is not None:
        r = gd.spectral_radius(rig.K, rig.D, rig.m, guard)
        assert r <= 1.0 + gd.RADIUS_TOL, (name, r)
    assert rig.g.stats()["error_flags"] == 0
    rig.g.destroy()


# ---- 2 -------------------------------------------------------------------------------------------------------------------
EXPONENTS_X = range(-3, -11, -1)       # a = 2^e H0 for the positions: from an eighth of the spacing down
EXPONENTS_V = (7,)                     # a = 2^7 H0 = 1 (m / s) for the velocities: the damping forces are linear in v


def secant(force, x0, phi, a, m, kind):
    """(q, sum |phi| (bound+ + bound-) / (2 a' phi^T M phi)) of force(x32, v32) -> (f, bound) at the float32 states
    x0 +- a phi (kind 'K') or (x0, +- a phi) (kind 'D'); a' is the float displacement actually uploaded"""
    z = np.zeros_like(x0)
    if kind == "K":
        sp, sm = ((x0.astype(np.float64) + s * a * phi).astype(F) for s in (1.0, -1.0))
        (fp, bp), (fm, bm) = force(sp, z), force(sm, z)
        step = sp.astype(np.float64) - sm.astype(np.float64)
    else:
        sp, sm = ((s * a * phi).astype(F) for s in (1.0, -1.0))
        (fp, bp), (fm, bm) = force(x0, sp), force(x0, sm)
        step = sp.astype(np.float64) - sm.astype(np.float64)
    # the quotient on the displacement that was uploaded: -step . (f+ - f-) / (step^T M step)
    den = float((m[:, None] * step * step).sum())
    q = -float((step * (np.asarray(fp, np.float64) - np.asarray(fm, np.float64))).sum()) / den
    carried = float((np.abs(step) * (np.abs(bp) + np.abs(bm))).sum()) / den
    return q, carried, (sp, sm)


def choose_a(ref, x0, phi, lam, m, kind):
    """the largest a = 2^e H0 at which the float64 secant is within 1 % of lambda_max and the carried rounding bound below
    1 % of it; None if there is none"""
    for e in (EXPONENTS_X if kind == "K" else EXPONENTS_V):
        a = 2.0 ** e * H0
        q, carried, _ = secant(ref, x0, phi, a, m, kind)
        if abs(q / lam - 1.0) < 0.01 and carried < 0.01 * lam:
            return a, q, carried
    return None


SPECTRA = [("bending fan", "K"), ("bending pair_multi", "K"), ("shell fan", "K"), ("shell icosphere1", "K"),
           ("shell damped jittered", "K"), ("shell damped jittered", "D"), ("weave fan", "K"), ("weave reshaped", "K"),
           ("damping jittered", "D"), ("damping pair_multi", "D"), ("links at_rest", "K"), ("links at_rest", "D"),
           ("anchors at_rest", "K"), ("anchors at_rest", "D")]


@pytest.mark.parametrize("name,kind", SPECTRA)
def test_the_device_force_has_that_spectrum(name, kind):
    rig = RIGS[name]()
    g = rig.g
    lam, phi = gd.lambda_max(rig.K if kind == "K" else rig.D, rig.m)
    phi = phi / np.abs(phi).max()
    chosen = choose_a(rig.ref, rig.x0, phi, lam, rig.m, kind)
    assert chosen is not None, "no step meets both conditions"
    a, q_ref, carried = chosen
    forces = rig.forces or (rig.forces_K if kind == "K" else rig.forces_D)

    def device(x32, v32):
        hs.upload(g, x32, v32)
        return forces().astype(np.float64), np.zeros((len(x32), 3))

    q_dev, _, _ = secant(device, rig.x0, phi, a, rig.m, kind)
    rel = carried / q_ref
    err = abs(q_dev / q_ref - 1.0)
    print(f"guards [engine]: spectrum {name} {kind}: a = 2^{int(round(math.log2(a / H0)))} H0, lambda_max {lam:.6g}, float64 secant "
          f"{q_ref / lam:.5f} of it, device / float64 - 1 = {err:.2e}, carried bound {rel:.2e}")
    _margin(f"device secant against float64, {name} {kind}", err / rel if err > 0 else 0.0)
    assert err <= rel, (name, kind, err, rel)
    guard = rig.guard()
    top = 2.0 / math.sqrt(q_dev) if kind == "K" else 2.0 / q_dev
    _margin(f"guard / limit of the device's quotient, {name} {kind}", guard / top)
    assert guard <= top * (1.0 + rel), (name, kind, guard, top)
    assert g.stats()["error_flags"] == 0
    g.destroy()


# ---- 3 -------------------------------------------------------------------------------------------------------------------
def test_the_fan_with_both_bending_models():
    """quadratic and shell bending on the fan, the shell's stiffness sized so that the two guards are equal: the engine
    accepts any dt up to that guard (each feature is tested alone), the true limit of the sum is below it, and
    composed_limit is a stable step"""
    X, T, _ = sb.mesh("fan")
    g = _engine([(X, T)])
    kb = float(F(1e-6))
    g.set_bending([kb])
    gb = g.bending_max_stable_dt()
    g.set_shell_bending([sb.K])
    ks = float(F(sb.K * (g.shell_max_stable_dt() / gb) ** 2))
    g.set_shell_bending([ks])
    gs = g.shell_max_stable_dt()
    assert abs(gs / gb - 1.0) < 1e-5
    m = _masses(g)
    ids, kc, psibar = g.shell_hinges()
    K = gd.sanity(gd.bending_K(kb, X, T)[0]) + gd.sanity(gd.shell_K(X.astype(np.float64), ids.astype(np.int64), kc, psibar))
    limit = gd.true_limit(K, None, m)
    guards = [gb, gs]
    _margin("true limit / min(guard), fan with both bending models", limit / min(guards))
    for dt in (gd.composed_limit(guards), gd.composed_limit_elastic(guards)):
        assert dt <= limit * (1.0 + 1e-6) and gd.spectral_radius(K, None, m, dt) <= 1.0 + gd.RADIUS_TOL
    assert limit < min(guards), (limit, guards)
    g.destroy()


PATCH = 9


def test_a_patch_of_feature_paths_cloth_1():
    """The first 9 x 9 vertices of cloth 1 of tests/feature_paths.py's scene (the second sheet: its jittered positions,
    its rolled rest shape for the shell model, its material), alone on an engine, with the features that scene puts on
    the cloth itself -- quadratic bending, shell bending, membrane and hinge damping --, each sized as there so that DT is
    SHARE = 0.499 of its guard.  composed_limit of the engine's three guards is a stable step for the sum of the
    operators with the engine's masses, and so is the scene's DT.
    NOT the whole cloth: its 1024 vertices make the one-step matrix 6144 x 6144, one nonsymmetric eigenvalue solve of
    which takes more than half a minute, and the bisection needs a dozen.  The patch keeps the spacing, the jitter, the
    curvature of the rest shape and the ratios of the three guards."""
    from drake_amd import scenes
    from tests import feature_paths as fp
    s = fp.scene()
    a, b = s["first"][1], s["first"][2]
    grid = lambda q: np.ascontiguousarray(q[a:b].reshape(fp.RES, fp.RES, 3)[:PATCH, :PATCH].reshape(-1, 3), np.float32)   # noqa: E731
    X, rest = grid(s["X"]), grid(s["rest"])
    T = np.asarray(scenes.sheet_indices(PATCH), np.int32).reshape(-1, 3)
    n = len(X)
    cm = fp.cloth_material(1)
    mats = [dict(youngs_modulus=cm.youngs_modulus, density=cm.density)]
    g = _engine([(X, T)], mats=mats)
    m = _masses(g)
    g.set_bending([1e-5])
    kb = float(F(1e-5 * (fp.SHARE * g.bending_max_stable_dt() / fp.DT) ** 2))
    g.set_bending([kb])
    g.set_shell_bending([1.0], rest)
    ks = float(F((fp.SHARE * g.shell_max_stable_dt() / fp.DT) ** 2))
    g.set_shell_bending([ks], rest)
    g.set_damping([(1.0, 1.0)])
    c = fp.SHARE * g.damping_max_stable_dt() / fp.DT
    betas = np.array([(c, c)], np.float32)
    g.set_damping(betas)
    guards = [g.bending_max_stable_dt(), g.shell_max_stable_dt(), g.damping_max_stable_dt()]
    for q in guards:
        assert abs(fp.DT / q / fp.SHARE - 1.0) < 1e-3, guards
    ids, kc, psibar = g.shell_hinges()
    Kb, H = gd.bending_K(kb, X, T)
    K = gd.sanity(Kb) + gd.sanity(gd.shell_K(rest.astype(np.float64), ids.astype(np.int64), kc, psibar))
    twin = _engine([(X, T)])
    dm, vol = _rest_records(twin)
    twin.destroy()
    mu, lam = _lame32(cm.youngs_modulus, cm.poisson_ratio)
    # (every operator at one state, the shell's rolled rest shape: an isometry of the sheet as added up to the chords of
    # a cylinder of radius 0.5, so the membrane damper sees F = a rotation there, as at its own rest shape)
    D = gd.membrane_D(rest.astype(np.float64), T, dm, vol, mu, lam, betas[0][0]) + gd.kron3(float(betas[0][1]) * kb * bd.q_dense(n, H)[0])
    D = gd.sanity(D)
    dt = gd.composed_limit(guards)
    r = gd.spectral_radius(K, D, m, dt)
    limit = gd.true_limit(K, D, m, start=dt)
    _margin("true limit / min(guard), patch of feature_paths cloth 1", limit / min(guards))
    _margin("composed limit / true limit, patch of feature_paths cloth 1", dt / limit)
    assert r <= 1.0 + gd.RADIUS_TOL, r
    assert gd.spectral_radius(K, D, m, fp.DT) <= 1.0 + gd.RADIUS_TOL
    assert g.stats()["error_flags"] == 0
    g.destroy()
