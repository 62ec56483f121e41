"""Stiffness-proportional damping (mpm_set_damping) on the engine, 64^3 grid.

1. mpm_damping_forces per vertex against the float64 restatement of tests/damping.py (membrane) and tests/bending.py
   (hinges, on the velocities), on every scene x deformation x velocity state, no vertex left out.  Tolerance per
   component: 2^-24 (R Bm_i + (h_i + 5) Bb_i) -- R = 24 from damp_face (mpm_damping.h) on Bm_i, the sum of the bounds of
   the vertex's records (the float sum of the records and the add of the hinge part have to fit into R as well); h_i + 3
   a bending row's count (tests/bending.py) on Bb_i, one more for the product beta c_ij, one for that add.  The same after two short
   substeps that force a re-sort and after mpm_rebuild_mapping(sort = 1); the same state uploaded again gives the same bits.
   The scenes: 288 faces (more than 256, no multiple of it), a fan whose hub has 12 faces (DP::G3), boundary vertices
   everywhere, 1152 faces with bending damping, two cloths one of which is undamped, a multi-material pair.
2. After mpm_calc_fem_state_and_force, MPM_ARR_FORCES of a damped engine minus an undamped twin's is mpm_damping_forces
   within (2 n_i - 1) 2^-24 (sum_j |e_j| + sum_j |d_j|): the damped engine sums fl(e_j + d_j) (one rounding each, n_i),
   the twin e_j, mpm_damping_forces d_j (n_i - 1 roundings of partial sums each, every partial sum below the sum of
   the absolute values); |e_j| from the float64 restatement of the face kernel (tests/fem_regimes.py), |d_j| from the
   float64 records.
3. ParticleToGrid node by node (tests/transfer_layouts.py) from the downloaded total forces, default and deterministic.
4. Scheduling: run_substeps(n) -- whose ParticleToGrid sums the vertex forces itself from DP::VF on this valence-6 sheet,
   and whose gated substeps skip themselves and are run again --, n x substep and the five phase calls are bit-equal
   through several re-sorts; the coupled path runs on a floor.
5. Off means off, to the bit and to the launch count of the re-sort checks.
6. Dynamics against an undamped twin, gravity 0: a rigidly spinning and translating sheet keeps the twin's kinetic energy
   and angular momentum (to the 1e-9 of the sum of the absolute terms that tests/measure.py allows those fields); a
   stretched sheet and a folded sheet with bending lose energy faster than their twins at every sample.
7. Refusals."""
import numpy as np
import pytest

from tests import bending as bd
from tests import damping as dp
from tests import harness as hs
from tests import transfer_layouts as tl

pytestmark = pytest.mark.gpu

U = dp.U
R = dp.rounding_count()
DT = 2e-4              # of the dynamics tests
SHARE = 0.25           # of mpm_damping_max_stable_dt that a test's dt is, where it does not say otherwise
# (the scenes' coefficients and bending stiffnesses are sized for tests/transfer_layouts.py's DT = 1e-3)
UP = np.array([0.0, 0.0, 0.05], np.float32)


def _lame32(E, nu):
    """the engine's float Lame parameters (lame, mpm_cloth_host.h): float32 arithmetic throughout"""
    E, nu, one, two = (np.float32(a) for a in (E, nu, 1.0, 2.0))
    return E / (two * (one + nu)), E * nu / ((one + nu) * (one - two * nu))


# ---- scenes -------------------------------------------------------------------------------------------------------------
# name -> (meshes, per-cloth material overrides or None, bending on per cloth, (membrane, bending) damping on per cloth:
# relative weights, scaled together to a quarter of the limit)
def _big():
    return bd.sheet(25, 25, alternate=True, jitter=0.2, seed=4)


_MATS = (dict(youngs_modulus=2.5e5, poisson_ratio=0.25), dict(youngs_modulus=6e5, density=1300.0))
SCENES = {
    "regular": (("regular",), None, (0,), ((1.0, 0.0),)),
    "fan": (("fan",), None, (0,), ((1.0, 0.0),)),
    "big": (("big",), None, (1,), ((1.0, 1.0),)),
    "pair": (("jittered", "fan"), None, (1, 1), ((1.0, 0.7), (0.0, 0.0))),
    "pair_multi": (("jittered", "regular"), _MATS, (1, 0), ((0.6, 1.0), (1.0, 1.0))),
}
_CACHE = {}


def _meshes(scene):
    out = []
    for k, name in enumerate(SCENES[scene][0]):
        X, T = _big() if name == "big" else bd.mesh(name)
        out.append(((X + k * UP).astype(np.float32), T))
    return out


def _vertex_state(g):
    A = hs.ARR()
    nf = g.n_faces
    pids, v = g.download(A.PIDS), g.download(A.VELOCITIES)
    vv = np.zeros((g.n_verts, 3), np.float32)
    vv[pids[pids >= nf] - nf] = v[pids >= nf]
    return g.dump_cpu_state()[0], vv


def _rest(g):
    """(dm (nf, 3), vol (nf,)) float32 in original face order, of a SINGLE-material engine (whose MPM_ARR_VOLUMES is the
    record the face kernels read)"""
    A = hs.ARR()
    nf = g.n_faces
    pids, vol = g.download(A.PIDS), g.download(A.VOLUMES)
    vf = np.zeros(nf, np.float32)
    vf[pids[pids < nf]] = vol[pids < nf]
    return g.download(A.DM_INVERSES).reshape(nf, 4)[:, [0, 1, 3]].copy(), vf


def _betas_for(g, on, dt=DT, share=SHARE):
    """[(membrane, bending)] = c x `on` such that dt is `share` of mpm_damping_max_stable_dt (the limit is 1 / c)"""
    on = np.asarray(on, np.float64).reshape(-1, 2)
    g.set_damping(on)
    lim = g.damping_max_stable_dt()
    assert np.isfinite(lim) and lim > 0
    d = (on * (share * lim / dt)).astype(np.float32)
    g.set_damping(d)
    got = g.damping_max_stable_dt()
    assert abs(got * share / dt - 1.0) < 1e-3, (got, dt)
    return d


def _scene(scene):
    """the scene's engine-independent data, made once: meshes, per-face cloth, float Lame parameters per cloth, rest
    records, hinges, bending stiffness and damping coefficients"""
    if scene in _CACHE:
        return _CACHE[scene]
    from drake_amd import GpuMpm
    _, mats, bend_on, damp_on = SCENES[scene]
    meshes = _meshes(scene)
    base = GpuMpm.default_material()
    lame = []
    for c in range(len(meshes)):
        m = dict(youngs_modulus=base.youngs_modulus, poisson_ratio=base.poisson_ratio)
        m.update({k: v for k, v in (mats[c] if mats else {}).items() if k in m})
        lame.append(_lame32(m["youngs_modulus"], m["poisson_ratio"]))
    single = hs.engine(meshes)                     # (rest records: Finalize's geometry does not depend on the material)
    rest = _rest(single)
    single.destroy()
    g = hs.engine(meshes, mats=mats)
    ks = [0.0] * len(meshes)
    if any(bend_on):
        g.set_bending([float(b) for b in bend_on])
        ks = [float(np.float32((0.25 * g.bending_max_stable_dt() / tl.DT) ** 2)) * b for b in bend_on]
        g.set_bending(ks)
    betas = _betas_for(g, damp_on, dt=tl.DT)
    g.destroy()
    cloth_of_face = np.concatenate([np.full(len(T), c) for c, (_, T) in enumerate(meshes)])
    first = np.cumsum([0] + [len(X) for X, _ in meshes])
    hinges = []
    for (X, T), k, b in zip(meshes, ks, betas):
        if k > 0 and b[1] > 0:
            H = bd.hinges(X, T)
            hinges.append((H, bd.q_dense(len(X), H)[1]))
        else:
            hinges.append(None)
    X0 = np.concatenate([X for X, _ in meshes])
    T0 = np.concatenate([T + o for (_, T), o in zip(meshes, first)])
    _CACHE[scene] = dict(meshes=meshes, mats=mats, lame=lame, rest=rest, ks=ks, betas=betas, cof=cloth_of_face, first=first,
                         hinges=hinges, X=X0, T=T0)
    return _CACHE[scene]


def _prepared(scene, **kw):
    s = _scene(scene)
    g = hs.engine(s["meshes"], mats=s["mats"], **kw)
    if any(s["ks"]):
        g.set_bending(s["ks"])
    g.set_damping(s["betas"])
    assert np.array_equal(g.get_damping(), s["betas"])
    return g, s


def _reference(s, x, v):
    """(f64 (n, 3), tolerance (n, 3)) of the damping force on float32 vertex positions and velocities"""
    T, cof = s["T"], s["cof"]
    mu = np.array([s["lame"][c][0] for c in cof], np.float32)
    lam = np.array([s["lame"][c][1] for c in cof], np.float32)
    beta = np.array([s["betas"][c][0] for c in cof], np.float32)
    f, Bm = dp.forces64(s["X"], T, x, v, (mu, lam), beta, rest=s["rest"])
    tol = U * R * Bm
    for c, hp in enumerate(s["hinges"]):
        if hp is None:
            continue
        H, P = hp
        a, b = s["first"][c], s["first"][c + 1]
        kb = float(np.float32(s["betas"][c][1])) * float(np.float32(s["ks"][c]))
        f[a:b] += bd.force64(kb, H, v[a:b])
        tol[a:b] += (U * (bd.rounding_count(P) + 2.0) * bd.bound(kb, H, v[a:b]))[:, None]
    return f, tol


def _check_forces(g, s, what):
    x, v = _vertex_state(g)
    f = g.damping_forces()
    ref, tol = _reference(s, x, v)
    err = np.abs(f.astype(np.float64) - ref)
    w = float(np.where(err == 0, 0.0, err / np.maximum(tol, 1e-300)).max())
    print(f"damping forces: {what}: {w:.3g} of the tolerance")
    hs.record(f"damping forces: {what}", w)
    assert w <= 1.0, (what, w)
    return x, v, f, ref


def _states(s, st, vn):
    x = np.concatenate([bd.state(st, X) for X, _ in s["meshes"]]).astype(np.float32)
    return x, dp.velocity(vn, x).astype(np.float32)


# ---- 1 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", list(SCENES))
def test_forces_against_float64(scene):
    g, s = _prepared(scene)
    assert g.cloth_count() == len(s["meshes"])
    undamped = np.concatenate([np.full(len(X), not (b[0] > 0 or (b[1] > 0 and k > 0)))
                               for (X, _), b, k in zip(s["meshes"], s["betas"], s["ks"])])
    for st in bd.STATES:
        for vn in dp.VELOCITIES:
            x0, v0 = _states(s, st, vn)
            hs.upload(g, x0, v0)
            x, v, f, ref = _check_forces(g, s, f"{scene} {st} {vn}")
            assert np.array_equal(x, x0) and np.array_equal(v, v0)
            assert not f[undamped].any()
            if vn in ("dilation", "shear", "random"):
                assert np.all(np.abs(f[~undamped]).max(axis=1) > 0), "a vertex was left out"
    # substeps that force a re-sort: the state five cells further along x, two short substeps
    x0, v0 = _states(s, "cylinder30", "random")
    hs.upload(g, x0, v0)
    f0 = g.damping_forces()
    before = g.stats()["rebuilds"]
    hs.upload(g, x0 + np.array([5.0 / 64, 0.0, 0.0], np.float32), v0)
    g.run_substeps(2, 1e-5, -1)
    g.gpu_sync()
    assert g.stats()["error_flags"] == 0 and g.stats()["rebuilds"] > before, g.stats()
    _check_forces(g, s, f"{scene} after a re-sort")
    # the first state again, in the new particle order: the same bits
    hs.upload(g, x0, v0)
    f1 = g.damping_forces()
    assert np.array_equal(hs.bits(f1), hs.bits(f0)), float(np.abs(f1 - f0).max())
    g.rebuild_mapping(True)
    _check_forces(g, s, f"{scene} after sort = 1")
    assert np.array_equal(hs.bits(g.damping_forces()), hs.bits(f0))
    assert g.stats()["error_flags"] == 0
    g.destroy()


def test_more_than_256_cloths():
    """A single-material engine holds any number of cloths: 300 two-face strips, every third one damped, cloths 0 and 256
    (and 1 and 257, ...) with different settings.  Forces per vertex against float64 within R 2^-24 bound, exact zeros on
    the undamped cloths, and the guard against its float64 restatement."""
    X0, T0 = bd.mesh("strip")
    n = 300
    meshes = []
    for c in range(n):
        off = np.array([(c % 20 - 9.5) * 2.5 * bd.H0, (c // 20 - 7.0) * 2.5 * bd.H0, 0.0])
        meshes.append(((X0.astype(np.float64) + off).astype(np.float32), T0))
    g = hs.engine(meshes)
    assert g.cloth_count() == n
    on = np.zeros((n, 2))
    on[::3, 0] = 1.0 + (np.arange(0, n, 3) % 7) / 7.0
    assert on[0, 0] > 0 and on[256, 0] == 0 and on[1, 0] == 0 and on[258, 0] > 0
    betas = _betas_for(g, on, dt=tl.DT)
    rest = _rest(g)
    lame = _lame32(g.default_material().youngs_modulus, g.default_material().poisson_ratio)
    X = np.concatenate([m[0] for m in meshes])
    T = np.concatenate([T0 + 4 * c for c in range(n)])
    x = bd.state("perturbed", X)
    v = dp.velocity("random", x).astype(np.float32)
    hs.upload(g, x, v)
    f = g.damping_forces()
    beta_f = np.repeat(betas[:, 0], 2)
    ref, B = dp.forces64(X, T, x, v, lame, beta_f, rest=rest)
    w = dp.margin(f - ref, B, R)
    hs.record("damping forces: 300 cloths", w)
    assert w <= 1.0, w
    damped = np.repeat(betas[:, 0] > 0, 4)
    assert not f[~damped].any() and np.all(np.abs(f[damped]).max(axis=1) > 0)
    lim = _guard64(g, T, rest, [lame] * n, betas, np.repeat(np.arange(n), 2))
    assert abs(g.damping_max_stable_dt() / lim - 1.0) < 1e-6, (g.damping_max_stable_dt(), lim)
    assert g.stats()["error_flags"] == 0
    g.destroy()


def _guard64(g, T, rest, lame, betas, cof, hinges=None, ks=None, first=None):
    """tests/damping.py's guard64 on the vertex particles' MPM_ARR_MASSES"""
    A = hs.ARR()
    nf = g.n_faces
    pids, m = g.download(A.PIDS), g.download(A.MASSES).astype(np.float64)
    mv = np.zeros(g.n_verts)
    mv[pids[pids >= nf] - nf] = m[pids >= nf]
    return dp.guard64(mv, T, rest, lame, betas, cof, hinges, ks, first)


@pytest.mark.parametrize("scene", ["big", "pair_multi"])
def test_guard_against_the_formula(scene):
    """mpm_damping_max_stable_dt against the documented Gershgorin expression in float64, from DM_INVERSES, the rest
    volumes, MPM_ARR_MASSES and the float Lame parameters: a single-material scene with bending damping, and the
    multi-material pair (per-cloth Lame parameters and densities; the engine's q[0].w holds masses there).  1e-6: the
    engine forms the same sums in double from the same floats and rounds the result to float, towards zero."""
    g, s = _prepared(scene)
    lim = _guard64(g, s["T"], s["rest"], s["lame"], s["betas"], s["cof"], s["hinges"], s["ks"], s["first"])
    got = g.damping_max_stable_dt()
    print(f"guard {scene}: engine {got:.9g}, formula {lim:.9g}")
    assert abs(got / lim - 1.0) < 1e-6, (got, lim)
    # each part alone, against the formula again (neither allows a shorter step than both)
    for part in (0, 1):
        d = s["betas"].copy()
        d[:, 1 - part] = 0.0
        g.set_damping(d)
        lim1 = _guard64(g, s["T"], s["rest"], s["lame"], d, s["cof"], s["hinges"], s["ks"], s["first"])
        got1 = g.damping_max_stable_dt()
        assert abs(got1 / lim1 - 1.0) < 1e-6 and got1 >= got, (part, got1, lim1)
    g.destroy()


def test_device_records_are_the_host_function_bits():
    """One cloth of 64 disjoint triangles: every vertex has one face, so mpm_damping_forces is minus the record k_damp_eval
    wrote (0 - G, exact) and can be compared with mpm_damping_face_records -- damp_face compiled for the host -- value for
    value.  (k_damp calls the same device function on the same loads as k_damp_eval.)"""
    from drake_amd import damping_face_records
    r = np.random.default_rng(9)
    X0, T0 = bd.mesh("triangle")
    n = 64
    X = np.concatenate([(X0.astype(np.float64) + np.array([(c % 8 - 3.5) * 2 * bd.H0, (c // 8 - 3.5) * 2 * bd.H0, 0.0])) for c in range(n)])
    X = (X + 0.1 * bd.H0 * r.normal(size=X.shape) * np.array([1, 1, 0])).astype(np.float32)
    T = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    g = hs.engine([(X, T)])
    betas = _betas_for(g, [(1.0, 0.0)], dt=tl.DT)
    rest = _rest(g)
    mu, lam = _lame32(g.default_material().youngs_modulus, g.default_material().poisson_ratio)
    for st in bd.STATES:
        x = bd.state(st, X)
        v = dp.velocity("random", x).astype(np.float32)
        hs.upload(g, x, v)
        f = g.damping_forces()
        rec = damping_face_records(rest[0], rest[1], mu, lam, betas[0][0], dp.corners(T, x), dp.corners(T, v))
        assert np.abs(rec).max() > 0
        assert np.array_equal(f.reshape(n, 3, 3), -rec), (st, float(np.abs(f.reshape(n, 3, 3) + rec).max()))
    g.destroy()


# ---- 2 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["regular", "fan", "pair_multi"])
def test_total_forces_include_damping(scene):
    """(the fan's hub has 12 faces: its records go through DP::G3 and the adjacency walk, the others through DP::VF;
    pair_multi runs k_fem_mat; membrane damping only, so that the vertex force is one sum of records)"""
    from tests import fem_regimes as fr
    A = hs.ARR()
    s = _scene(scene)
    betas = s["betas"].copy()
    betas[:, 1] = 0.0
    a, b = hs.engine(s["meshes"], mats=s["mats"]), hs.engine(s["meshes"], mats=s["mats"])
    a.set_damping(betas)
    x0, v0 = _states(s, "affine", "random")
    nf, T = len(s["T"]), s["T"]
    out = []
    for g in (a, b):
        hs.upload(g, x0, v0)
        F_up = g.download(A.DEFORMATION_GRADIENTS)
        g.rebuild_mapping(False)
        g.calc_fem_state_and_force(tl.DT)
        f, pids = g.download(A.FORCES), g.download(A.PIDS)
        fv = np.zeros((len(x0), 3), np.float32)
        fv[pids[pids >= nf] - nf] = f[pids >= nf]
        out.append(fv)
    fd = a.damping_forces()
    assert fd.any() and out[1].any()
    # magnitudes of the records: elastic from the float64 face kernel, damping from the float64 records
    base = a.default_material()
    xc, vc = dp.corners(T, x0), dp.corners(T, v0)
    dm4 = a.download(A.DM_INVERSES).reshape(nf, 4)
    E = np.zeros((nf, 3, 3))
    for c in range(len(s["meshes"])):
        m = dict(fr.DEFAULT)
        m.update({k: getattr(base, k) for k in ("youngs_modulus", "poisson_ratio", "gamma", "K", "c_F")})
        m.update({k: v for k, v in (s["mats"][c] if s["mats"] else {}).items() if k in m})
        sel = s["cof"] == c
        E[sel] = fr.face64(fr.Mat(m), F_up[sel].astype(np.float64), np.zeros((int(sel.sum()), 9)), xc[sel].astype(np.float64),
                           dm4[sel].astype(np.float64), s["rest"][1][sel])["force"]
    mu = np.array([s["lame"][c][0] for c in s["cof"]], np.float32)
    lam = np.array([s["lame"][c][1] for c in s["cof"]], np.float32)
    beta = np.array([betas[c][0] for c in s["cof"]], np.float32)
    D = dp.records64(s["rest"][0], s["rest"][1], mu, lam, beta, xc, vc)
    mag = -dp.vertex_sum(T, len(x0), np.abs(E) + np.abs(D))
    n = dp.valence(T, len(x0))
    tol = (2.0 * n - 1.0)[:, None] * U * mag * (1.0 + 1e-3)     # (1e-3: the magnitudes are float64 values of float sums)
    err = np.abs(out[0].astype(np.float64) - out[1].astype(np.float64) - fd.astype(np.float64))
    w = float(np.where(err == 0, 0.0, err / np.maximum(tol, 1e-300)).max())
    print(f"total forces: {scene}: {w:.3g} of the tolerance; |damping| / |elastic| = {np.abs(fd).max() / np.abs(out[1]).max():.3g}")
    hs.record(f"damping: total forces {scene}", w)
    assert w <= 1.0, w
    assert np.abs(fd).max() > 1e3 * tol.max(), "the damping force is far above the tolerance"
    assert not b.damping_forces().any() and b.damping_max_stable_dt() == np.inf
    for g in (a, b):
        assert g.stats()["error_flags"] == 0
        g.destroy()


# ---- 3 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["default", "deterministic"])
def test_p2g_node_by_node(mode):
    from tests import helpers
    helpers.tag_default_engine(mode == "default")
    A = hs.ARR()
    s = _scene("regular")
    nf = len(s["T"])
    g = hs.engine(s["meshes"], deterministic=mode == "deterministic")
    _betas_for(g, [(1.0, 0.0)], dt=tl.DT)
    x0, v0 = _states(s, "affine", "shear")
    hs.upload(g, x0, 0.1 * v0)
    g.rebuild_mapping(False)
    g.calc_fem_state_and_force(tl.DT)
    d = {k: g.download(a) for k, a in (("pids", A.PIDS), ("x", A.POSITIONS), ("v", A.VELOCITIES), ("C", A.AFFINE),
                                       ("m", A.MASSES), ("taus", A.TAUS), ("f", A.FORCES))}
    fd = g.damping_forces()
    g.particle_to_grid(tl.DT)
    gm, gmv, flags = g.download(A.GRID_MASSES), g.download(A.GRID_MOMENTUM), g.download(A.GRID_TOUCHED_FLAGS)
    assert g.stats()["error_flags"] == 0
    g.destroy()
    face = d["pids"] < nf
    taus = np.where(face[:, None], d["taus"], 0.0)
    f = np.where(face[:, None], 0.0, d["f"])
    r = tl.p2g64(d["x"], d["v"], d["C"], d["m"], taus, f, 6, 2)
    bm, bmv = tl.p2g_bounds(r, tl.fixed_quanta(d["m"]) if mode != "default" else None)
    for field, err, bnd in (("mass", np.abs(gm - r["m"]), bm), ("momentum", np.abs(gmv - r["mv"]), bmv)):
        w = tl.margin(err, bnd)
        print(f"damping p2g [{mode}] {field}: {w:.4g} of the bound")
        hs.record(f"damping: p2g [{mode}] {field}", w)
        assert w <= 1.0, (field, w)
    assert np.array_equal(flags, r["flags"])
    # damping is in the sums: without it the momentum is outside the bound
    fv = f.copy()
    fv[~face] -= fd[d["pids"][~face] - nf]
    r0 = tl.p2g64(d["x"], d["v"], d["C"], d["m"], taus, fv, 6, 2)
    assert tl.margin(np.abs(gmv - r0["mv"]), bmv) > 10


# ---- 4 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["regular", "big"])
def test_scheduling_through_resorts(scene):
    """a strained sheet that flies through several re-sorts, deterministic: run_substeps(n), n x substep and n x the five
    phase calls give the same bits in x, v, C and F -- a force added twice under the gate, or missing from the vertex
    forces ParticleToGrid sums itself (regular: no bending, every valence <= 8), would not.  big: with bending damping.
    Substeps of the batches do skip themselves and are run again with k_damp / k_bend_damp in them: Ctl::skipped is read
    (mpm_debug_owed_substeps) after every batch."""
    n = 60
    es = [_prepared(scene)[0] for _ in range(3)]
    s = _scene(scene)
    x0, v0 = _states(s, "cylinder30", "dilation")
    v0 = (0.05 * v0 + np.array([3.0, 0.4, 0.0], np.float32)).astype(np.float32)
    for g in es:
        hs.upload(g, x0, v0)
    before = es[0].stats()["rebuilds"]
    # (in batches of 10, so that the substeps that skipped themselves can be counted before the next call runs them again)
    # One single substep first: it carries its re-sort launches and moves the engine's count of substeps by one, so that
    # the batches' check launches (every 4th substep) are out of step with the re-sort cadence of a sheet in uniform motion.
    es[0].substep(tl.DT, -1)
    replayed = 0
    for k in (9, 10, 10, 10, 10, 10):
        es[0].run_substeps(k, tl.DT, -1)
        replayed += es[0].owed_substeps()
    print(f"scheduling {scene}: {replayed} substeps skipped themselves and were run again")
    # (asserted on the large sheet, which runs k_damp and k_bend_damp both; the 13 x 13 sheet happens never to find a
    # re-sort pending in a substep without check launches on this trajectory -- 0 on an MI355X, with either offset)
    assert replayed > 0 or scene != "big", "no substep of the batches was gated out and run again"
    for _ in range(n):
        es[1].substep(tl.DT, -1)
    for _ in range(n):
        g = es[2]
        g.rebuild_mapping(False)
        g.calc_fem_state_and_force(tl.DT)
        g.particle_to_grid(tl.DT)
        g.update_grid(-1)
        g.grid_to_particle(tl.DT)
    for g in es:
        g.gpu_sync()
        assert g.stats()["error_flags"] == 0, g.stats()
    assert es[0].stats()["rebuilds"] - before >= 3, es[0].stats()
    st = [hs.state(g) for g in es]
    hs.same_bits(st[0], st[1], "run_substeps(n) against n substeps")
    hs.same_bits(st[0], st[2], "run_substeps(n) against the phase calls")
    assert es[0].damping_forces().any()
    for g in es:
        g.destroy()


def test_coupled_path_runs():
    from drake_amd import Collider
    g, s = _prepared("regular", bodies=1)
    x0, v0 = _states(s, "cylinder30", "dilation")
    hs.upload(g, x0, 0.05 * v0)
    floor = [Collider(0, body=0, p_WB=(0.5, 0.5, float(x0[:, 2].min()) - 0.002))]
    res = g.run_coupled_substeps(40, tl.DT, floor, 0.5, 1e5, 1e-4)
    g.gpu_sync()
    assert g.stats()["error_flags"] == 0
    assert max(r["contacts"] for r in res) > 0, "the sheet never reached the floor"
    assert np.isfinite(g.download(hs.ARR().VELOCITIES)).all()
    g.destroy()


# ---- 5 -------------------------------------------------------------------------------------------------------------
def test_off_means_off():
    """20 deterministic substeps through re-sorts: never set == all zeros == set and cleared with (h, 0, NULL), to the bit
    in x, v, C and F, and with the same launch counters (mpm_stats: substeps, re-sorts, re-sort check launches -- the
    quiet-time hint is in use again)"""
    from drake_amd import scenes
    pos, idx = scenes.cloth_sheet(32, 0.3, 0.6, (0.3, 0.5))
    es = [hs.engine([(pos, idx.reshape(-1, 3))]) for _ in range(3)]
    es[1].set_damping([(0.0, 0.0)])
    es[2].set_damping([(1e-5, 1e-5)])
    assert es[2].damping_max_stable_dt() < np.inf
    es[2].set_damping([])
    for g in es:
        assert not g.get_damping().any() and g.damping_max_stable_dt() == np.inf and not g.damping_forces().any()
    vel = np.array([4.0, 0.3, 0.0], np.float32) + 0.05 * np.random.default_rng(3).normal(size=pos.shape).astype(np.float32)
    before = es[0].stats()["rebuilds"]
    for g in es:
        pids = g.download(hs.ARR().PIDS)
        allv = np.concatenate([vel[g._tri].mean(axis=1), vel]).astype(np.float32)
        g.upload_particle_state(None, allv[pids], None, None, None)
        for _ in range(2):
            g.run_substeps(10, tl.DT, -1)
        g.gpu_sync()
        assert g.stats()["error_flags"] == 0
    assert es[0].stats()["rebuilds"] - before >= 1, es[0].stats()
    st = [hs.state(g) for g in es]
    hs.same_bits(st[0], st[1], "all zeros")
    hs.same_bits(st[0], st[2], "set and cleared")
    for k in ("substeps", "rebuilds", "resort_checks"):
        assert es[0].stats()[k] == es[1].stats()[k] == es[2].stats()[k], k
    for g in es:
        g.destroy()


# ---- 6 -------------------------------------------------------------------------------------------------------------
def _energy(total):
    return float(total["kinetic"] + total["kinetic_affine"] + total["elastic_in_plane"] + total["elastic_normal"] +
                 total["elastic_shear"] + total["bending"])


def test_rigid_motion_is_not_damped():
    """The regular sheet at rest shape, spinning in its plane about its centre (1/8 rad / s) while it translates
    (0.5, 0.25, 0), gravity 0, DT a twentieth of mpm_damping_max_stable_dt, N = 1 substep; kinetic energy and angular
    momentum of mpm_measure against the twin's, within the 1e-9 of the sum of the absolute terms that tests/measure.py
    allows those fields.
    Why one substep, and these numbers.  That tolerance is sixty times finer than the float32 resolution of a velocity
    (2^-24), so it can only hold while the two trajectories are the same floats almost everywhere -- while the damping
    force is zero not to rounding but exactly.  Here it is: the rest positions are multiples of 2^-8 about the centre,
    the spin and the translation powers of two, so every uploaded velocity IS the rigid field, every difference and
    every product of Edot is exact and the terms cancel to zero.  From the second substep on the velocities are
    generic floats that carry the rigid field with an error of half a last bit (3e-8); to the kernel that is a strain
    rate at the scale of the mesh like any other, and the damper takes its share of it, a tenth of a last bit per
    substep, so that about a tenth of the 1371 velocity components round the other way in every substep.  Measured on
    an MI355X: N = 2 gives 6.2e-9 of the kinetic energy and 3.4e-9 of the angular momentum's absolute terms, N = 10
    1e-8 to 5e-8 and 1e-8 to 1e-7 (spins of 1/8, 1/2 and 2 rad / s, a twentieth and a quarter of the limit alike) --
    what two float32 trajectories that differ at all differ by, not a loss: the sign varies.  The spin is slow because
    a sheet that spins at its rest shape is not in equilibrium: the centripetal acceleration w^2 r strains it, and the
    damper rightly acts on that.  A kernel that damped rigid rotation would take a share-sized fraction of the
    rotation's kinetic energy (2e-4 of the total) in the one substep: 1e4 tolerances."""
    s = _scene("regular")
    mat = dict(gravity=0.0)
    a, b = hs.engine(s["meshes"], material=mat), hs.engine(s["meshes"], material=mat)
    _betas_for(a, [(1.0, 0.0)], share=0.05)
    X = s["X"].astype(np.float64)
    w, v0 = np.array([0.0, 0.0, 0.125]), np.array([0.5, 0.25, 0.0])
    v = (v0 + np.cross(w, X - bd.CENTER)).astype(np.float32)
    for g in (a, b):
        hs.upload(g, s["X"], v)
        g.run_substeps(1, DT, -1)
        g.gpu_sync()
        assert g.stats()["error_flags"] == 0
    ta, tb = a.measure()[1], b.measure()[1]
    # the sums of the absolute terms, as tests/measure.py forms them (a face at the mean of its corners)
    A = hs.ARR()
    pids, m = b.download(A.PIDS), b.download(A.MASSES).astype(np.float64)
    mo = np.zeros(len(m))
    mo[pids] = m
    xv, vv = (q.astype(np.float64) for q in _vertex_state(b))
    Xp, Vp = np.concatenate([xv[s["T"]].mean(axis=1), xv]), np.concatenate([vv[s["T"]].mean(axis=1), vv])
    i, j = (1, 2, 0), (2, 0, 1)
    abs_L = (mo[:, None] * (np.abs(Xp[:, i] * Vp[:, j]) + np.abs(Xp[:, j] * Vp[:, i]))).sum(axis=0)
    wk = abs(float(ta["kinetic"]) - float(tb["kinetic"])) / (1e-9 * float(tb["kinetic"]))
    wl = float((np.abs(np.asarray(ta["angular_momentum"]) - np.asarray(tb["angular_momentum"])) / (1e-9 * abs_L)).max())
    print(f"rigid motion: kinetic {wk:.3g}, angular momentum {wl:.3g} of 1e-9 of the absolute terms")
    hs.record("damping: rigid motion, kinetic energy", wk)
    hs.record("damping: rigid motion, angular momentum", wl)
    assert float(tb["kinetic"]) > 0 and abs(float(tb["angular_momentum"][2])) > 0
    assert wk <= 1.0 and wl <= 1.0, (wk, wl)
    # Ten substeps: the damper now sees rounded rigid fields in a running engine.  The two float32 trajectories may
    # differ in the last bits of every velocity; allowing each component four of them, all to one side, the kinetic
    # energy may differ by 8 x 2^-24 of itself and the angular momentum by 8 x 2^-24 of its absolute terms (4.8e-7).  A
    # kernel that damped the rotation would take a share-sized fraction of its energy, 2e-4 of the total, per substep.
    for g in (a, b):
        g.run_substeps(9, DT, -1)
        g.gpu_sync()
        assert g.stats()["error_flags"] == 0
    ta, tb = a.measure()[1], b.measure()[1]
    wk = abs(float(ta["kinetic"]) - float(tb["kinetic"])) / (8 * U * float(tb["kinetic"]))
    wl = float((np.abs(np.asarray(ta["angular_momentum"]) - np.asarray(tb["angular_momentum"])) / (8 * U * abs_L)).max())
    print(f"rigid motion, 10 substeps: kinetic {wk:.3g}, angular momentum {wl:.3g} of 8 x 2^-24 of the absolute terms")
    hs.record("damping: rigid motion after 10 substeps, kinetic energy", wk)
    hs.record("damping: rigid motion after 10 substeps, angular momentum", wl)
    assert wk <= 1.0 and wl <= 1.0, (wk, wl)
    for g in (a, b):
        g.destroy()


def _inscribed_cylinder(X, radius, h):
    """the regular sheet folded along its grid lines onto a cylinder (tests/test_bending_gpu.py): every triangle
    congruent to its rest triangle"""
    X = np.asarray(X, np.float64)
    i = np.rint((X[:, 0] - X[:, 0].min()) / h)
    th = (i - 0.5 * i.max()) * 2.0 * np.arcsin(h / (2.0 * radius))
    return np.stack([bd.CENTER[0] + radius * np.sin(th), X[:, 1], bd.CENTER[2] + radius * (1.0 - np.cos(th))], 1)


def _frames(x, T):
    x = np.asarray(x, np.float64)
    d1, d2 = x[T[:, 1]] - x[T[:, 0]], x[T[:, 2]] - x[T[:, 0]]
    n = np.cross(d1, d2)
    n /= np.linalg.norm(n, axis=1)[:, None]
    return np.stack([d1, d2, n], axis=2)


@pytest.mark.parametrize("case", ["stretched", "folded"])
def test_released_sheet_loses_energy(case):
    """Gravity 0, a 13 x 13 sheet released from rest, damped engine and undamped twin, 24 substeps phase by phase, the
    report sampled every 4.
    stretched: the regular sheet with a uniform in-plane stretch of 3 % about the centre; beta_membrane such that DT is a
    quarter of mpm_damping_max_stable_dt.
    folded: a sheet with a vertex spacing of ONE cell (1 / 64) on the inscribed cylinder of radius 6 spacings, without
    membrane strain; bending stiffness such that DT is a quarter of mpm_bending_max_stable_dt, beta_bending alone, DT a
    quarter of the damping limit.  The spacing is chosen so that the grid resolves the hinge forces.  The engine's own
    dissipation -- the momentum a vertex shares with its neighbours through the grid -- is large where the force varies
    below the cell size, and it falls with the speed of the motion, which the damper lowers: on the half-cell sheets of the
    other tests the twin loses 1.4 % of its energy in 16 substeps, a hundred times the damper's work (9e-7 of 1.0e-2),
    and the damped sheet's energy is below the twin's only from substep 3 to 9 (by up to 6e-8) and above it from
    substep 10 on (by 1.9e-7 at 16); a sharp crease behaves like that at either spacing.  On this sheet the damped
    energy stays below, by 5e-6 of 1.66e-1 after 4 substeps and 2.0e-4 after 24 (measured on an MI355X).
    * At every sample (substeps 4, 8, ..., 24) the damped engine's kinetic + strain energy is below the twin's.
    * Linear momentum stays at the twin's: what the substeps add -- the change of sum m v from after the FEM call to after
      GridToParticle (the FEM call itself resets the face particles' velocities, in either engine; see
      tests/test_bending_gpu.py) -- stays, in each engine, within steps x (128 u sum m |v| + dt u sum_i F_i): the transfers
      round a particle's 27 contributions twice (128 u covers both, as there), and the internal forces sum to zero
      within the roundings of their records, F_i = 64 x the sum of the absolute elastic and damping records at vertex i
      at the start (the strain only relaxes from there; 64 roundings is more than either face kernel's chain) plus the
      bending rows' own bounds."""
    from tests import fem_regimes as fr
    A = hs.ARR()
    h = bd.H0 if case == "stretched" else 1.0 / 64
    X, T = bd.sheet(13, 13, h=h)
    steps, every = 24, 4
    mat = dict(gravity=0.0)
    a, b = hs.engine([(X, T)], material=mat), hs.engine([(X, T)], material=mat)
    rest = _rest(a)
    lame = _lame32(a.default_material().youngs_modulus, a.default_material().poisson_ratio)
    F = None
    if case == "stretched":
        x0 = ((X.astype(np.float64) - bd.CENTER) * np.array([1.03, 1.03, 1.0]) + bd.CENTER).astype(np.float32)
        betas = _betas_for(a, [(1.0, 0.0)])
        ks = [0.0]
    else:
        x0 = _inscribed_cylinder(X, 6 * h, h).astype(np.float32)
        rot = _frames(x0, T) @ np.linalg.inv(_frames(X, T))
        F = (rot @ a.download(A.DEFORMATION_GRADIENTS).reshape(-1, 3, 3).astype(np.float64)).astype(np.float32).reshape(-1, 9)
        a.set_bending([1.0])
        ks = [float(np.float32((0.25 * a.bending_max_stable_dt() / DT) ** 2))]
        for g in (a, b):
            g.set_bending(ks)
        betas = _betas_for(a, [(0.0, 1.0)])
    assert DT <= a.damping_max_stable_dt() and DT <= a.bending_max_stable_dt()
    for g in (a, b):
        hs.upload(g, x0, None, F)
    # F_i at the start
    F_up = a.download(A.DEFORMATION_GRADIENTS).astype(np.float64)
    base = a.default_material()
    m = dict(fr.DEFAULT)
    m.update({k: getattr(base, k) for k in ("youngs_modulus", "poisson_ratio", "gamma", "K", "c_F")})
    xc = dp.corners(T, x0)
    E = fr.face64(fr.Mat(m), F_up, np.zeros((len(T), 9)), xc.astype(np.float64),
                  a.download(A.DM_INVERSES).reshape(-1, 4).astype(np.float64), rest[1])["force"]
    Fi = 64.0 * -dp.vertex_sum(T, len(X), np.abs(E))
    H = bd.hinges(X, T)
    P = bd.q_dense(len(X), H)[1]

    def momentum(g):
        mm, v = g.download(A.MASSES).astype(np.float64), g.download(A.VELOCITIES).astype(np.float64)
        return (mm[:, None] * v).sum(axis=0), float((mm[:, None] * np.abs(v)).sum(axis=0).max())

    samples = {0: [], 1: []}
    added, gross, extra = [np.zeros(3), np.zeros(3)], [0.0, 0.0], [0.0, 0.0]
    for k in range(steps):
        for e, g in enumerate((a, b)):
            g.rebuild_mapping(False)
            g.calc_fem_state_and_force(DT)
            p0, _ = momentum(g)
            if e == 0:      # the damping records' bounds on the state the force was formed on
                xv, vv = _vertex_state(g)
                if case == "stretched":
                    _, Bd = dp.forces64(X, T, xv, vv, lame, betas[0][0], rest=rest)
                    extra[0] = max(extra[0], 64.0 * float(Bd.sum(axis=0).max()))
                else:
                    kb = float(betas[0][1]) * ks[0]
                    extra[0] = max(extra[0], float((bd.rounding_count(P) * bd.bound(kb, H, vv)).sum()))
            g.particle_to_grid(DT)
            g.update_grid(-1)
            g.grid_to_particle(DT)
            p1, g1 = momentum(g)
            added[e] += p1 - p0
            gross[e] = max(gross[e], g1)
            if (k + 1) % every == 0:
                samples[e].append(_energy(g.measure()[1]))
    for g in (a, b):
        g.gpu_sync()
        assert g.stats()["error_flags"] == 0
    print(f"{case}: energy damped {['%.4e' % q for q in samples[0]]}")
    print(f"{case}: energy twin   {['%.4e' % q for q in samples[1]]}")
    bend_rows = 0.0
    if case == "folded":
        bend_rows = float((bd.rounding_count(P) * bd.bound(ks[0], H, x0)).sum())
    for e, name in enumerate(("damped", "twin")):
        bound = steps * (128 * U * gross[e] + DT * U * (float(Fi.sum(axis=0).max()) + bend_rows + extra[e]))
        mom = float(np.abs(added[e]).max())
        print(f"{case}: momentum added by the substeps, {name}: {mom:.3e}, bound {bound:.3e}, gross {gross[e]:.3e}")
        hs.record(f"damping: momentum of the {case} sheet, {name}", mom / bound)
        assert gross[e] > 0 and mom <= bound, (name, mom, bound)
    for g in (a, b):
        g.destroy()
    for k in range(len(samples[0])):      # (every sample is after the first substep)
        assert samples[0][k] < samples[1][k], (case, k, samples[0][k], samples[1][k])


# ---- 7 -------------------------------------------------------------------------------------------------------------
def test_refusals():
    from drake_amd import Collider, GpuMpm, MpmError

    def refused(call, says=None):
        with pytest.raises(MpmError) as e:
            call()
        assert e.value.code == -1, e.value
        if says:
            assert says in str(e.value), e.value

    X, T = bd.mesh("regular")
    # before Finalize
    g0 = GpuMpm(6)
    g0.add_qr_cloth(X, np.zeros_like(X), T)
    refused(lambda: g0.set_damping([(1e-4, 0.0)]), says="finalize")
    g0.destroy()

    g = hs.engine([(X, T)], bodies=1)
    g.set_damping([(0.0, 1e-3)])        # bending damping on a cloth without bending stiffness: accepted, does nothing
    assert not g.damping_forces().any() and np.array_equal(g.get_damping(), np.array([(0.0, 1e-3)], np.float32))
    good = _betas_for(g, [(1.0, 0.0)], dt=tl.DT, share=0.9)
    lim = g.damping_max_stable_dt()
    s = _scene("regular")
    x0, v0 = _states(s, "cylinder30", "shear")
    hs.upload(g, x0, 0.1 * v0)
    f_before = g.damping_forces()
    for bad in ([(-1e-5, 0.0)], [(0.0, -1e-5)], [(np.nan, 0.0)], [(0.0, np.inf)], [(1e-5, 0.0), (1e-5, 0.0)]):
        refused(lambda bad=bad: g.set_damping(bad))
    assert np.array_equal(g.get_damping(), good) and g.damping_max_stable_dt() == lim
    assert np.array_equal(hs.bits(g.damping_forces()), hs.bits(f_before))
    # partitioned, halo, team and chain calls on an engine with damping
    nb = 64 // 4
    refused(lambda: g.dist_init(0, 1, [0, nb], 2, 2, 2), says="damping")
    refused(lambda: g.substep_mid_halo(tl.DT), says="damping")
    refused(lambda: g.team_prepare(), says="damping")
    refused(lambda: g.chain_substeps(1, tl.DT), says="damping")
    refused(lambda: g.substep_begin_halo(tl.DT, (0, None, None, None, None), 0), says="damping")
    refused(lambda: GpuMpm.world_coupled_substeps([g], 1, tl.DT, [Collider(0, body=0, p_WB=(0.5, 0.5, 0.3))], 0.5, 1e5, 1e-4),
            says="damping")
    # a dt above the limit: every entry point that takes one, nothing enqueued
    before = g.stats()["substeps"]
    big = 1.01 * lim
    floor = [Collider(0, body=0, p_WB=(0.5, 0.5, 0.3))]
    for call in (lambda: g.run_substeps(2, big, -1), lambda: g.substep(big, -1), lambda: g.particle_to_grid(big),
                 lambda: g.profile_substeps(2, big, -1), lambda: g.run_coupled_substeps(2, big, floor, 0.5, 1e5, 1e-4),
                 lambda: g.substep_begin(big)):
        refused(call, says="mpm_damping_max_stable_dt")
    assert g.stats()["substeps"] == before
    g.run_substeps(2, tl.DT, -1)
    ph, _ = g.profile_substeps(2, tl.DT, -1)
    assert ph["fem"] > 0.0, ph
    g.gpu_sync()
    assert g.stats()["error_flags"] == 0
    # a later mpm_set_bending: the bending damping follows the new stiffness
    g.set_damping([(0.0, 1e-4)])
    assert g.damping_max_stable_dt() == np.inf and not g.damping_forces().any()
    g.set_bending([2e-5])
    f1 = g.damping_forces()
    assert f1.any() and g.damping_max_stable_dt() < np.inf
    g.set_bending([4e-5])
    f2 = g.damping_forces()
    H = bd.hinges(X, T)
    xv, vv = _vertex_state(g)
    kb = float(np.float32(1e-4)) * float(np.float32(4e-5))
    w = bd.margin(f2 - bd.force64(kb, H, vv), bd.bound(kb, H, vv), bd.rounding_count(bd.q_dense(len(X), H)[1]))
    assert w <= 1.0, w
    g.set_bending([0.0])
    assert not g.damping_forces().any()
    # off lifts the refusals; a partitioned engine refuses the call
    g.set_damping([])
    g.run_substeps(1, big, -1)
    g.dist_init(0, 1, [0, nb], 2, 2, 2)
    refused(lambda: g.set_damping(good), says="partitioned")
    assert not g.get_damping().any()
    g.destroy()
