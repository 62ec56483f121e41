"""CalcFemStateAndForce on the device in every constitutive regime of tests/fem_regimes.py, face by face, against the
double build of the oracle:

    err_face  <=  k * max(err32_face, sens_face)  +  c * 2^-23 * scale_face        (every field, every non-excluded face)

err_face = max |engine - oracle64| over the face's components; err32_face = max |oracle32 - oracle64|; sens_face the
measured sensitivity of the face to float rounding (fem_regimes.sensitivity: the largest change of the field, in double,
over 16 draws of one normwise 2^-24 rounding of every stage of the face); scale_face the face's natural size
(fem_regimes.face_scales: max|F| for F, vol E max(1, |F|^2) for tau, that over dx for the corner forces, the corners'
max |x|, |v| for the face particle's centroid and mean velocity); c = 64.  A whole-array bound would let a face of small
stress be badly wrong while a face of large stress sets the bound; this one cannot.

Why sens_face and not err32_face alone: err32_face is ONE draw of float rounding, and on a face that cancels it can be
small by luck.  A second, equally valid float evaluation -- the oracle's own source compiled with fused multiply-adds --
lands beyond 2 err32_face on a fraction of the faces of every regime, up to 78 x on the corner forces of the nearly flat
faces (I6, material d), where R^-1 carries the rounding residue of R[5] divided by R[4] ~ 1e-3.  Against
2 max(err32, sens) + c 2^-23 scale it stays within 0.23 of the bound in every regime, I6 included (I6: <= 0.18).

k = 2 on the strict path (FM = 0: k_fem<0>, k_fem_mat<0>).  The fast path (FM = 1: k_fem<1>, k_fem_mat<1>, the hardware
reciprocal and reciprocal square root plus one Newton step, results within ~0.6 ulp) is held to k = K_FAST = 3, the
factor tests/test_fast_math_gpu.py uses for benign states; measured, the fast path's worst per-face margin is 0.19 of
that bound (test_zz_margins lists every kernel instance and regime).

Kernel instances: k_fem<FM> through an engine created with each of materials (a) - (d); k_fem_mat<FM> through one engine
holding four cloths, one per material, each compared with an oracle that holds only that cloth.  Both oracles take the
engine's own Dm^-1 (the kernel under test is CalcFemStateAndForce, not Finalize).  Also: a fan whose centre vertex has
twelve faces (its force is summed from the G3 records), the collapsed triangle (NaN stress) and the over-range momentum
that ParticleToGrid must report as MPM_ERR_RANGE, and one substep further on the material (b) scene."""
import numpy as np
import pytest

from tests import fem_regimes as fr

pytestmark = pytest.mark.gpu

N_PER_CELL = 130
C_ULP = 64.0
K_STRICT = 2.0
K_FAST = 3.0
ERR_RANGE = -7   # MPM_ERR_RANGE (include/mpm_hip.h)
_SCENES = {}


def _scene(mk, xrange=(0.0, 1.0), seed=None):
    key = (mk, xrange)
    if key not in _SCENES:
        sc = fr.Scene(mk, N_PER_CELL, seed=100 + ord(mk) if seed is None else seed, xrange=xrange)
        _SCENES[key] = (sc,) + fr.oracle_pair(sc)
    return _SCENES[key]


WORST = {}   # (kernel, regime) -> worst error / allowed over fields and materials


def _compare(tag, sc, eng_view, v32, v64, ex, k, x32, F32, Dm):
    """the per-face bound on every non-excluded face; margins per (regime, field) to helpers.MARGINS"""
    from tests.helpers import MARGINS
    e_g, e_32 = fr.face_errors(eng_view, v64), fr.face_errors(v32, v64)
    scale = fr.face_scales(v64, sc.mat.E)
    sens = fr.sensitivity(sc.mat, fr.f32(F32), fr.f32(sc.C_face), fr.f32(x32).reshape(-1, 3, 3), fr.f32(Dm), v64["vol"])
    failures = []
    for f in fr.FIELDS:
        allowed = k * np.maximum(e_32[f], sens.get(f, 0.0)) + C_ULP * fr.EPS32 * scale[f]
        ratio = e_g[f] / allowed
        finite = np.isfinite(np.asarray(eng_view[f], np.float64).reshape(sc.nf, -1)).all(axis=1)
        ratio[~finite] = np.inf
        for i in fr.I_LABELS:
            for n in fr.N_OF[sc.mk]:
                m = (sc.I == i) & (sc.N == n) & ~ex
                w = int(np.argmax(ratio[m]))
                worst = float(ratio[m][w])
                rel = float((e_g[f][m] / scale[f][m]).max())
                MARGINS.append((worst, f"{tag} {i}/{n} {f} (per face)", C_ULP * fr.EPS32, rel, rel))
                key = (tag.split(" ")[0], i)
                WORST[key] = max(WORST.get(key, 0.0), worst)
                if not worst <= 1.0:
                    face = int(np.flatnonzero(m)[w])
                    failures.append(f"{tag} {i}/{n} {f}: face {face} engine {e_g[f][face]:.3e} from the double oracle, "
                                    f"float oracle {e_32[f][face]:.3e}, scale {scale[f][face]:.3e} ({worst:.2f} x allowed)")
    assert not failures, "\n".join(failures[:12])


def _engine(material=None, fast=False, deterministic=False):
    from drake_amd import GpuMpm
    g = GpuMpm(fr.BITS, fr.engine_material(material) if material else None)
    g.set_deterministic(deterministic)
    g.set_fast_math(fast)
    return g


@pytest.mark.parametrize("mk", sorted(fr.MATERIALS))
@pytest.mark.parametrize("kernel", ["k_fem<0>", "k_fem<1>"])
def test_single_material_kernel_face_by_face(kernel, mk):
    from drake_amd import ARR as A
    fast = kernel.endswith("<1>")
    sc, o32, o64, (x32, F32), q, ex = _scene(mk)
    g = _engine(sc.m, fast)
    g.add_qr_cloth(*sc.sheet())
    g.finalize()
    pos, vel, C, F, _ = fr.combined_state([(sc, 0, 0, o32.DmInv)], sc.nf, 3 * sc.nf)
    fr.set_engine_state(g, pos, vel, C, F)
    g.rebuild_mapping(True)
    g.calc_fem_state_and_force(fr.DT)
    g.gpu_sync()
    # (the kernel under test is CalcFemStateAndForce: both oracles take the engine's Dm^-1 from its Finalize)
    Dm = g.download(A.DM_INVERSES)
    c32, c64 = fr.run_fem_copy(o32, Dm), fr.run_fem_copy(o64, Dm)
    v32, v64 = fr.face_view(fr.of_oracle(c32), sc.nf), fr.face_view(fr.of_oracle(c64), sc.nf)
    _compare(f"{kernel} ({mk})", sc, fr.face_view(fr.of_engine(g), sc.nf), v32, v64, ex, K_FAST if fast else K_STRICT,
             x32, F32, Dm)
    g.destroy()


_MAT_RESULTS = {}


def _multi_material(fast):
    """one engine (the default material) holding four cloths, materials (a) - (d), side by side along x"""
    if fast in _MAT_RESULTS:
        return _MAT_RESULTS[fast]
    parts = [_scene(mk, xrange=(0.25 * c, 0.25 * (c + 1)), seed=200 + c) for c, mk in enumerate(sorted(fr.MATERIALS))]
    g = _engine(None, fast)
    for sc, *_ in parts:
        g.add_qr_cloth(*sc.sheet(), material=fr.cloth_material(sc.m))
    g.finalize()
    info = [g.cloth_info(c) for c in range(len(parts))]
    nf, nv = g.n_faces, g.n_verts
    pos, vel, C, F, _ = fr.combined_state([(sc, inf["first_face"], inf["first_vertex"], o32.DmInv)
                                           for (sc, o32, *_), inf in zip(parts, info)], nf, nv)
    fr.set_engine_state(g, pos, vel, C, F)
    g.rebuild_mapping(True)
    g.calc_fem_state_and_force(fr.DT)
    g.gpu_sync()
    assert g.stats()["error_flags"] == 0
    eng = fr.of_engine(g)
    from drake_amd import ARR as A
    Dm = g.download(A.DM_INVERSES)
    g.destroy()
    _MAT_RESULTS[fast] = (parts, info, nf, eng, Dm)
    return _MAT_RESULTS[fast]


@pytest.mark.parametrize("mk", sorted(fr.MATERIALS))
@pytest.mark.parametrize("kernel", ["k_fem_mat<0>", "k_fem_mat<1>"])
def test_multi_material_kernel_face_by_face(kernel, mk):
    """each cloth of the four-material engine against oracles that hold only that cloth, with its material"""
    fast = kernel.endswith("<1>")
    parts, info, nf, eng, Dm = _multi_material(fast)
    c = sorted(fr.MATERIALS).index(mk)
    sc, o32, o64, (x32, F32), q, ex = parts[c]
    view = fr.face_view(eng, nf, info[c]["first_face"], info[c]["first_vertex"], sc.nf)
    Dm = Dm[info[c]["first_face"]:info[c]["first_face"] + sc.nf]
    v32, v64 = (fr.face_view(fr.of_oracle(fr.run_fem_copy(o, Dm)), sc.nf) for o in (o32, o64))
    _compare(f"{kernel} ({mk})", sc, view, v32, v64, ex, K_FAST if fast else K_STRICT, x32, F32, Dm)


def _fan(n=12, seed=5):
    """n triangles around one centre vertex (index 0), rest edges ~0.4 dx, in a random plane"""
    rng = np.random.default_rng(seed)
    ang = np.linspace(0, 2 * np.pi, n, endpoint=False) + rng.uniform(-0.1, 0.1, n)
    rad = 0.4 * fr.DX * rng.uniform(0.9, 1.1, n)
    p2 = np.concatenate([np.zeros((1, 2)), np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)])
    Rot = fr._rot3(rng, 1)[0]
    cen = np.array([0.5, 0.5, 0.5])
    rest = cen + p2 @ Rot[:, :2].T
    idx = np.array([[0, 1 + k, 1 + (k + 1) % n] for k in range(n)], np.int32)
    # deformation: one shear in the plane (I4), so the mesh stays connected
    G = np.array([[1.0, 0.45], [0.0, 1.0]])
    Rd = fr._rot3(rng, 1)[0]
    x = (cen + (p2 @ G.T) @ Rd[:, :2].T).astype(np.float32)
    # N3 under material (d): r33 in [0.5, 0.9], shear 1.5 - 3 times the cone's edge
    mat = fr.Mat(fr.MATERIALS["d"])
    r33 = rng.uniform(0.5, 0.9, n)
    s = rng.uniform(1.5, 3.0, n) * mat.cF * (1 - r33) ** 2 / mat.gok
    a = rng.uniform(0, 2 * np.pi, n)
    r = np.stack([s * np.cos(a), s * np.sin(a), r33], 1)
    Cf = rng.normal(size=(n, 9))
    Cf = (Cf * (1e-2 / fr.DT) / np.abs(Cf).max(axis=1, keepdims=True)).astype(np.float32)
    vel = rng.uniform(-0.1, 0.1, (n + 1, 3)).astype(np.float32)
    return rest.astype(np.float32), vel, idx, x, r, Cf, mat


@pytest.mark.parametrize("kernel", ["k_fem<0>", "k_fem<1>"])
def test_vertex_with_twelve_faces_in_the_cone_return(kernel):
    """I4 / N3 under material (d) on a fan: the centre vertex's force, summed from twelve G3 records, within
    k err32 + c 2^-23 (sum of the magnitudes of its twelve face contributions); every other vertex likewise"""
    from oracle import oracle as orc
    from tests.helpers import MARGINS, oracle_copy
    fast = kernel.endswith("<1>")
    rest, vel, idx, x, r, Cf, mat = _fan()
    m = fr.MATERIALS["d"]
    o32 = orc.OracleMpm(fr.BITS)
    fr.oracle_material(o32, m)
    g = _engine(m, fast)
    for s in (o32, g):
        s.add_qr_cloth(rest, vel, idx)
        s.finalize()
    nf, nv = len(idx), len(rest)
    F = fr.upload_F(x, idx, o32.DmInv, r, Cf)
    pos = np.concatenate([(fr.f32(x)[idx].sum(axis=1) / 3).astype(np.float32), x])
    velo = np.concatenate([(fr.f32(vel)[idx].sum(axis=1) / 3).astype(np.float32), vel])
    C = np.concatenate([Cf, np.zeros((nv, 9), np.float32)])
    fr.set_oracle_state(o32, pos, velo, C, F)
    fr.set_engine_state(g, pos, velo, C, F)
    o64 = oracle_copy(o32, np.float64)
    for s in (o32, o64, g):
        s.rebuild_mapping(True)
        s.calc_fem_state_and_force(fr.DT)
    g.gpu_sync()
    fe, f32_, f64_ = (fr.of_engine(g)["force"][nf:], fr.of_oracle(o32)["force"][nf:], fr.of_oracle(o64)["force"][nf:])
    # every face is in the cone return, away from its thresholds
    q_ps = fr.project_strain(mat, fr.updated_normal(fr.f32(F), fr.f32(Cf)))[1]
    assert np.all(q_ps["branch"] == 3) and np.all(np.abs(q_ps["f"]) > 1e-3 * q_ps["f_scale"])
    # the face contributions in double: V P[:, 0:2] grad N of every face
    Fp = fr.of_oracle(o64)["F"]
    P, _ = fr.cloth_dphi_dF(mat, Fp)
    vol = fr.of_oracle(o64)["vol"][:nf]
    Dm = fr.f32(o32.DmInv)
    scale = np.zeros(nv)
    for f in range(nf):
        VP = (P[f] * vol[f]).reshape(3, 3)
        DmiT = np.array([[Dm[f, 0], Dm[f, 2]], [Dm[f, 1], Dm[f, 3]]])
        Gm = VP[:, :2] @ (DmiT @ np.array([[-1.0, 1.0, 0.0], [-1.0, 0.0, 1.0]]))
        for c in range(3):
            scale[idx[f, c]] += np.linalg.norm(Gm[:, c])
    assert (idx == 0).sum() == 12
    e_g, e_32 = np.abs(fe - f64_).max(axis=1), np.abs(f32_ - f64_).max(axis=1)
    k = K_FAST if fast else K_STRICT
    allowed = k * e_32 + C_ULP * fr.EPS32 * scale
    MARGINS.append((float((e_g / allowed).max()), f"{kernel} fan vertex forces (per vertex)", C_ULP * fr.EPS32,
                    float((e_g / scale).max()), float((e_g / scale).max())))
    assert np.isfinite(fe).all()
    assert np.all(e_g <= allowed), (e_g, e_32, scale)
    assert np.abs(f64_[0]).max() > 1e-3 * scale[0]   # (the centre's force is not a cancellation to nothing)
    g.destroy()


def _few_triangles(n=4, seed=9):
    rng = np.random.default_rng(seed)
    sc = fr.Scene("a", 1, seed=seed)
    k = rng.choice(sc.nf, n, replace=False)
    idx = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    rest = sc.rest_pos.reshape(-1, 3, 3)[k].reshape(-1, 3)
    return rest, sc.vel.reshape(-1, 3, 3)[k].reshape(-1, 3), idx


@pytest.mark.parametrize("deterministic", [False, True], ids=["default", "deterministic"])
def test_collapsed_triangle_is_non_finite_where_the_oracle_is_and_p2g_reports_range(deterministic):
    """three vertices on one point: the in-plane block is exactly zero, J = 0 and the reference's stress is NaN.  The
    engine's outputs are non-finite on exactly the particles where the float oracle's are, positions stay finite, and
    the ParticleToGrid that follows raises MPM_ERR_RANGE at the next synchronisation"""
    from drake_amd import ARR as A, MpmError
    from oracle import oracle as orc
    rest, vel, idx = _few_triangles()
    o32 = orc.OracleMpm(fr.BITS)
    g = _engine(None, False, deterministic)
    for s in (o32, g):
        s.add_qr_cloth(rest, vel, idx)
        s.finalize()
    nf = len(idx)
    orig = fr.of_oracle(o32)
    x = orig["x"][nf:].astype(np.float32)
    x[3:6] = x[3:6].mean(axis=0)                       # face 1 collapses
    pos = np.concatenate([(fr.f32(x)[idx].sum(axis=1) / 3).astype(np.float32), x])
    velo = orig["v"].astype(np.float32)
    C = np.zeros((len(pos), 9), np.float32)
    F = o32.F.copy()
    fr.set_oracle_state(o32, pos, velo, C, F)
    fr.set_engine_state(g, pos, velo, C, F)
    for s in (o32, g):
        s.rebuild_mapping(True)
        s.calc_fem_state_and_force(fr.DT)
    g.gpu_sync()
    eo, oo = fr.of_engine(g), fr.of_oracle(o32)
    bad_o = {f: ~np.isfinite(oo[f].reshape(len(oo[f]), -1)).all(axis=1) for f in ("F", "tau", "force")}
    assert bad_o["force"][nf + 3:nf + 6].all() and bad_o["tau"][1] and bad_o["force"].sum() == 3
    for f in ("F", "tau", "force"):
        bad_g = ~np.isfinite(eo[f].reshape(len(eo[f]), -1)).all(axis=1)
        assert np.array_equal(bad_g, bad_o[f]), (f, np.flatnonzero(bad_g), np.flatnonzero(bad_o[f]))
    assert np.isfinite(g.download(A.POSITIONS)).all()
    g.particle_to_grid(fr.DT)
    with pytest.raises(MpmError) as e:
        g.gpu_sync()
    assert e.value.code == ERR_RANGE, e.value
    assert np.isfinite(g.download(A.POSITIONS)).all()
    g.destroy()


@pytest.mark.parametrize("deterministic", [False, True], ids=["default", "deterministic"])
def test_momentum_beyond_the_fixed_point_range(deterministic):
    """one triangle moving at 1e6: its node momentum exceeds total mass x 2^15 (set_fixed_point_scales,
    mpm_engine.hip).  The fixed-point tiles of the deterministic engine must say so (MPM_ERR_RANGE at the sync); the
    double tiles of the default engine hold it, and their grid momentum matches the double oracle"""
    from drake_amd import ARR as A, MpmError
    from oracle import oracle as orc
    from tests.helpers import MARGINS, oracle_copy
    rest, vel, idx = _few_triangles(1, seed=3)
    o32 = orc.OracleMpm(fr.BITS)
    g = _engine(None, False, deterministic)
    for s in (o32, g):
        s.add_qr_cloth(rest, vel, idx)
        s.finalize()
    orig = fr.of_oracle(o32)
    velo = (np.array([1.0e6, -0.6e6, 0.8e6], np.float32) + orig["v"]).astype(np.float32)
    C = np.zeros((len(velo), 9), np.float32)
    fr.set_oracle_state(o32, orig["x"].astype(np.float32), velo, C, o32.F.copy())
    fr.set_engine_state(g, orig["x"].astype(np.float32), velo, C, o32.F.copy())
    o64 = oracle_copy(o32, np.float64)
    mass = float(np.sum(fr.of_oracle(o64)["vol"])) * float(o64.p.density)
    for s in (o32, o64, g):
        s.rebuild_mapping(True)
        s.calc_fem_state_and_force(fr.DT)
        s.particle_to_grid(fr.DT)
    assert np.abs(o64.g_mv).max() > mass * 2 ** 16     # (beyond the bound, whatever the rounding of log2(mass))
    if deterministic:
        with pytest.raises(MpmError) as e:
            g.gpu_sync()
        assert e.value.code == ERR_RANGE, e.value
    else:
        g.gpu_sync()
        assert g.stats()["error_flags"] == 0
        mv = g.download(A.GRID_MOMENTUM).astype(np.float64)
        e_g, e_32 = np.abs(mv - o64.g_mv).max(), np.abs(o32.g_mv - o64.g_mv).max()
        allowed = K_STRICT * e_32 + C_ULP * fr.EPS32 * np.abs(o64.g_mv).max()
        MARGINS.append((e_g / allowed, "over-range momentum, double tiles", C_ULP * fr.EPS32,
                        e_g / np.abs(o64.g_mv).max(), e_g / np.abs(o64.g_mv).max()))
        assert e_g <= allowed, (e_g, e_32)
    assert np.isfinite(g.download(A.POSITIONS)).all()
    g.destroy()


@pytest.mark.parametrize("deterministic", [False, True], ids=["default", "deterministic"])
def test_branch_mixed_stresses_through_one_substep(deterministic):
    """the material (b) scene, one substep on from the regime state (FEM, P2G, grid, G2P): the whole-array bound of
    tests/test_precision_gpu.py (engine within 2x the float oracle's distance from the double one), grid velocities
    mass-weighted"""
    from drake_amd import ARR as A
    from tests.test_precision_gpu import _check
    sc, o32, o64, _, q, ex = _scene("b")
    g = _engine(sc.m, False, deterministic)
    g.add_qr_cloth(*sc.sheet())
    g.finalize()
    pos, vel, C, F, _ = fr.combined_state([(sc, 0, 0, o32.DmInv)], sc.nf, 3 * sc.nf)
    fr.set_engine_state(g, pos, vel, C, F)
    from tests.helpers import oracle_copy
    a32, a64 = oracle_copy(o32, np.float32), oracle_copy(o64, np.float64)
    g.rebuild_mapping(True)
    for s in (a32, a64, g):
        s.calc_fem_state_and_force(fr.DT)
        s.particle_to_grid(fr.DT)
        s.update_grid(-1)
    tag = f"regimes (b) {'deterministic' if deterministic else 'default'}"
    w = (a64.g_m / a64.g_m.max())[:, None]
    _check(f"{tag} p2g mass", g.download(A.GRID_MASSES), a32.g_m, a64.g_m)
    _check(f"{tag} grid v", g.download(A.GRID_MOMENTUM), a32.g_mv, a64.g_mv, weight=w)
    _check(f"{tag} grid v*", g.download(A.GRID_V_STAR), a32.g_vstar, a64.g_vstar, weight=w)
    for s in (a32, a64, g):
        s.grid_to_particle(fr.DT)
    g.gpu_sync()
    assert g.stats()["error_flags"] == 0
    eo, o3, o6 = fr.of_engine(g), fr.of_oracle(a32), fr.of_oracle(a64)
    _check(f"{tag} g2p x", eo["x"], o3["x"], o6["x"], floor=1e-7)
    _check(f"{tag} g2p v", eo["v"], o3["v"], o6["v"])
    Cg = g.download(A.AFFINE)
    un = lambda a, p: (lambda o: (o.__setitem__(p, a), o)[1])(np.empty(a.shape, np.float64))
    _check(f"{tag} g2p C", un(Cg, g.download(A.PIDS)), un(a32.C, a32.pids), un(a64.C, a64.pids))
    g.destroy()


def test_zz_margins():
    """the worst per-face margin (error / allowed, over fields and materials) of every kernel instance and in-plane
    regime of the tests above, printed.  Measured on an MI355X (every one <= 1 by the tests above):
                     I1    I2    I3    I4    I5    I6
      k_fem<0>      0.237 0.234 0.166 0.217 0.149 0.224
      k_fem<1>      0.171 0.189 0.141 0.122 0.173 0.173
      k_fem_mat<0>  0.171 0.194 0.184 0.215 0.158 0.279
      k_fem_mat<1>  0.148 0.167 0.130 0.132 0.109 0.186
    The fast path, held to K_FAST = 3, uses at most 0.19 of it: it would meet k = 2 as well (worst 0.19 x 3 / 2 = 0.29)."""
    lines = [f"  {k:14s} " + " ".join(f"{i}:{WORST.get((k, i), float('nan')):5.3f}" for i in fr.I_LABELS)
             for k in ("k_fem<0>", "k_fem<1>", "k_fem_mat<0>", "k_fem_mat<1>")]
    print("worst per-face margin per kernel instance and in-plane regime\n" + "\n".join(lines))
