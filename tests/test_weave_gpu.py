"""Woven cloth (mpm_set_weave) on the engine, 64^3 grid (tests/weave.py holds the model, the scenes and the bound).

1. mpm_weave_forces: the records per face and the forces per vertex against records64 within R 2^-24 record_bound (a
   vertex with n records: R + n), on every scene x axis case x state, in default and deterministic mode, with fast math
   on and off; the device records, strains and axes are the host functions' bits.
2. After mpm_calc_fem_state_and_force, MPM_ARR_FORCES of an engine with the weave minus a twin's without is
   mpm_weave_forces within the roundings of the float sums; again with membrane damping on in both (k_fem, k_weave, k_damp).
3. Particle order: forces and energy by original id are the same bits after re-sorts; the energy against energy64.
4. Every substep path of tests/substep_paths.py with every other feature on, to the bit; the coupled path against the
   seven calls.
5. Off means off.  6. More than 256 cloths.  7. Dynamics: hanging twins, and the energy of a released sheet.
8. The guard and the refusals."""
import functools

import numpy as np
import pytest

from tests import bending as bd
from tests import harness as hs
from tests import weave as wv

pytestmark = pytest.mark.gpu

U = wv.U
R = wv.rounding_count()
_CACHE = {}


_record = functools.partial(hs.record, prefix="weave: ")
_engine = functools.partial(hs.engine, fast_math=False)
_by_id = functools.partial(hs.by_id, split=True)


def _note(line):
    """a measured figure of the dynamics tests, printed (profiles/weave_margins.txt is written from this output)"""
    print("weave_margins: " + line)


def _rest(g):
    """(dm (nf, 3), vol (nf,)) float32 in original face order, of a SINGLE-material engine (whose MPM_ARR_VOLUMES is the
    record the face kernels read)"""
    A = hs.ARR()
    nf = g.n_faces
    return g.download(A.DM_INVERSES).reshape(nf, 4)[:, [0, 1, 3]].copy(), _by_id(g, A.VOLUMES)[0].copy()


def _scene(name):
    """tests/weave.py's scene with the engine's own rest records (Finalize's geometry does not depend on the material)"""
    if name not in _CACHE:
        s = wv.scene(name)
        single = _engine(s["meshes"])
        s["rest"] = _rest(single)
        single.destroy()
        s["coef_f"] = s["coef"][s["cof"]]
        s["woven"] = np.any(s["coef_f"] != 0, axis=1)
        s["Xc"] = wv.corners(s["T"], s["X"])
        _CACHE[name] = s
    return _CACHE[name]


def _set_case(g, s, case):
    """the axis case in force -> cs32 (nf, 2) as the host function gives it, (0, 0) on the faces without weave"""
    from drake_amd import weave_face_axes
    table, fd, dirs = wv.axis_case(s, case)
    g.set_weave(table, fd)
    cs, bad = weave_face_axes(s["Xc"], dirs)
    assert bad == -1
    cs[~s["woven"]] = 0.0
    return cs


def _check(g, s, cs, x, what):
    """records, forces, strains and energies of the engine at the uploaded positions x against float64 and the host"""
    from drake_amd import weave_face_records
    dm, vol = s["rest"]
    T = s["T"]
    xc = wv.corners(T, x)
    f, rec = g.weave_forces(records=True)
    ref = wv.records64(dm, vol, s["coef_f"], cs, xc)
    B = wv.record_bound(dm, vol, s["coef_f"], cs, xc)
    w_rec = wv.margin(rec - ref, B, R)
    n = wv.valence(T, len(x))
    w_f = wv.margin(f - wv.vertex_sum(T, len(x), ref), -wv.vertex_sum(T, len(x), B), (R + n)[:, None])
    host_rec, host_strain, host_energy = weave_face_records(dm, vol, s["coef_f"], cs, xc)
    # (a face without weave: the engine writes nothing, +0; the host function forms products with zero coefficients, -0)
    host_rec = np.where(s["woven"][:, None, None], host_rec, 0.0).astype(np.float32)
    assert np.array_equal(hs.bits(rec), hs.bits(host_rec)), (what, int((hs.bits(rec) != hs.bits(host_rec)).sum()))
    assert np.array_equal(hs.bits(g.weave_strain()), hs.bits(np.where(s["woven"][:, None], host_strain, 0.0).astype(np.float32))), what
    assert w_rec <= 1.0 and w_f <= 1.0, (what, w_rec, w_f)
    assert not rec[~s["woven"]].any()
    return w_rec, w_f, f, host_energy


# ---- 1 -------------------------------------------------------------------------------------------------------------------
MODES = {"default": (False, False), "deterministic": (True, False), "default_fast": (False, True), "deterministic_fast": (True, True)}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(wv.SCENES))
def test_forces_against_float64(name, mode):
    from tests import helpers
    det, fast = MODES[mode]
    helpers.tag_default_engine(not det)
    s = _scene(name)
    g = _engine(s["meshes"], mats=s["mats"], deterministic=det, fast_math=fast)
    assert g.cloth_count() == len(s["meshes"])
    worst = [0.0, 0.0]
    for case in wv.axis_cases(name):
        cs = _set_case(g, s, case)
        assert np.array_equal(hs.bits(g.weave_axes()), hs.bits(cs)), (name, case)
        got = g.get_weave()
        assert np.array_equal(np.array([got["E_warp"], got["E_weft"], got["nu"], got["G"]]).T,
                              wv.axis_case(s, case)[0][:, :4])
        for st in wv.STATES:
            x = wv.state(st, s)
            hs.upload(g, x)
            assert np.array_equal(g.dump_cpu_state()[0], x)
            w_rec, w_f, f, _ = _check(g, s, cs, x, f"{name} {case} {st} [{mode}]")
            worst = [max(worst[0], w_rec), max(worst[1], w_f)]
            if st not in wv.UNSTRAINED:
                on = np.zeros(len(x), bool)
                on[s["T"][s["woven"]].reshape(-1)] = True
                assert np.all(np.abs(f[on]).max(axis=1) > 0), "a vertex was left out"
                assert not f[~on].any()
    print(f"weave forces {name} [{mode}]: records {worst[0]:.3g}, vertex forces {worst[1]:.3g} of the bound")
    _record(f"records {name} [{mode}]", worst[0])
    _record(f"vertex forces {name} [{mode}]", worst[1])
    assert g.stats()["error_flags"] == 0
    g.destroy()


# ---- 2 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("damped", [False, True], ids=["", "damped"])
@pytest.mark.parametrize("name", ["sheet54", "fan", "pair_multi"])
def test_total_forces_include_the_weave(name, damped):
    """FORCES(weave) - FORCES(twin) = mpm_weave_forces within the roundings of the float sums.  A vertex with n records:
    the engine with the weave sums fl(fl(e_j + w_j) + d_j) -- 2 n roundings of the adds (n without damping) and n - 1 of
    k_vforce's sum --, the twin fl(e_j + d_j) -- n (0) and n - 1 --, mpm_weave_forces n - 1; each rounding is below
    2^-24 of the sum of the absolute records at the vertex: (6 n - 3) with damping, (4 n - 3) without.  |e_j| from the
    float64 restatement of the face kernel (tests/fem_regimes.py), |w_j| and |d_j| from the float64 records.  (The fan's
    hub has 12 faces: DP::G3; pair_multi runs k_fem_mat.)  The order k_fem, k_weave, k_damp is what the count assumes."""
    from tests import damping as dp
    from tests import fem_regimes as fr
    from tests import transfer_layouts as tl
    A = hs.ARR()
    s = _scene(name)
    dm, vol = s["rest"]
    T, nf = s["T"], len(s["T"])
    a, b = _engine(s["meshes"], mats=s["mats"]), _engine(s["meshes"], mats=s["mats"])
    cs = _set_case(a, s, "30")
    betas = None
    if damped:
        for g in (a, b):
            g.set_damping([(1.0, 0.0)] * len(s["meshes"]))
            betas = np.array([(0.25 * g.damping_max_stable_dt() / tl.DT, 0.0)] * len(s["meshes"]), np.float32)
            g.set_damping(betas)
    x0 = wv.state("affine", s)
    v0 = dp.velocity("random", x0).astype(np.float32)
    out = []
    for g in (a, b):
        hs.upload(g, x0, v0)
        F_up = g.download(A.DEFORMATION_GRADIENTS)
        g.rebuild_mapping(False)
        g.calc_fem_state_and_force(tl.DT)
        out.append(_by_id(g, A.FORCES)[1].copy())
    fw = a.weave_forces()
    assert fw.any() and out[1].any() and not b.weave_forces().any() and b.weave_max_stable_dt() == np.inf
    base = a.default_material()
    xc, vc = wv.corners(T, x0), wv.corners(T, v0)
    dm4 = a.download(A.DM_INVERSES).reshape(nf, 4)
    E = np.zeros((nf, 3, 3))
    D = np.zeros((nf, 3, 3))
    for c in range(len(s["meshes"])):
        m = dict(fr.DEFAULT)
        m.update({k: getattr(base, k) for k in ("youngs_modulus", "poisson_ratio", "gamma", "K", "c_F")})
        m.update({k: v for k, v in (s["mats"][c] if s["mats"] else {}).items() if k in m})
        sel = s["cof"] == c
        E[sel] = fr.face64(fr.Mat(m), F_up[sel].astype(np.float64), np.zeros((int(sel.sum()), 9)), xc[sel].astype(np.float64),
                           dm4[sel].astype(np.float64), vol[sel])["force"]
        if damped:
            Ey, nu = np.float32(m["youngs_modulus"]), np.float32(m["poisson_ratio"])
            mu, lam = Ey / (np.float32(2) * (np.float32(1) + nu)), Ey * nu / ((np.float32(1) + nu) * (np.float32(1) - np.float32(2) * nu))
            D[sel] = dp.records64(dm[sel], vol[sel], mu, lam, betas[c][0], xc[sel], vc[sel])
    W = wv.records64(dm, vol, s["coef_f"], cs, xc)
    mag = -wv.vertex_sum(T, len(x0), np.abs(E) + np.abs(W) + np.abs(D))
    n = wv.valence(T, len(x0))
    count = (6.0 * n - 3.0) if damped else (4.0 * n - 3.0)
    tol = count[:, None] * U * mag * (1.0 + 1e-3)      # (1e-3: the magnitudes are float64 values of float sums)
    err = np.abs(out[0].astype(np.float64) - out[1].astype(np.float64) - fw.astype(np.float64))
    w = float(np.where(err == 0, 0.0, err / np.maximum(tol, 1e-300)).max())
    print(f"total forces with the weave: {name} damped={damped}: {w:.3g} of the tolerance; |weave| / |rest| = "
          f"{np.abs(fw).max() / np.abs(out[1]).max():.3g}")
    _record(f"total forces {name} damped={damped}", w)
    assert w <= 1.0, w
    assert np.abs(fw).max() > 1e3 * tol.max(), "the weave's force is far above the tolerance"
    for g in (a, b):
        assert g.stats()["error_flags"] == 0
        g.destroy()


# ---- 3 -------------------------------------------------------------------------------------------------------------------
def test_particle_order_and_energy():
    """`big`: a state uploaded, substeps five cells further along x with a re-sort check forced on every substep
    (MPM_RESORT_EVERY = 1) until slots have moved, the state uploaded again: forces, records and energy by original id
    are the bits of a fresh engine given the same state; the energy is the same bits in default mode.  Against energy64:
    a face's float vol Psi carries at most 18 roundings of its absolute terms (the strains 13, S 14, the products and the
    chain of Psi 3 more, vol 1), the double sum of n faces n 2^-53 of the sum: (18 2^-24 + n 2^-53) sum_f |vol Psi|_abs."""
    s = _scene("big")
    dm, vol = s["rest"]
    env = {"MPM_RESORT_EVERY": "1", "MPM_QUIET_FACTOR": "0"}
    g, fresh, dflt = _engine(s["meshes"], env=env), _engine(s["meshes"]), _engine(s["meshes"], deterministic=False)
    cs = None
    for e in (g, fresh, dflt):
        cs = _set_case(e, s, "130")
    x0 = wv.state("cylinder3", s)
    pid0 = g.download(hs.ARR().PIDS)
    before = g.stats()["rebuilds"]
    # (the rotated sheet of `affine`, five cells along x: another order of the cells than the flat rest sheet's)
    hs.upload(g, wv.state("affine", s) + np.array([5.0 / 64, 0.0, 0.0], np.float32), np.array([3.0, 0.5, 0.0], np.float32))
    g.run_substeps(12, 1e-4, -1)
    g.gpu_sync()
    assert g.stats()["error_flags"] == 0 and g.stats()["rebuilds"] > before, g.stats()
    g.rebuild_mapping(True)       # (and the full sort, as tests/test_feature_paths_gpu.test_particle_order does)
    assert not np.array_equal(g.download(hs.ARR().PIDS), pid0), "no slot moved"
    res = []
    for e in (g, fresh, dflt):
        hs.upload(e, x0)
        f, rec = e.weave_forces(records=True)
        res.append((f, rec, e.weave_strain(), e.weave_energy()))
    for k in (1, 2):
        for a, b in zip(res[0][:3], res[k][:3]):
            assert np.array_equal(hs.bits(a), hs.bits(b))
        assert np.array_equal(res[0][3][0].view(np.uint64), res[k][3][0].view(np.uint64)) and res[0][3][1] == res[k][3][1]
    xc = wv.corners(s["T"], x0)
    ref = float(wv.energy64(dm, vol, s["coef_f"], cs, xc).sum())
    bound = (18 * U + len(xc) * 2.0 ** -53) * float(wv.energy_bound(dm, vol, s["coef_f"], cs, xc).sum())
    rows, total = res[0][3]
    w = abs(total - ref) / bound
    print(f"weave energy on big: {total:.9g}, float64 {ref:.9g}: {w:.3g} of the bound")
    _record("energy against float64", w)
    assert len(rows) == 1 and rows[0] == total and total > 0 and w <= 1.0, (total, ref, w)
    for e in (g, fresh, dflt):
        assert e.stats()["error_flags"] == 0
        e.destroy()


# ---- 4 -------------------------------------------------------------------------------------------------------------------
def _paths_weave(g):
    """a weave on both sheets of tests/feature_paths.py's scene, sized so that DT is SHARE of its guard"""
    from tests import feature_paths as fp
    if "paths_table" not in _CACHE:
        base = np.array([(10.0, 2.0, 0.2, 0.05, 1.0, 0.5, 0.0), (4.0, 8.0, 0.1, 0.02, 0.3, 1.0, 0.0), (0, 0, 0, 0, 1, 0, 0),
                         (0, 0, 0, 0, 1, 0, 0)], np.float32)
        g.set_weave(base)
        scale = np.float32((fp.SHARE * g.weave_max_stable_dt() / fp.DT) ** 2)      # (the guard goes with 1 / sqrt(k))
        t = base.copy()
        t[:, [0, 1, 3]] *= scale
        _CACHE["paths_table"] = t
    g.set_weave(_CACHE["paths_table"])
    assert fp.DT <= 0.5 * g.weave_max_stable_dt(), g.weave_max_stable_dt()


def _paths_state(g):
    from tests import feature_paths as fp
    st = fp.state(g)
    f, rec = g.weave_forces(records=True)
    rows, total = g.weave_energy()
    st.update(forces_weave=fp.words(f), weave_records=fp.words(rec), weave_strain=fp.words(g.weave_strain()),
              weave_energy=fp.words(rows), weave_total=fp.words(np.array([total])))
    return st


def _paths_run(name):
    from tests import feature_paths as fp
    key = ("paths", name)
    if key not in _CACHE:
        runner, env = fp.FUSED[name]
        g = fp.engine(fp.EVERYTHING, env=env)
        _paths_weave(g)
        runner(g, -1)
        skipped = g.owed_substeps()
        _CACHE[key] = (_paths_state(g), g.stats(), skipped)
        g.destroy()
    return _CACHE[key]


@pytest.mark.parametrize("name", ["run_substeps_sparse_checks", "substeps", "profile_substeps", "phase_calls", "phase_calls_undeferred"])
def test_every_substep_path_ends_in_the_same_bits(name):
    """tests/feature_paths.engine(EVERYTHING) plus a weave on both sheets: every runner of FUSED leaves the bits of
    run_substeps after N = 48 substeps, through re-sorts and substeps that skipped themselves"""
    from tests import feature_paths as fp
    assert fp.N == 48
    (sa, ta, _), (sb, tb, skipped) = _paths_run("run_substeps"), _paths_run(name)
    for st in (ta, tb):
        assert st["error_flags"] == 0 and st["substeps"] == fp.N and st["rebuilds"] > 1, st
    assert ta["rebuilds"] == tb["rebuilds"]
    if name == "run_substeps_sparse_checks":
        assert skipped > 0, "no substep skipped itself with k_weave in it"
    assert set(sa) == set(sb)
    for k in sa:
        assert sa[k].size and np.array_equal(sa[k], sb[k]), (name, k, int((sa[k] != sb[k]).sum()))
    f = fp.floats(sa, "forces_weave").reshape(-1, 3)
    s = fp.scene()
    assert f[:s["first"][2]].any() and not f[s["first"][2]:].any() and np.isfinite(f).all()
    # the weave acted: the run differs from the one of the engine without it
    if name == "substeps":
        bare = fp.run("run_substeps")[0]
        assert not np.array_equal(bare["vel"], sa["vel"])


def test_coupled_equals_the_seven_calls():
    """run_coupled_substeps in two calls against the reference's seven calls per substep, over the floor the lower sheet
    reaches, with everything and the weave on: the same contact rows and the same bits (tests/test_feature_paths_gpu.py)"""
    from tests import feature_paths as fp
    out = []
    for runner in (lambda g: fp.seven_calls(g, fp.floor(), fp.N), lambda g: fp.coupled(g, fp.floor())):
        g = fp.engine()
        _paths_weave(g)
        rows = runner(g)
        out.append((_paths_state(g), g.stats(), rows))
        g.destroy()
    (sa, ta, ra), (sb, tb, rb) = out
    assert ta["error_flags"] == 0 and tb["error_flags"] == 0 and ta["substeps"] == tb["substeps"] == fp.N
    assert ta["rebuilds"] >= 2 and ta["rebuilds"] == tb["rebuilds"]
    contacts = [r["contacts"] for r in ra]
    assert max(contacts) > 0 and min(contacts) == 0, contacts
    for key in ("iterations", "contacts", "residual"):
        a, b = np.array([float(r[key]) for r in ra]), np.array([float(r[key]) for r in rb])
        assert np.all((a == b) | (np.isnan(a) & np.isnan(b))), key
    for k in sa:
        assert sa[k].size and np.array_equal(sa[k], sb[k]), (k, int((sa[k] != sb[k]).sum()))
    assert fp.floats(sa, "forces_weave").any()


def test_sums_family_with_the_weave():
    """substep_begin / substep_end, the one member of the sums family the feature supports (the halo calls stay refused):
    one substep_begin leaves the forces of RebuildMapping + CalcFemStateAndForce to the bit, and N x (begin, end) runs.
    (The two families' particle states are not compared: gather + update from sums is another order of arithmetic.)"""
    from drake_amd import MpmError
    from tests import feature_paths as fp
    from tests import substep_paths as sp
    x0, v0 = fp.perturbed_state()
    g, twin = fp.engine(), fp.engine()
    for e in (g, twin):
        _paths_weave(e)
        fp.upload(e, x0, v0)
    with pytest.raises(MpmError, match="halo substeps: not available"):
        g.substep_mid_halo(fp.DT, -1)
    g.substep_begin(fp.DT)
    twin.rebuild_mapping(False)
    twin.calc_fem_state_and_force(fp.DT)
    fa, fb = fp.vertices(g, hs.ARR().FORCES), fp.vertices(twin, hs.ARR().FORCES)
    assert fa.any() and np.array_equal(hs.bits(fa), hs.bits(fb))
    wa, wb = g.weave_forces(), twin.weave_forces()
    assert wa.any() and np.array_equal(hs.bits(wa), hs.bits(wb))
    g.substep_end(fp.DT, -1)
    twin.destroy()
    run = fp.engine()
    _paths_weave(run)
    sp._begin_end(run)
    stats = run.stats()
    f = run.weave_forces()
    assert stats["error_flags"] == 0 and stats["substeps"] == fp.N and stats["rebuilds"] > 1, stats
    assert f.any() and np.isfinite(f).all()
    for e in (g, run):
        assert e.stats()["error_flags"] == 0
        e.destroy()


# ---- 5 -------------------------------------------------------------------------------------------------------------------
def test_off_means_off():
    """20 deterministic substeps through re-sorts: never set == all zeros == n_cloths = 0 == set and cleared, to the bit in
    x, v, C and F, and with the same launch counters (the quiet-time hint is in use again)"""
    from drake_amd import scenes
    from tests import transfer_layouts as tl
    pos, idx = scenes.cloth_sheet(32, 0.3, 0.6, (0.3, 0.5))
    es = [_engine([(pos, idx.reshape(-1, 3))]) for _ in range(4)]
    es[1].set_weave([(0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0)])
    es[2].set_weave([])
    es[3].set_weave([wv.DENIM + (1.0, 0.0, 0.0)])
    assert es[3].weave_max_stable_dt() < np.inf and es[3].weave_axes().any()
    es[3].set_weave([])
    for g in es:
        assert g.weave_max_stable_dt() == np.inf and not g.weave_forces().any() and not g.weave_axes().any()
        assert not g.weave_strain().any() and g.weave_energy()[1] == 0.0 and not g.get_weave()["E_warp"].any()
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
    for k in (1, 2, 3):
        for key in st[0]:
            assert np.array_equal(hs.bits(st[0][key]), hs.bits(st[k][key])), (k, key)
        for key in ("substeps", "rebuilds", "resort_checks"):
            assert es[0].stats()[key] == es[k].stats()[key], (k, key)
    for g in es:
        g.destroy()


# ---- 6 -------------------------------------------------------------------------------------------------------------------
def test_more_than_256_cloths():
    """A single-material engine holds any number of cloths: 300 lone triangles, one cloth each, the weave on every other
    one with constants and directions that change from cloth to cloth (0 and 256, 2 and 258 differ).  Every vertex has one
    record: the force is minus the record, compared with the host function to the bit and with float64 within the bound."""
    from drake_amd import weave_face_axes, weave_face_records
    X0, T0 = bd.mesh("triangle")
    n = 300
    meshes = []
    for c in range(n):
        off = np.array([(c % 20 - 9.5) * 2.5 * bd.H0, (c // 20 - 7.0) * 2.5 * bd.H0, 0.0])
        meshes.append(((X0.astype(np.float64) + off).astype(np.float32), T0))
    g = _engine(meshes)
    assert g.cloth_count() == n
    table = np.zeros((n, 7), np.float32)
    table[:, 4] = 1.0
    for c in range(0, n, 2):
        th = 0.3 + 0.01 * c
        table[c] = (1e5 * (1 + c % 7), 4e4 * (1 + c % 5), 0.1 + 0.001 * (c % 100), 5e2 * (1 + c % 3), np.cos(th), np.sin(th), 0.0)
    assert table[0, 0] != table[256, 0] or table[0, 5] != table[256, 5]
    g.set_weave(table)
    X = np.concatenate([m[0] for m in meshes])
    T = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    coef = np.stack([wv.coefficients(*table[c, :4]) for c in range(n)])
    cs, bad = weave_face_axes(wv.corners(T, X), table[:, 4:7])
    assert bad == -1
    cs[1::2] = 0.0
    assert np.array_equal(hs.bits(g.weave_axes()), hs.bits(cs))
    dm, vol = _rest(g)
    x = bd.state("perturbed", X)
    hs.upload(g, x)
    f, rec = g.weave_forces(records=True)
    host = weave_face_records(dm, vol, coef, cs, wv.corners(T, x))[0]
    host[1::2] = 0.0          # (the engine writes nothing there; the host function forms -0 from zero coefficients)
    assert np.array_equal(hs.bits(rec), hs.bits(host)) and np.array_equal(hs.bits(f.reshape(n, 3, 3)), hs.bits(0.0 - host))
    w = wv.margin(rec - wv.records64(dm, vol, coef, cs, wv.corners(T, x)), wv.record_bound(dm, vol, coef, cs, wv.corners(T, x)), R)
    _record("300 cloths", w)
    assert w <= 1.0, w
    assert not rec[1::2].any() and np.all(np.abs(rec[0::2]).max(axis=(1, 2)) > 0)
    rows, total = g.weave_energy()
    assert len(rows) == n and not rows[1::2].any() and (rows[0::2] > 0).all() and total == float(np.add.reduce(rows))
    mass = _by_id(g, hs.ARR().MASSES)[1].astype(np.float64)
    lim = wv.guard64(T, dm, vol, coef, mass)
    assert abs(g.weave_max_stable_dt() / lim - 1.0) < 1e-6, (g.weave_max_stable_dt(), lim)
    assert g.stats()["error_flags"] == 0
    g.destroy()


# ---- 7 -------------------------------------------------------------------------------------------------------------------
E_BASE = 2.0e5                                    # a soft matrix: half of E_weft, a twentieth of E_warp
HANG = (4.0e6, 4.0e5, 0.0, 4.0e3)                 # E_warp = 10 E_weft, a small G


def _hanging(warp_dir, steps, every=None):
    """a 16 x 16 sheet in the plane y = const, its top edge pinned to a resting body, under gravity along -z, with
    membrane damping; -> (mean strain along the load (vertical), the drop of the bottom edge, dt) at the end, or the
    list of them every `every` substeps"""
    from drake_amd import BodyMotion, Pin
    X, T = bd.sheet(16, 16)
    X = np.stack([X[:, 0], np.full(len(X), 0.5, np.float32), 0.5 + (X[:, 1] - 0.5)], 1).astype(np.float32)
    g = _engine([(X, T)], material=dict(youngs_modulus=E_BASE), bodies=1)
    g.set_body_motions([BodyMotion(0)])
    top = np.nonzero(X[:, 2] >= X[:, 2].max() - 1e-6)[0]
    bottom = np.nonzero(X[:, 2] <= X[:, 2].min() + 1e-6)[0]
    g.set_pins([Pin(int(v), 0, X[v]) for v in top])
    g.set_weave([HANG + tuple(warp_dir)])
    dt = 0.25 * g.weave_max_stable_dt()
    g.set_damping([(1.0, 0.0)])
    g.set_damping([(0.25 * g.damping_max_stable_dt() / dt, 0.0)])
    # the vertical in a face's (warp, weft) frame: u = (a . z, b . z); the strain along it is u^T E u.  The faces' rest
    # normal is -y here (the sheet of tests/bending.py with y and z exchanged), so the weft is b = n x a.
    a3 = np.asarray(warp_dir, np.float64) / np.linalg.norm(warp_dir)
    b3 = np.cross(np.array([0.0, -1.0, 0.0]), a3)
    ua, ub = a3[2], b3[2]

    def sample():
        e = g.weave_strain().astype(np.float64)
        along = e[:, 0] * ua * ua + e[:, 1] * ub * ub + 2.0 * e[:, 2] * ua * ub
        x = g.dump_cpu_state()[0]
        assert np.isfinite(x).all()
        return float(along.mean()), float((X[bottom, 2].astype(np.float64) - x[bottom, 2]).mean()), dt

    out = []
    for _ in range(steps // (every or steps)):
        g.run_substeps(every or steps, dt, -1)
        out.append(sample())
    g.gpu_sync()
    assert g.stats()["error_flags"] == 0 and g.weave_axes().any()
    g.destroy()
    return out if every else out[-1]


def test_hanging_twins():
    """the weft-hung twin stretches more along the load than the warp-hung one after the same number of substeps, by a
    ratio strictly between 1 and E_warp / E_weft -- the matrix adds to both: at rest (E_warp + E) / (E_weft + E) = 7 --; a
    third twin hung on the 45 degree bias, where only the small G and the matrix resist, drops more than either.
    2400 substeps (0.095 s): the slowest twin's first swing is over and the engine's own dissipation has taken most of the
    oscillation (measured on an MI355X: sampled every 300 substeps, the ratio stays between 6.0 and 8.7 from substep
    1200 to substep 3000).  Not
    longer: a sheet hung from pins creeps UPWARDS in this engine, with or without the weave (an isotropic sheet of
    E = 4e5 without weave loses its whole static drop of 1 mm in 0.3 s), which is not this feature's to explain, and the
    warp-hung twin's small strain is the first to drown in it."""
    steps = 2400
    warp = _hanging((0.0, 0.0, 1.0), steps)
    weft = _hanging((1.0, 0.0, 0.0), steps)
    bias = _hanging((1.0, 0.0, 1.0), steps)
    ratio = weft[0] / warp[0]
    _note(f"hanging twins, {steps} substeps of dt = {warp[2]:.3e}: mean strain along the load warp-hung {warp[0]:.4e}, weft-hung "
          f"{weft[0]:.4e}, ratio {ratio:.3f} (E_warp / E_weft = {HANG[0] / HANG[1]:.0f}); drop of the bottom edge warp {warp[1]:.4e}, "
          f"weft {weft[1]:.4e}, bias {bias[1]:.4e}")
    assert warp[0] > 0 and weft[0] > 0
    assert 1.0 < ratio < HANG[0] / HANG[1], ratio
    assert bias[1] > weft[1] > warp[1] > 0, (warp, weft, bias)


def test_released_sheet_does_not_gain_energy():
    """a 13 x 13 sheet released from a 5 % stretch along the warp (x), gravity 0, no damping: kinetic + the three elastic
    terms of mpm_measure + mpm_weave_energy, every 8 substeps, never exceeds its initial value by more than twice the
    largest upward excursion of the same scene without the weave (whose total has no weave term), measured here"""
    X, T = bd.mesh("regular")
    x0 = ((X.astype(np.float64) - bd.CENTER) * np.array([1.05, 1.0, 1.0]) + bd.CENTER).astype(np.float32)
    mat = dict(gravity=0.0, youngs_modulus=4.0e4)
    a, b = _engine([(X, T)], material=mat), _engine([(X, T)], material=mat)
    a.set_weave([(2.0e5, 2.0e4, 0.3, 1.0e3, 1.0, 0.0, 0.0)])
    dt = min(2e-4, 0.25 * a.weave_max_stable_dt())
    steps, every = 160, 8

    def total(g, weave):
        t = g.measure()[1]
        return float(t["kinetic"] + t["elastic_in_plane"] + t["elastic_normal"] + t["elastic_shear"]) + (g.weave_energy()[1] if weave else 0.0)

    series = {}
    for name, g in (("weave", a), ("twin", b)):
        hs.upload(g, x0)
        s = [total(g, name == "weave")]
        for _ in range(steps // every):
            g.run_substeps(every, dt, -1)
            s.append(total(g, name == "weave"))
        g.gpu_sync()
        assert g.stats()["error_flags"] == 0
        series[name] = np.array(s)
    up = {k: float(np.maximum(v - v[0], 0.0).max()) for k, v in series.items()}
    _note(f"released sheet, dt = {dt:.3e}, {steps} substeps sampled every {every}: initial total weave {series['weave'][0]:.6e}, twin "
          f"{series['twin'][0]:.6e}; largest upward excursion weave {up['weave']:.3e}, twin {up['twin']:.3e}; final weave "
          f"{series['weave'][-1]:.6e}, twin {series['twin'][-1]:.6e}")
    assert a.weave_energy()[1] < series["weave"][0] and series["weave"][0] > series["twin"][0] > 0
    assert up["weave"] <= 2.0 * up["twin"], (up, series["weave"][:6])
    for g in (a, b):
        g.destroy()


# ---- 8 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["big", "pair_multi"])
def test_guard_against_the_formula(name):
    """mpm_weave_max_stable_dt against guard64 from DM_INVERSES, the rest volumes, MPM_ARR_MASSES and the float table.
    1e-6: the engine forms the same sums in double from the same floats and rounds the result to float, towards zero."""
    s = _scene(name)
    g = _engine(s["meshes"], mats=s["mats"])
    _set_case(g, s, "30")
    mass = _by_id(g, hs.ARR().MASSES)[1].astype(np.float64)
    lim = wv.guard64(s["T"], s["rest"][0], s["rest"][1], s["coef_f"], mass)
    got = g.weave_max_stable_dt()
    print(f"weave guard {name}: engine {got:.9g}, formula {lim:.9g}")
    assert abs(got / lim - 1.0) < 1e-6 and got <= lim * (1 + 1e-12), (got, lim)
    g.destroy()


def test_refusals():
    from drake_amd import Collider, GpuMpm, MpmError
    from tests import transfer_layouts as tl

    def refused(call, says=None):
        with pytest.raises(MpmError) as e:
            call()
        assert e.value.code == -1, e.value
        if says:
            assert says in str(e.value), e.value

    X, T = bd.mesh("regular")
    g0 = GpuMpm(6)
    g0.add_qr_cloth(X, np.zeros_like(X), T)
    refused(lambda: g0.set_weave([wv.DENIM + (1.0, 0.0, 0.0)]), says="finalize")
    g0.destroy()

    g = _engine([(X, T)], bodies=1)
    good = np.array([wv.DENIM + (0.6, 0.8, 0.0)], np.float32)
    g.set_weave(good)
    lim = g.weave_max_stable_dt()
    x0 = bd.state("cylinder30", X)
    hs.upload(g, x0)
    f_before, axes_before = g.weave_forces(), g.weave_axes()
    assert f_before.any()
    nf = g.n_faces
    perp = np.zeros((nf, 3), np.float32)
    perp[17] = (1e-4, 0.0, 1.0)
    bad_tables = [[(-1.0, 1e4, 0.0, 1e2, 1, 0, 0)], [(1e5, -1e4, 0.0, 1e2, 1, 0, 0)], [(1e5, 1e4, 0.0, -1e2, 1, 0, 0)],
                  [(np.nan, 1e4, 0.0, 1e2, 1, 0, 0)], [(1e5, np.inf, 0.0, 1e2, 1, 0, 0)], [(1e5, 1e4, np.nan, 1e2, 1, 0, 0)],
                  [(1e4, 1e5, 0.4, 1e2, 1, 0, 0)],                  # D = 1 - 0.16 x 10 < 0
                  [(1e4, 1e4, 1.0, 1e2, 1, 0, 0)],                  # D = 0
                  [(0.0, 1e4, 0.2, 1e2, 1, 0, 0)],                  # E_warp = 0 with nu != 0
                  [(1e5, 1e4, 0.0, 1e2, 1, 0, 0)] * 2,              # a wrong count
                  [(1e5, 1e4, 0.0, 1e2, 0, 0, 1)],                  # the warp along the normal
                  [(1e5, 1e4, 0.0, 1e2, 0, 0, 0)],                  # a zero direction
                  [(1e5, 1e4, 0.0, 1e2, np.nan, 0, 0)]]
    for bad in bad_tables:
        refused(lambda bad=bad: g.set_weave(bad))
    refused(lambda: g.set_weave(good, perp), says="face 17")
    assert np.array_equal(g.get_weave().view(np.float32).reshape(-1, 7), good) and g.weave_max_stable_dt() == lim
    assert np.array_equal(hs.bits(g.weave_forces()), hs.bits(f_before)) and np.array_equal(hs.bits(g.weave_axes()), hs.bits(axes_before))
    # E_warp = 0 with nu = 0 is legal: kb = E_weft alone; a zero direction on a cloth WITHOUT weave is accepted
    g.set_weave([(0.0, 1e4, 0.0, 1e2, 1, 0, 0)])
    assert g.weave_forces().any()
    g.set_weave([(0.0, 0.0, 0.0, 0.0, 0, 0, 0)])
    assert g.weave_max_stable_dt() == np.inf
    g.set_weave(good)
    # partitioned, halo, team, chain and world calls on an engine with a weave
    nb = 64 // 4
    refused(lambda: g.dist_init(0, 1, [0, nb], 2, 2, 2), says="weave")
    refused(lambda: g.substep_mid_halo(tl.DT), says="weave")
    refused(lambda: g.team_prepare(), says="weave")
    refused(lambda: g.chain_substeps(1, tl.DT), says="weave")
    refused(lambda: g.substep_begin_halo(tl.DT, (0, None, None, None, None), 0), says="weave")
    refused(lambda: GpuMpm.world_coupled_substeps([g], 1, tl.DT, [Collider(0, body=0, p_WB=(0.5, 0.5, 0.3))], 0.5, 1e5, 1e-4),
            says="weave")
    # a dt above the limit: every entry point that takes one, nothing enqueued
    before = g.stats()["substeps"]
    big = 1.01 * lim
    floor = [Collider(0, body=0, p_WB=(0.5, 0.5, 0.3))]
    for call in (lambda: g.run_substeps(2, big, -1), lambda: g.substep(big, -1), lambda: g.particle_to_grid(big),
                 lambda: g.profile_substeps(2, big, -1), lambda: g.run_coupled_substeps(2, big, floor, 0.5, 1e5, 1e-4),
                 lambda: g.substep_begin(big)):
        refused(call, says="mpm_weave_max_stable_dt")
    assert g.stats()["substeps"] == before
    ok = 0.5 * lim
    g.run_substeps(2, ok, -1)
    ph, _ = g.profile_substeps(2, ok, -1)
    assert ph["fem"] > 0.0, ph
    g.gpu_sync()
    assert g.stats()["error_flags"] == 0
    # off lifts the refusals; a partitioned engine refuses the call
    g.set_weave([])
    g.run_substeps(1, big, -1)
    g.dist_init(0, 1, [0, nb], 2, 2, 2)
    refused(lambda: g.set_weave(good), says="partitioned")
    assert not g.get_weave()["E_warp"].any()
    g.destroy()
