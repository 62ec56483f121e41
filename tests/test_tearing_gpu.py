"""Tearing cloth (mpm_set_tearing, mpm_set_torn_faces) on the engine, 64^3 grid (tests/tearing.py holds the float64 model,
the scenes, the states and the bound that says which faces are undecided; undecided faces are skipped, nothing else).

1. After one mpm_calc_fem_state_and_force: the flags are float64's verdicts on every decided face, in every scene and
   state; mpm_tear_measure is the host function's bits.
2. Forces after one mpm_calc_fem_state_and_force: a vertex whose faces are all torn has force zero, a vertex without a
   torn face the bits of a twin without tearing, every other vertex the float64 sum over its intact faces within the
   per-face FEM bound of tests/fem_regimes.py; again with weave and damping on; with the forces formed inside k_p2g
   (valence 6, read behind ParticleToGrid) and by k_vforce (over DP::VF, and over DP::G3 on the hub).
3. Scissors: flags read back, counts per cloth, monotone, cleared by mpm_set_torn_faces alone.
4. Every fused substep path of tests/feature_paths.py leaves the same flags and the same state to the bit, substeps
   that skipped themselves included; run_coupled_substeps against the seven calls to the bit; substep_begin / end
   against itself under sparse re-sort checks; a shuffled particle order gives the same flags by original id.
5. Off means off.  6. Dynamics.  7. Refusals."""
import functools

import numpy as np
import pytest

from tests import bending as bd
from tests import harness as hs
from tests import tearing as tr

pytestmark = pytest.mark.gpu

U = tr.U
_CACHE = {}


_by_id = functools.partial(hs.by_id, split=True)


def _rest(g):
    A = hs.ARR()
    nf = g.n_faces
    return g.download(A.DM_INVERSES).reshape(nf, 4)[:, [0, 1, 3]].copy(), _by_id(g, A.VOLUMES)[0].copy()


def _fem(g, dt=None, p2g=False):
    """RebuildMapping + CalcFemStateAndForce; a download behind them launches the vertex forces as k_vforce.  p2g: also
    ParticleToGrid, after which the held-back calls go through the substep's path: on a mesh of valence <= 8 the vertex
    forces are formed inside k_p2g from DP::VF (fused_forces), which writes them out as well"""
    from tests import transfer_layouts as tl
    dt = tl.DT if dt is None else dt
    g.rebuild_mapping(False)
    g.calc_fem_state_and_force(dt)
    if p2g:
        g.particle_to_grid(dt)


def refused(call, says=None):
    from drake_amd import MpmError
    with pytest.raises(MpmError) as e:
        call()
    assert e.value.code == -1, e.value
    if says:
        assert says in str(e.value), e.value


# ---- 1 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(tr.SCENES))
def test_flags_are_float64_verdicts_and_measure_is_the_host_bits(name):
    from drake_amd import tear_face
    s = tr.scene(name)
    g = hs.engine(s["meshes"])
    g.set_tearing(s["limits"])
    assert np.array_equal(g.get_tearing(), s["limits"])
    dm, _ = _rest(g)
    tears = s["L_f"] > 0
    skipped = 0
    for st in tr.STATES:
        x = tr.state(st, s)
        g.set_torn_faces(np.zeros(g.n_faces, np.uint8))       # (restore: the flags are monotone across the states)
        hs.upload(g, x)
        assert np.array_equal(g.dump_cpu_state()[0], x)
        _fem(g)
        torn, count = g.tear_state()
        xc = tr.corners(s["T"], x)
        ref, decided = tr.verdict64(dm, xc, s["L_f"])
        assert (~decided).mean() <= tr.CAP, (name, st)
        skipped += int((~decided).sum())
        assert np.array_equal(torn[decided], ref[decided]), (name, st, int((torn != ref)[decided].sum()))
        assert not torn[~tears].any()
        assert np.array_equal(count, np.bincount(s["cof"], weights=torn, minlength=len(s["limits"])).astype(np.uint32))
        mq, would = g.tear_measure()
        host_mq, host_fails = tear_face(dm, xc, s["L_f"])
        assert np.array_equal(hs.bits(mq), hs.bits(host_mq)), (name, st)
        assert np.array_equal(would, host_fails & tears) and np.array_equal(would, torn), (name, st)
    print(f"tearing flags {name}: {skipped} undecided faces skipped over {len(tr.STATES)} states")
    assert g.stats()["error_flags"] == 0
    g.destroy()


# ---- 2 -------------------------------------------------------------------------------------------------------------------
C_ULP, K_STRICT = 64.0, 2.0      # tests/test_fem_regimes_gpu.py's constants of the per-face bound


def _extras(g, extras):
    """weave and membrane damping on every cloth -> (weave table, damping betas) or (None, None)"""
    from tests import transfer_layouts as tl
    if not extras:
        return None, None
    n = g.cloth_count()
    table = np.array([(2.0e5, 2.0e4, 0.3, 1.0e3, 0.6, 0.8, 0.0)] * n, np.float32)
    g.set_weave(table)
    g.set_damping([(1.0, 0.0)] * n)
    betas = np.array([(0.25 * g.damping_max_stable_dt() / tl.DT, 0.0)] * n, np.float32)
    g.set_damping(betas)
    return table, betas


@pytest.mark.parametrize("extras", [False, True], ids=["", "weave_damping"])
@pytest.mark.parametrize("name,fused", [("quad12", True), ("quad12", False), ("hub", False)],
                         ids=["quad12-fused_in_k_p2g", "quad12-k_vforce_VF", "hub-k_vforce_G3"])
def test_forces_of_torn_intact_and_mixed_vertices(name, fused, extras):
    """MPM_ARR_FORCES after one CalcFemStateAndForce.  The bound of a mixed vertex: the sum over its intact faces of the
    per-face bound of tests/test_fem_regimes_gpu.py, K_STRICT sens + C_ULP 2^-23 scale (fem_regimes.sensitivity and
    face_scales; no float oracle here, so the sensitivity stands alone), plus, with weave and damping on, their records'
    rounding bounds (tests/weave.py, tests/damping.py) and the roundings of the sums: a record is up to three float
    adds, a vertex with n records n - 1 more, each below 2^-24 of the sum of the absolute records.
    fused: the forces are read behind RebuildMapping, CalcFemStateAndForce AND ParticleToGrid: on quad12 (valence 6)
    the three held-back calls go through the substep's path, whose k_p2g forms the vertex forces from DP::VF itself and
    writes them out.  Not fused: they are read behind CalcFemStateAndForce, which launches k_vforce -- over DP::VF on
    quad12, over DP::VF and the hub's DP::G3 records on the hub (twelve faces: such an engine never fuses)."""
    from drake_amd import weave_face_axes
    from tests import damping as dp
    from tests import fem_regimes as fr
    from tests import transfer_layouts as tl
    from tests import weave as wv
    A = hs.ARR()
    s = tr.scene(name)
    a, b = hs.engine(s["meshes"]), hs.engine(s["meshes"])
    a.set_tearing(s["limits"])
    table = betas = None
    for g in (a, b):
        table, betas = _extras(g, extras)
    x0 = tr.state("uniaxial_rot", s)
    v0 = dp.velocity("random", x0).astype(np.float32)
    out = []
    F_up = None
    for g in (a, b):
        hs.upload(g, x0, v0)
        F_up = g.download(A.DEFORMATION_GRADIENTS)
        _fem(g, dt=0.5 * tl.DT, p2g=fused)                          # (ParticleToGrid checks dt against the weave's guard)
        out.append(_by_id(g, A.FORCES)[1].copy())
    fa, fb = out
    torn, _ = a.tear_state()
    assert torn.any() and not torn.all() and not b.tear_state()[0].any()
    T, nv, nf = s["T"], len(x0), len(s["T"])
    n_torn = np.bincount(T[torn].reshape(-1), minlength=nv)
    n_all = np.bincount(T.reshape(-1), minlength=nv)
    all_torn, none_torn = n_torn == n_all, n_torn == 0
    mixed = ~all_torn & ~none_torn
    assert all_torn.any() and none_torn.any() and mixed.any()
    assert not fa[all_torn].any(), "a vertex whose faces are all torn has a force"
    assert np.array_equal(hs.bits(fa[none_torn]), hs.bits(fb[none_torn]))
    assert np.abs(fb[all_torn]).max() > 0 and not np.array_equal(fa[mixed], fb[mixed])
    # the float64 records of the intact faces
    dm, vol = _rest(a)
    dm4 = a.download(A.DM_INVERSES).reshape(nf, 4)
    xc, vc = tr.corners(T, x0), tr.corners(T, v0)
    base = a.default_material()
    m = dict(fr.DEFAULT)
    m.update({k: getattr(base, k) for k in ("youngs_modulus", "poisson_ratio", "gamma", "K", "c_F")})
    mat = fr.Mat(m)
    args = (mat, F_up[:nf].astype(np.float64), np.zeros((nf, 9)), xc.astype(np.float64), dm4.astype(np.float64), vol)
    E = -fr.face64(*args)["force"]                                  # records: the force on a corner is -record
    v64 = dict(F=fr.face64(*args)["F"], vol=vol.astype(np.float64), xc=xc.astype(np.float64), vc=vc.astype(np.float64))
    sens = fr.sensitivity(*args)["force"]
    scale = fr.face_scales(v64, mat.E)["force"]
    face_tol = K_STRICT * sens + C_ULP * fr.EPS32 * scale           # (nf,), every component of the face's records
    rec, mag, tol = E.copy(), np.abs(E), np.broadcast_to(face_tol[:, None, None], E.shape).copy()
    if extras:
        Ey, nu = np.float32(m["youngs_modulus"]), np.float32(m["poisson_ratio"])
        mu, lam = Ey / (np.float32(2) * (np.float32(1) + nu)), Ey * nu / ((np.float32(1) + nu) * (np.float32(1) - np.float32(2) * nu))
        cs, bad = weave_face_axes(tr.corners(T, s["X"]), table[0, 4:7])
        assert bad == -1
        coef = wv.coefficients(*table[0, :4])
        W, D = wv.records64(dm, vol, coef, cs, xc), dp.records64(dm, vol, mu, lam, betas[0][0], xc, vc)
        rec = rec + W + D
        mag = mag + np.abs(W) + np.abs(D)
        tol = tol + wv.rounding_count() * U * wv.record_bound(dm, vol, coef, cs, xc) + \
            dp.rounding_count() * U * dp.record_bound(dm, vol, mu, lam, betas[0][0], xc, vc)
    keep = (~torn)[:, None, None]
    ref = dp.vertex_sum(T, nv, np.where(keep, rec, 0.0))
    bound = -dp.vertex_sum(T, nv, np.where(keep, tol, 0.0)) + (n_all + 2.0)[:, None] * U * -dp.vertex_sum(T, nv, np.where(keep, mag, 0.0))
    err = np.abs(fa.astype(np.float64) - ref)
    w = float((err[mixed] / bound[mixed]).max())
    print(f"tearing forces {name} fused={fused} extras={extras}: {int(torn.sum())} of {nf} faces torn, {int(mixed.sum())} mixed "
          f"vertices, worst {w:.3g} of the bound")
    assert w <= 1.0, w
    # the bound separates: leaving the torn faces IN would miss it
    full = dp.vertex_sum(T, nv, rec)
    assert float((np.abs(fa.astype(np.float64) - full)[mixed] / bound[mixed]).max()) > 10.0
    for g in (a, b):
        assert g.stats()["error_flags"] == 0
        g.destroy()


# ---- 3 -------------------------------------------------------------------------------------------------------------------
def test_scissors_counts_and_monotone_flags():
    s = tr.scene("pair")
    g = hs.engine(s["meshes"])
    nf = g.n_faces
    assert not g.tear_state()[0].any() and not g.tear_state()[1].any() and not g.get_tearing().any()
    cut = np.zeros(nf, bool)
    cut[[0, 5, 17, nf - 1, nf - 40]] = True
    g.set_torn_faces(cut)                                      # (allowed with every limit 0)
    torn, count = g.tear_state()
    assert np.array_equal(torn, cut) and np.array_equal(count, np.bincount(s["cof"], weights=cut).astype(np.uint32))
    g.set_tearing(s["limits"])
    assert np.array_equal(g.tear_state()[0], cut), "mpm_set_tearing changed the flags"
    hs.upload(g, tr.state("uniaxial", s))
    _fem(g)
    loaded = g.tear_state()[0]
    assert np.all(loaded[cut]) and loaded.sum() > cut.sum() and not loaded[(s["cof"] == 1) & ~cut].any()
    # the load goes, the flags stay; the limits go, the flags stay
    hs.upload(g, s["X"])
    _fem(g)
    assert np.array_equal(g.tear_state()[0], loaded) and not g.tear_measure()[1].any()
    g.set_tearing([0.0, 0.0])
    _fem(g)
    assert np.array_equal(g.tear_state()[0], loaded)
    # mpm_set_torn_faces alone clears
    g.set_torn_faces(cut)
    assert np.array_equal(g.tear_state()[0], cut)
    g.set_torn_faces(np.zeros(nf, bool))
    assert not g.tear_state()[0].any() and not g.tear_state()[1].any()
    assert g.stats()["error_flags"] == 0
    g.destroy()


# ---- 4 -------------------------------------------------------------------------------------------------------------------
PATH_FEATURES = frozenset(("materials", "damping", "links", "anchors", "pins", "fields"))      # what composes with tearing
PATH_LIMIT = 1.001


def _paths_run(name):
    from tests import feature_paths as fp
    key = ("paths", name)
    if key not in _CACHE:
        runner, env = fp.FUSED[name]
        g, cut = _armed(env)
        runner(g, -1)
        skipped = g.owed_substeps()
        st = fp.state(g)
        torn = _tear_words(g, st)
        _CACHE[key] = (st, g.stats(), skipped, cut, torn)
        g.destroy()
    return _CACHE[key]


@pytest.mark.parametrize("name", ["run_substeps_sparse_checks", "substeps", "profile_substeps", "phase_calls", "phase_calls_undeferred"])
def test_every_substep_path_ends_in_the_same_flags_and_bits(name):
    """tests/feature_paths.engine with every feature that composes with tearing, a pre-cut and a limit low enough to tear
    during the run: every runner of FUSED leaves the flags and the bits of run_substeps after N = 48 substeps, through
    re-sorts and substeps that skipped themselves"""
    from tests import feature_paths as fp
    (sa, ta, _, cut, torn), (sb, tb, skipped, _, _) = _paths_run("run_substeps"), _paths_run(name)
    for st in (ta, tb):
        assert st["error_flags"] == 0 and st["substeps"] == fp.N and st["rebuilds"] > 1, st
    assert ta["rebuilds"] == tb["rebuilds"]
    if name == "run_substeps_sparse_checks":
        assert skipped > 0, "no substep skipped itself with k_tear in it"
    assert np.all(torn[cut]) and cut.sum() < torn.sum() < len(torn), (int(cut.sum()), int(torn.sum()))
    assert set(sa) == set(sb)
    for k in sa:
        # (the states of the features that are off here -- shell bending -- are empty)
        assert np.array_equal(sa[k], sb[k]), (name, k, int((sa[k] != sb[k]).sum()))
    assert all(sa[k].size for k in ("pos", "vel", "C", "F", "pids", "torn", "count"))
    if name == "substeps":
        bare = fp.run("run_substeps", PATH_FEATURES)[0]
        assert not np.array_equal(bare["pos"], sa["pos"]), "tearing changed nothing"


def _tear_words(g, st):
    from tests import feature_paths as fp
    torn, count = g.tear_state()
    st.update(torn=fp.words(torn.astype(np.uint32)), count=fp.words(count))
    return torn


def _armed(env=None):
    """tests/feature_paths.engine with what composes with tearing, a pre-cut and the low limit"""
    from tests import feature_paths as fp
    g = fp.engine(PATH_FEATURES, env=env)
    cut = np.zeros(g.n_faces, bool)
    cut[::97] = True
    g.set_torn_faces(cut)
    g.set_tearing([PATH_LIMIT] * g.cloth_count())
    return g, cut


def test_coupled_equals_the_seven_calls():
    """run_coupled_substeps in two calls against the reference's seven calls per substep, over the floor the lower sheet
    reaches, with tearing on: the same contact rows, the same flags and counts, the same bits
    (tests/test_weave_gpu.py's comparison)"""
    from tests import feature_paths as fp
    out = []
    for runner in (lambda g: fp.seven_calls(g, fp.floor(), fp.N), lambda g: fp.coupled(g, fp.floor())):
        g, cut = _armed()
        rows = runner(g)
        st = fp.state(g)
        torn = _tear_words(g, st)
        out.append((st, g.stats(), rows, torn, cut))
        g.destroy()
    (sa, ta, ra, torn, cut), (sb, tb, rb, _, _) = out
    assert ta["error_flags"] == 0 and tb["error_flags"] == 0 and ta["substeps"] == tb["substeps"] == fp.N
    assert ta["rebuilds"] >= 2 and ta["rebuilds"] == tb["rebuilds"]
    contacts = [r["contacts"] for r in ra]
    assert max(contacts) > 0 and min(contacts) == 0, contacts
    for key in ("iterations", "contacts", "residual"):
        a, b = np.array([float(r[key]) for r in ra]), np.array([float(r[key]) for r in rb])
        assert np.all((a == b) | (np.isnan(a) & np.isnan(b))), key
    assert set(sa) == set(sb)
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), (k, int((sa[k] != sb[k]).sum()))
    assert np.all(torn[cut]) and cut.sum() < torn.sum() < len(torn), (int(cut.sum()), int(torn.sum()))


def test_sums_family_with_tearing():
    """substep_begin / substep_end (the member of the sums family that is not a halo call, which stay refused): one
    substep_begin leaves the flags and forces of RebuildMapping + CalcFemStateAndForce; N x (begin, end) ends in the
    same flags and the same bits with a re-sort check in front of every substep as with the sparse checks that make
    substeps skip themselves.  (The two families' particle states are not compared: gather + update from sums is
    another order of arithmetic.)"""
    from tests import feature_paths as fp
    from tests import substep_paths as sp
    x0, v0 = fp.perturbed_state()
    g, twin = fp.engine(PATH_FEATURES), fp.engine(PATH_FEATURES)
    for e in (g, twin):
        e.set_tearing([PATH_LIMIT] * e.cloth_count())
        fp.upload(e, x0, v0)
    refused(lambda: g.substep_mid_halo(fp.DT, -1), says="halo substeps: not available")
    g.substep_begin(fp.DT)
    twin.rebuild_mapping(False)
    twin.calc_fem_state_and_force(fp.DT)
    ta, tb = g.tear_state()[0], twin.tear_state()[0]
    assert ta.any() and np.array_equal(ta, tb)
    fa, fb = fp.vertices(g, hs.ARR().FORCES), fp.vertices(twin, hs.ARR().FORCES)
    assert np.array_equal(hs.bits(fa), hs.bits(fb))
    g.substep_end(fp.DT, -1)
    for e in (g, twin):
        e.destroy()
    out = []
    for env in (None, fp.SPARSE_CHECKS):
        run, cut = _armed(env)
        sp._begin_end(run)
        st = fp.state(run)
        torn = _tear_words(run, st)
        stats = run.stats()
        assert stats["error_flags"] == 0 and stats["substeps"] == fp.N and stats["rebuilds"] > 1, stats
        assert np.all(torn[cut]) and cut.sum() < torn.sum() < len(torn)
        out.append(st)
        run.destroy()
    assert set(out[0]) == set(out[1])
    for k in out[0]:
        assert np.array_equal(out[0][k], out[1][k]), (k, int((out[0][k] != out[1][k]).sum()))


def test_particle_order():
    """flags, counts and (m, q) by original id are the same bits on an engine whose slots have moved (substeps with a
    re-sort check forced on every substep, then the full sort) as on a fresh one, and in default mode; the forces of the
    fresh engines in both modes too (the moved engine's deformation gradients have a history of their own)"""
    s = tr.scene("quad12")
    env = {"MPM_RESORT_EVERY": "1", "MPM_QUIET_FACTOR": "0"}
    g, fresh, dflt = hs.engine(s["meshes"], env=env), hs.engine(s["meshes"]), hs.engine(s["meshes"], deterministic=False)
    pid0 = g.download(hs.ARR().PIDS)
    hs.upload(g, tr.state("shear_rot", s) + np.array([5.0 / 64, 0.0, 0.0], np.float32), np.array([3.0, 0.5, 0.0], np.float32))
    g.run_substeps(12, 1e-4, -1)
    g.gpu_sync()
    g.rebuild_mapping(True)
    assert not np.array_equal(g.download(hs.ARR().PIDS), pid0), "no slot moved"
    x = tr.state("uniaxial_rot", s)
    res = []
    for e in (g, fresh, dflt):
        e.set_tearing(s["limits"])
        hs.upload(e, x)
        _fem(e)
        torn, count = e.tear_state()
        res.append((torn, count, hs.bits(e.tear_measure()[0]), hs.bits(_by_id(e, hs.ARR().FORCES)[1])))
    assert res[0][0].any() and not res[0][0].all()
    for k in (1, 2):
        for a, b in zip(res[0][:3], res[k][:3]):
            assert np.array_equal(a, b), k
    assert np.array_equal(res[1][3], res[2][3])
    for e in (g, fresh, dflt):
        assert e.stats()["error_flags"] == 0
        e.destroy()


# ---- 5 -------------------------------------------------------------------------------------------------------------------
def test_off_means_off():
    """20 deterministic substeps through re-sorts: never set == a table of zeros == set, cleared and restored, to the bit
    in x, v, C and F, and with the same launch counters (the quiet-time hint is in use again)"""
    from drake_amd import scenes
    from tests import transfer_layouts as tl
    pos, idx = scenes.cloth_sheet(32, 0.3, 0.6, (0.3, 0.5))
    es = [hs.engine([(pos, idx.reshape(-1, 3))]) for _ in range(3)]
    es[1].set_tearing([0.0])
    es[2].set_tearing([1.5])
    es[2].set_torn_faces(np.arange(es[2].n_faces) % 7 == 0)
    es[2].set_tearing([0.0])
    assert es[2].tear_state()[0].any()
    es[2].set_torn_faces(np.zeros(es[2].n_faces, bool))
    for g in es:
        assert not g.tear_state()[0].any() and not g.get_tearing().any() and not g.tear_measure()[1].any()
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
    for k in (1, 2):
        for key in st[0]:
            assert np.array_equal(hs.bits(st[0][key]), hs.bits(st[k][key])), (k, key)
        for key in ("substeps", "rebuilds", "resort_checks"):
            assert es[0].stats()[key] == es[k].stats()[key], (k, key)
    for g in es:
        g.destroy()


def test_a_cloth_without_limit_is_its_twins_bits_while_the_other_tears():
    """two cloths 0.05 apart (more than three cells: no grid node in common), the first with a limit and stretched past
    it, the second without: 20 substeps leave the second cloth's particles with the bits of a twin engine without
    tearing, while the first cloth tears and differs"""
    s = tr.scene("pair")
    a, b = hs.engine(s["meshes"]), hs.engine(s["meshes"])
    a.set_tearing(s["limits"])
    x0 = tr.state("uniaxial", s)
    x0[s["first"][1]:] = tr.state("shear", s)[s["first"][1]:] * np.float32(1.0)     # (the second cloth strained too)
    for g in (a, b):
        hs.upload(g, x0)
        g.run_substeps(20, 2e-4, -1)
        g.gpu_sync()
        assert g.stats()["error_flags"] == 0
    torn = a.tear_state()[0]
    assert torn[s["cof"] == 0].any() and not torn[s["cof"] == 1].any()
    xa, va = a.dump_cpu_state()[:2]
    xb, vb = b.dump_cpu_state()[:2]
    second = slice(s["first"][1], None)
    assert np.array_equal(hs.bits(xa[second]), hs.bits(xb[second])) and np.array_equal(hs.bits(va[second]), hs.bits(vb[second]))
    assert not np.array_equal(xa[:s["first"][1]], xb[:s["first"][1]])
    Fa, Fb = a.download(hs.ARR().DEFORMATION_GRADIENTS), b.download(hs.ARR().DEFORMATION_GRADIENTS)
    assert np.array_equal(hs.bits(Fa[s["cof"] == 1]), hs.bits(Fb[s["cof"] == 1]))
    for g in (a, b):
        g.destroy()


# ---- 6 -------------------------------------------------------------------------------------------------------------------
STRIP_N, STRIP_M = 21, 9            # vertices along and across the strip: 20 x 8 quads, 320 faces
STRIP_V = 1.5                       # m/s: the left half starts at -STRIP_V, the right half at +STRIP_V
STRIP_DT, STRIP_EVERY, STRIP_SAMPLES = 1e-4, 40, 12


def _strip(limit):
    """a free strip of 20 x 8 quads, gravity off, no grips: its halves start with opposite velocities -+STRIP_V along its
    length, and a notch cut through the three lowest and the three highest quads of the middle column leaves the two
    quads in the middle to hold them together.  The grid mixes the momenta of the columns next to the cut while they
    share its nodes, so the ligament sees a part of 2 STRIP_V only; at 1.5 m/s that part takes it past the limit of 1.1.
    -> (vertex positions every STRIP_EVERY substeps, flags at each sample, rest positions, triangles, the notch
    column's faces, the notch)"""
    n, m = STRIP_N, STRIP_M
    X, T = bd.sheet(n, m)
    g = hs.engine([(X, T)], material=dict(gravity=0.0))
    col = n // 2 - 1                                                # quads between vertex columns 9 and 10
    quad_of_face = np.arange(len(T)) // 2                           # (sheet(): two faces per quad, quads in (i, j) order)
    in_col = quad_of_face // (m - 1) == col
    row = quad_of_face % (m - 1)
    notch = in_col & ((row < 3) | (row > 4))
    assert in_col.sum() == 16 and notch.sum() == 12
    v0 = np.zeros_like(X)                                           # (vertex i * m + j: column i)
    v0[:(col + 1) * m, 0], v0[(col + 1) * m:, 0] = -STRIP_V, STRIP_V
    g.set_torn_faces(notch)
    g.set_tearing([limit])
    hs.upload(g, X, v0)
    xs, flags = [], []
    for _ in range(STRIP_SAMPLES):
        g.run_substeps(STRIP_EVERY, STRIP_DT, -1)
        x = g.dump_cpu_state()[0].astype(np.float64)
        assert np.isfinite(x).all()
        xs.append(x)
        flags.append(g.tear_state()[0])
    g.gpu_sync()
    assert g.stats()["error_flags"] == 0
    g.destroy()
    return xs, flags, X.astype(np.float64), T, in_col, notch


def _component(T, intact, seeds, nv):
    """the vertices joined to `seeds` through intact faces"""
    label = np.arange(nv)
    faces = T[intact]
    while True:
        new = label.copy()
        np.minimum.at(new, faces.reshape(-1), np.repeat(label[faces].min(axis=1), 3))
        if np.array_equal(new, label):
            break
        label = new
    return np.isin(label, label[seeds])


def test_a_notched_strip_tears_through_and_its_halves_part():
    """the strip with a limit loses every face of the notch's column (and, where the grid has spread the jump of the
    velocity over the columns next to it, faces of those): no chain of intact faces joins its two ends any more.  The
    two HALVES are what still hangs together with either end, free vertices all; the gap is the least x of the right
    half minus the greatest x of the left one, less its rest value.  From the first sample at which the strip has
    parted the gap grows from sample to sample -- nothing joins the halves and each keeps its momentum, less what the
    grid mixes while they share nodes -- and ends beyond what joined cloth allows, the bound that follows.
    The twin without a limit never tears.  Between the same two sets of vertices its cloth stops the halves: their
    kinetic energy, rho t A v^2 with A = 80 h^2 per half, put into the two ligament quads alone, mu t 2 h^2 (x / h)^2
    with mu = E / 2.6, allows x = h v sqrt(80 rho / (2 mu)) = 1.08 h; with up to eight whole columns in series, four
    times as stiff each, sqrt(3) times that, 1.87 h.  Its gap is held below two spacings at every sample; the torn
    strip's must end above them."""
    xs, flags, X, T, in_col, notch = _strip(tr.LIMIT)
    xs0, flags0, _, _, _, _ = _strip(0.0)
    assert all(np.array_equal(f, notch) for f in flags0), "the twin tore"
    for a, b in zip(flags[:-1], flags[1:]):
        assert np.all(b[a]), "a flag was cleared"
    nv, m = len(X), STRIP_M
    ends = np.arange(m), np.arange(nv - m, nv)
    parted = [bool(np.all(f[in_col])) and not _component(T, ~f, ends[0], nv)[ends[1]].any() for f in flags]
    assert any(parted), "the strip did not tear through"
    k = parted.index(True)
    assert k <= len(xs) - 4 and all(parted[k:])
    L, R = _component(T, ~flags[-1], ends[0], nv), _component(T, ~flags[-1], ends[1], nv)
    assert not (L & R).any() and L.sum() >= 5 * m and R.sum() >= 5 * m, (int(L.sum()), int(R.sum()))
    rest = X[R, 0].min() - X[L, 0].max()
    assert rest <= 9 * bd.H0 * 1.001, "more than eight columns between the halves"
    gap = np.array([x[R, 0].min() - x[L, 0].max() - rest for x in xs])
    gap0 = np.array([x[R, 0].min() - x[L, 0].max() - rest for x in xs0])
    print("tearing strip: gap " + " ".join(f"{x:.4e}" for x in gap) + "; twin " + " ".join(f"{x:.4e}" for x in gap0) +
          f"; parted at sample {k}; torn {[int(f.sum()) for f in flags]}; halves {int(L.sum())} + {int(R.sum())} vertices")
    assert np.all(np.diff(gap[k:]) > 0), gap
    assert gap[-1] > 2.0 * bd.H0, gap
    assert np.abs(gap0).max() < 2.0 * bd.H0, gap0


HANG_H = 3.0 / 128      # the hanging sheet's spacing: three cells of the 128^3 grid


def _hanging(cut_row):
    """a 13 x 13 sheet (288 faces) of spacing HANG_H in the plane y = const of a 128^3 grid, its top edge pinned to a
    resting body, under gravity along -z; cut_row: every face of one row of quads below the middle is cut first.  -> the
    mean drop of the vertices below the cut after 600 substeps of 2e-4 s.
    The spacing is three cells because the two sides of a cut share the grid's velocity field while they are within
    about two cells of each other -- the method's own cohesion, which no face force can switch off.  A cut that is to
    let a part go under a uniform load must be wider than that."""
    from drake_amd import BodyMotion, Pin
    X, T = bd.sheet(13, 13, h=HANG_H)
    X = np.stack([X[:, 0], np.full(len(X), 0.5, np.float32), 0.5 + (X[:, 1] - 0.5)], 1).astype(np.float32)
    g = hs.engine([(X, T)], bits=7, bodies=1)
    g.set_body_motions([BodyMotion(0)])
    top = np.nonzero(X[:, 2] >= X[:, 2].max() - 1e-6)[0]
    g.set_pins([Pin(int(v), 0, X[v]) for v in top])
    zc = X[T].astype(np.float64).mean(axis=1)[:, 2]
    zs = np.unique(np.round(X[:, 2].astype(np.float64), 5))
    assert len(zs) == 13
    lo, hi = zs[4], zs[5]                                            # the fifth row of quads from the bottom
    row = (zc > lo) & (zc < hi)
    assert row.sum() == 24
    if cut_row:
        g.set_torn_faces(row)
    below = X[:, 2] <= lo + 1e-6
    g.run_substeps(600, 2e-4, -1)
    x = g.dump_cpu_state()[0]
    g.gpu_sync()
    assert g.stats()["error_flags"] == 0 and np.isfinite(x).all()
    torn = g.tear_state()[0]
    assert np.array_equal(torn, row if cut_row else np.zeros(len(T), bool))
    g.destroy()
    return float((X[below, 2].astype(np.float64) - x[below, 2]).mean())


def test_a_hanging_sheet_cut_along_a_row_drops_its_lower_part():
    """0.12 s: free fall is 1/2 g t^2 = 70.6 mm.  The part below the cut still shares grid nodes with the part above
    during the first cells of its fall and is slowed by them, so it is asked for a fifth of the free fall; the uncut twin
    hangs: its lower part moves by less than a fifth of what the cut one's does"""
    cut, whole = _hanging(True), _hanging(False)
    fall = 0.5 * 9.81 * 0.12 ** 2
    print(f"tearing hanging sheet: drop of the lower part cut {cut:.4e}, uncut {whole:.4e} (free fall {fall:.4e})")
    assert cut > 0.2 * fall and abs(whole) < 0.2 * cut, (cut, whole)


def test_measure_drops_the_torn_faces_share_and_keeps_the_momenta():
    """mpm_measure before and after a cut on a strained, moving sheet: the three strain energies drop by the cut faces'
    share (mpm_face_strain's V psi before the cut; 1e-6: floats summed against doubles), mass and momenta are the same
    bits, the cut faces report V psi = 0 and leave the stretch extremes"""
    from tests import damping as dp
    s = tr.scene("quad12")
    g = hs.engine(s["meshes"])
    x = tr.state("uniaxial", s)
    hs.upload(g, x, dp.velocity("random", x).astype(np.float32))
    _fem(g)
    rows0, tot0 = g.measure()
    fs0 = g.face_strain()
    cut = np.zeros(g.n_faces, bool)
    cut[np.argsort(fs0[:, 0])[-40:]] = True                         # the forty most stretched faces
    g.set_torn_faces(cut)
    rows1, tot1 = g.measure()
    fs1 = g.face_strain()
    elastic = lambda t: float(t["elastic_in_plane"] + t["elastic_normal"] + t["elastic_shear"])   # noqa: E731
    share = float(fs0[cut, 3].astype(np.float64).sum())
    assert share > 0.1 * elastic(tot0)
    assert abs(elastic(tot1) - (elastic(tot0) - share)) <= 1e-6 * elastic(tot0), (elastic(tot0), elastic(tot1), share)
    for key in ("mass", "momentum", "angular_momentum", "kinetic", "faces", "vertices"):
        if key in tot0.dtype.names:
            assert np.array_equal(np.asarray(tot0[key]), np.asarray(tot1[key])), key
    assert "mass" in tot0.dtype.names and "momentum" in tot0.dtype.names
    assert not fs1[cut, 3].any() and np.array_equal(hs.bits(fs1[~cut]), hs.bits(fs0[~cut]))
    assert np.array_equal(hs.bits(fs1[:, :3]), hs.bits(fs0[:, :3]))
    assert tot1["stretch_max"] == fs0[~cut, 0].max() < tot0["stretch_max"]
    g.set_torn_faces(np.zeros(g.n_faces, bool))
    assert g.measure()[1].tobytes() == tot0.tobytes()
    g.destroy()


# ---- 7 -------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from drake_amd import PRESSURE_CONSTANT, PRESSURE_DTYPE, Collider, GpuMpm
    from tests import transfer_layouts as tl
    s = tr.scene("pair")
    (X, T) = s["meshes"][0]
    g0 = GpuMpm(6)
    g0.add_qr_cloth(X, np.zeros_like(X), T)
    refused(lambda: g0.set_tearing([1.1]), says="finalize")
    refused(lambda: g0.set_torn_faces(np.zeros(len(T), bool)), says="finalize")
    g0.destroy()

    g = hs.engine(s["meshes"], bodies=1)
    nf = g.n_faces
    for bad in ([1.0, 0.0], [0.5, 0.0], [-1.1, 0.0], [np.nan, 0.0], [np.inf, 0.0], [1.1, 0.999]):
        refused(lambda bad=bad: g.set_tearing(bad), says="stretch_limit")
    for bad in ([1.1], [1.1, 0.0, 0.0], []):
        refused(lambda bad=bad: g.set_tearing(bad), says="n_cloths")
    assert not g.get_tearing().any() and not g.tear_state()[0].any()

    def pressure(c):
        t = np.zeros(2, PRESSURE_DTYPE)
        t["mode"][c], t["p"][c] = PRESSURE_CONSTANT, 10.0
        return t

    cut1 = np.zeros(nf, bool)
    cut1[nf - 1] = True                                             # a face of cloth 1
    # the other feature first: tearing refuses that cloth, in both of its calls, and accepts the other cloth
    for setter, clear, says in ((lambda: g.set_bending([0.0, 1e-6]), lambda: g.set_bending([]), "mpm_set_bending"),
                                (lambda: g.set_shell_bending([0.0, 1e-6]), lambda: g.set_shell_bending([]), "mpm_set_shell_bending"),
                                (lambda: g.set_pressure(pressure(1)), lambda: g.set_pressure([]), "mpm_set_pressure")):
        setter()
        refused(lambda: g.set_tearing([0.0, 1.2]), says=says)
        refused(lambda: g.set_torn_faces(cut1), says=says)
        g.set_tearing([1.2, 0.0])
        g.set_torn_faces(~cut1 & (np.arange(nf) == 0))
        assert g.tear_state()[1].tolist() == [1, 0]
        g.set_torn_faces(np.zeros(nf, bool))
        g.set_tearing([0.0, 0.0])
        clear()
    # tearing first: the other features refuse that cloth (a limit, or a torn face alone) and accept the other
    for arm, disarm in ((lambda: g.set_tearing([0.0, 1.2]), lambda: g.set_tearing([0.0, 0.0])),
                        (lambda: g.set_torn_faces(cut1), lambda: g.set_torn_faces(np.zeros(nf, bool)))):
        arm()
        refused(lambda: g.set_bending([0.0, 1e-6]), says="mpm_set_tearing")
        refused(lambda: g.set_shell_bending([0.0, 1e-6]), says="mpm_set_tearing")
        refused(lambda: g.set_pressure(pressure(1)), says="mpm_set_tearing")
        g.set_bending([1e-6, 0.0])
        g.set_shell_bending([1e-6, 0.0])
        g.set_pressure(pressure(0))
        g.set_bending([])
        g.set_shell_bending([])
        g.set_pressure([])
        disarm()
    # partitioned, halo, team, chain and world calls on an engine with tearing
    g.set_tearing([1.2, 0.0])
    nb = 64 // 4
    refused(lambda: g.dist_init(0, 1, [0, nb], 2, 2, 2), says="tearing")
    refused(lambda: g.substep_mid_halo(tl.DT), says="tearing")
    refused(lambda: g.team_prepare(), says="tearing")
    refused(lambda: g.chain_substeps(1, tl.DT), says="tearing")
    refused(lambda: g.substep_begin_halo(tl.DT, (0, None, None, None, None), 0), says="tearing")
    refused(lambda: GpuMpm.world_coupled_substeps([g], 1, tl.DT, [Collider(0, body=0, p_WB=(0.5, 0.5, 0.3))], 0.5, 1e5, 1e-4),
            says="tearing")
    g.run_substeps(2, tl.DT, -1)
    g.gpu_sync()
    assert g.stats()["error_flags"] == 0
    # off lifts the refusals; a partitioned engine refuses the calls
    g.set_tearing([0.0, 0.0])
    assert not g.tear_state()[0].any()
    g.dist_init(0, 1, [0, nb], 2, 2, 2)
    refused(lambda: g.set_tearing([1.2, 0.0]), says="partitioned")
    refused(lambda: g.set_torn_faces(cut1), says="partitioned")
    g.destroy()
