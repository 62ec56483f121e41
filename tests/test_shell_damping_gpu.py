"""Hinge damping of the shell model (mpm_set_shell_damping) on the engine.  tests/shell_damping.py is the float64 model,
the float32 restatement and the counted bound (R_SHELL_DAMP = 62.5 + n_i per row, psidot 29).

1. mpm_shell_damping_forces, psidot and the power on every mesh x state x velocity state: against the restatement's bits
   (the host function's, tests/test_shell_damping.py) and against float64 within the bound; mpm_shell_forces keeps
   reporting the elastic part alone; MPM_ARR_FORCES of one CalcFemStateAndForce minus a twin's without shell bending is
   the gather of the damped hinge's records, within one rounding of the sum.
2. The layout strips around a wave and a block.
3. Three cloths in one engine: damped, shell with beta = 0, no shell.
4. The same bits after forced re-sorts and in non-deterministic mode.
5. Every feature on, every path: the fused family bit-equal, the coupled path against the seven calls through substeps
   that skipped themselves.
6. Creases: the psibar a substep leaves is mpm_crease_measure's prediction, whatever beta.
7. A cut hinge's records are exact zeros under any velocities; restored, it acts again.
8. Off means off; set, get, replace; mpm_set_shell_bending drops the table.
9. The guard; refusals.
10. Dynamics, orderings only."""

import functools

import numpy as np
import pytest

from tests import bending as bd
from tests import creases as cr
from tests import harness as hs
from tests import shell_bending as sb
from tests import shell_damping as sd
from tests import shell_scenes as ss
from tests import transfer_layouts as tl

pytestmark = pytest.mark.gpu

U = sb.U
F = np.float32


_record = functools.partial(hs.record, prefix="shell damping: ")


def _refused(call, says=()):
    from drake_amd import MpmError
    with pytest.raises(MpmError) as e:
        call()
    assert e.value.code == -1, e.value
    for s in (says,) if isinstance(says, str) else says:
        assert s in str(e.value), e.value


def _bkc(beta, k, cbar):
    return (float(F(beta)) * float(F(k)) * np.asarray(cbar, np.float64)).astype(F)


def _sum_in_order(terms):
    s = 0.0
    for t in np.asarray(terms, F):
        s += float(t)
    return s


def _check(g, x0, v0, H, kc, psibar, bkc, what, cloth_of_hinge=None, n_cloths=1):
    """mpm_shell_damping_forces / _state of the engine on the uploaded state against the restatement's bits and float64"""
    fd = g.shell_damping_forces()
    power, pd = g.shell_damping_state()
    rec, _, pd32, pw32, on = sd.hinges32(x0, v0, H, kc, psibar, bkc, elastic=False)
    assert np.array_equal(hs.bits(fd), hs.bits(sb.gather32(rec, H, len(x0)))), (what, float(np.abs(fd - sb.gather32(rec, H, len(x0))).max()))
    assert np.array_equal(hs.bits(pd), hs.bits(pd32)), what
    ch = np.zeros(len(H), int) if cloth_of_hinge is None else cloth_of_hinge
    for c in range(n_cloths):
        assert power[c] == _sum_in_order(pw32[ch == c]) and power[c] >= 0.0, (what, c)
    x64, v64 = x0.astype(np.float64), v0.astype(np.float64)
    B, N = sd.row_bounds(x64, v64, H, bkc, on)
    w = sd.share(fd - sd.force64(x64, v64, H, bkc, on), B, sd.R_SHELL_DAMP + N)
    _, pu = sd.scales(x64, v64, H, bkc, on)
    _, pd64, pw64 = sd.records64(x64, v64, H, bkc, on)
    wp = sd.share(pd - pd64, pu, sd.R_PSIDOT)
    pb = sd.power_bound(x64, v64, H, bkc, on)
    we = 0.0
    for c in range(n_cloths):
        err, tol = abs(power[c] - pw64[ch == c].sum()), pb[ch == c].sum() + 1e-15 * pw64[ch == c].sum()
        we = max(we, err / tol if err > 0 else 0.0)
    print(f"shell damping: {what}: force {w:.3g}, psidot {wp:.3g}, power {we:.3g} of the bound")
    _record("forces: " + what, w), _record("psidot: " + what, wp), _record("power: " + what, we)
    assert w <= 1.0 and wp <= 1.0 and we <= 1.0, (what, w, wp, we)
    assert np.isfinite(fd).all() and not fd[N == 0].any()
    return fd


# ---- 1 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,st", sb.CASES)
def test_forces_psidot_and_power_against_float64_and_the_restatement(name, st):
    from drake_amd import SHELL_DAMPING_DTYPE
    A = hs.ARR()
    X, T, rest = sb.mesh(name)
    H = sb.hinges(T)
    a, b = hs.engine([(X, T)]), hs.engine([(X, T)])
    a.set_shell_bending([sb.K], rest)
    if len(H) == 0:                    # (no hinge: shell bending is not in force)
        _refused(lambda: a.set_shell_damping([sd.BETA]), says="shell bending")
        a.destroy(), b.destroy()
        return
    elastic_limit = a.shell_max_stable_dt()
    a.set_shell_damping([sd.BETA])
    want = np.zeros(1, SHELL_DAMPING_DTYPE)
    want["beta"] = sd.BETA
    assert np.array_equal(a.get_shell_damping(), want) and a.shell_max_stable_dt() < elastic_limit
    ids, kc, psibar = a.shell_hinges()
    assert np.array_equal(ids, H)
    bkc = _bkc(sd.BETA, sb.K, sb.cbar64(sb.rest_shape(name).astype(np.float64), H))
    x0 = sb.state(name, st)
    dt = min(1e-5, 0.5 * a.shell_max_stable_dt())
    el32 = sb.gather32(sb.hinges32(x0, H, kc, psibar)[0], H, len(x0))
    for kind in sd.VELOCITIES:
        v0 = sd.velocity(name, st, kind)
        hs.upload(a, x0, v0)
        fd = _check(a, x0, v0, H, kc, psibar, bkc, f"{name} {st} {kind}")
        if kind in ("zero", "common"):
            assert not fd.any()
        assert np.array_equal(hs.bits(a.shell_forces()), hs.bits(el32))            # (the elastic part alone, whatever v)
        if st == "collinear":          # (its face of zero area: the membrane model's forces are not finite there)
            continue
        out = []
        for g in (a, b):
            hs.upload(g, x0, v0)
            g.rebuild_mapping(False)
            g.calc_fem_state_and_force(dt)
            out.append(hs.vertices(g, A.FORCES).astype(np.float64))
        full = sb.gather32(sd.hinges32(x0, v0, H, kc, psibar, bkc)[0], H, len(x0)).astype(np.float64)
        err = np.abs(out[0] - (out[1] + full))
        assert (err <= U * np.abs(out[0])).all(), (name, st, kind, float((err / np.maximum(np.abs(out[0]), 1e-300)).max()))
    for g in (a, b):
        assert g.stats()["error_flags"] == 0
        g.destroy()


# ---- 2 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_faces", cr.STRIPS)
def test_strips_around_a_wave_and_a_block(n_faces):
    X, T, x = cr.strip(n_faces)
    H = sb.hinges(T)
    assert len(H) == n_faces - 1
    g = hs.engine([(X, T)])
    g.set_shell_bending([sb.K])
    g.set_shell_damping([sd.BETA])
    ids, kc, psibar = g.shell_hinges()
    bkc = _bkc(sd.BETA, sb.K, sb.cbar64(X.astype(np.float64), H))
    v = np.random.default_rng(n_faces).normal(size=x.shape).astype(F)
    hs.upload(g, x, v)
    fd = _check(g, x, v, H, kc, psibar, bkc, f"strip of {n_faces} faces")
    assert fd[H[-1]].any() and fd[H[0]].any()             # (the last hinge of the last wave wrote its records)
    g.rebuild_mapping(False)
    g.calc_fem_state_and_force(min(1e-5, 0.5 * g.shell_max_stable_dt()))
    assert np.isfinite(hs.vertices(g, hs.ARR().FORCES)).all() and g.stats()["error_flags"] == 0
    g.destroy()


# ---- 3 -------------------------------------------------------------------------------------------------------------------
def test_three_cloths_damped_undamped_and_without_shell():
    A = hs.ARR()
    cloths, _, x = cr.three_cloths(0.8)
    first = np.cumsum([0] + [len(X) for X, _ in cloths])
    a, b = hs.engine(cloths), hs.engine(cloths)
    for g in (a, b):
        g.set_shell_bending([sb.K, sb.K, 0.0])
    a.set_shell_damping([sd.BETA, 0.0, sd.BETA])          # (beta > 0 on the cloth without hinges: accepted, does nothing)
    assert a.shell_max_stable_dt() < b.shell_max_stable_dt()
    ids, kc, psibar = a.shell_hinges()
    H = ids.astype(np.int64)
    ch = np.searchsorted(first, H[:, 0], side="right") - 1
    assert set(ch) == {0, 1}
    Xall = np.concatenate([X for X, _ in cloths]).astype(np.float64)
    bkc = _bkc(sd.BETA, sb.K, sb.cbar64(Xall, H))
    bkc[ch == 1] = 0.0
    v = np.random.default_rng(9).normal(size=x.shape).astype(F)
    hs.upload(a, x, v)
    fd = _check(a, x, v, H, kc, psibar, bkc, "three cloths", ch, 3)
    power, pd = a.shell_damping_state()
    assert fd[first[0]:first[1]].any() and not fd[first[1]:].any()
    assert power[0] > 0 and power[1] == 0 and power[2] == 0 and pd[ch == 1].any()     # (psidot is reported for every hinge)
    dt = min(1e-5, 0.5 * a.shell_max_stable_dt())
    out = []
    for g in (a, b):
        hs.upload(g, x, v)
        g.rebuild_mapping(False)
        g.calc_fem_state_and_force(dt)
        out.append(hs.vertices(g, A.FORCES))
    # the undamped shell cloth and the cloth without shell bending: the twin's bits; the damped one differs
    assert np.array_equal(hs.bits(out[0][first[1]:]), hs.bits(out[1][first[1]:]))
    assert not np.array_equal(hs.bits(out[0][:first[1]]), hs.bits(out[1][:first[1]]))
    assert not b.shell_damping_forces().any() and not b.get_shell_damping()["beta"].any()
    pb, pdb = b.shell_damping_state()
    assert not pb.any() and np.array_equal(hs.bits(pdb), hs.bits(pd))                 # (psidot without a damper: the same bits)
    for g in (a, b):
        assert g.stats()["error_flags"] == 0
        g.destroy()


# ---- 4 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deterministic", [True, False])
def test_particle_order_and_determinism_mode(deterministic):
    cloths, rest, H, ch = ss.scene()
    g = hs.engine(cloths, deterministic=deterministic)
    g.set_shell_bending([sb.K, sb.K], rest)
    g.set_shell_damping([sd.BETA, 0.5 * sd.BETA])
    x0 = bd.perturbed(rest, seed=7).astype(F)
    v0 = np.random.default_rng(4).normal(size=x0.shape).astype(F)
    hs.upload(g, x0, v0)
    f0, s0 = g.shell_damping_forces(), g.shell_damping_state()
    assert f0.any()
    before = g.stats()["rebuilds"]
    hs.upload(g, x0 + np.array([5.0 / 64, 0.0, 0.0], F), np.zeros_like(v0))
    g.run_substeps(2, 1e-5, -1)
    g.gpu_sync()
    assert g.stats()["error_flags"] == 0 and g.stats()["rebuilds"] > before, g.stats()
    for sort in (False, True):
        if sort:
            g.rebuild_mapping(True)
        hs.upload(g, x0, v0)
        f1, s1 = g.shell_damping_forces(), g.shell_damping_state()
        assert np.array_equal(hs.bits(f1), hs.bits(f0)) and np.array_equal(hs.bits(s1[0]), hs.bits(s0[0])) and np.array_equal(hs.bits(s1[1]), hs.bits(s0[1]))
    g.destroy()


# ---- 5 -------------------------------------------------------------------------------------------------------------------
def _fp_engine(env=None):
    """tests/feature_paths.py's every-feature engine with the hinge damper on top, beta half a substep on every shell cloth"""
    from tests import feature_paths as fp
    g = fp.engine(env=env)
    n = g.cloth_count()
    g.set_shell_damping([0.5 * fp.DT] * n)
    assert fp.DT <= g.shell_max_stable_dt(), g.shell_max_stable_dt()
    return g


def _fp_state(g):
    from tests import feature_paths as fp
    st = fp.state(g)
    power, pd = g.shell_damping_state()
    st["damping_power"], st["damping_psidot"], st["forces_shell_damping"] = fp.words(power), fp.words(pd), fp.words(g.shell_damping_forces())
    return st


def _same_state(a, b, what):
    assert set(a) == set(b)
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (what, k, int((a[k] != b[k]).sum()))


def test_every_feature_with_the_damper_on_every_path():
    from tests import feature_paths as fp
    ref = None
    for name in ("run_substeps", "run_substeps_sparse_checks", "substeps", "phase_calls"):
        runner, env = fp.FUSED[name]
        g = _fp_engine(env)
        runner(g, -1)
        st, stats = _fp_state(g), g.stats()
        g.destroy()
        assert stats["error_flags"] == 0 and stats["substeps"] == fp.N and stats["rebuilds"] > 1, (name, stats)
        if ref is None:
            ref = st
            assert fp.floats(st, "forces_shell_damping").any() and np.isfinite(fp.floats(st, "vel")).all()
            assert (fp.floats(st, "damping_power", np.float64) >= 0).all() and fp.floats(st, "damping_power", np.float64).any()
        else:
            _same_state(ref, st, name)
    # the damper changes that run
    g = fp.engine()
    fp.FUSED["run_substeps"][0](g, -1)
    plain = fp.state(g)
    g.destroy()
    assert not np.array_equal(plain["vel"], ref["vel"])


def test_coupled_equals_the_seven_calls_through_skipped_substeps():
    from tests import feature_paths as fp
    a = _fp_engine()
    ra = fp.seven_calls(a, fp.floor(), fp.N)
    sa, ta = _fp_state(a), a.stats()
    a.destroy()
    b = _fp_engine({"MPM_CT_GATE_ALWAYS": "1", "MPM_CT_NO_WATCH": "1"})
    rb = fp.coupled(b, fp.floor())
    sb_, tb, cb = _fp_state(b), b.stats(), b.contact_counters()
    b.destroy()
    assert ta["error_flags"] == 0 and tb["error_flags"] == 0 and ta["substeps"] == fp.N == tb["substeps"]
    assert ta["rebuilds"] >= 2 and ta["rebuilds"] == tb["rebuilds"] and cb["refused_stale"] >= 1, (ta, tb, cb)
    assert [r["contacts"] for r in ra] == [r["contacts"] for r in rb] and max(r["contacts"] for r in ra) > 0
    _same_state(sa, sb_, "coupled, gate always")          # (a damping force added twice would show in vel)


# ---- 6 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", [0.0, sd.BETA, 4 * sd.BETA])
def test_creases_yield_on_the_elastic_moment_alone(beta):
    from drake_amd import CREASE_DTYPE
    cloths, rows, x = cr.three_cloths()
    g = hs.engine(cloths)
    g.set_shell_bending([sb.K] * 3)
    t = np.zeros(3, CREASE_DTYPE)
    for c, (ya, eta, ma) in enumerate(rows):
        t[c] = (ya, eta, ma, 0.0)
    g.set_creases(t)
    g.set_shell_damping([beta] * 3)
    v = np.random.default_rng(3).normal(size=x.shape).astype(F)
    hs.upload(g, x, v)
    psi, dpsi, nxt = g.crease_measure()
    before = g.crease_state()[0]
    g.rebuild_mapping(False)
    g.calc_fem_state_and_force(min(1e-5, 0.5 * g.shell_max_stable_dt()))
    after = g.crease_state()[0]
    assert np.array_equal(hs.bits(after), hs.bits(nxt)) and (hs.bits(after) != hs.bits(before)).any()
    # whatever beta: the same psibar as the undamped engine leaves (computed once, shared)
    key = "psibar"
    if key not in _CREASED:
        _CREASED[key] = hs.bits(after).copy()
    assert np.array_equal(hs.bits(after), _CREASED[key])
    assert g.stats()["error_flags"] == 0
    g.destroy()


_CREASED = {}


# ---- 7 -------------------------------------------------------------------------------------------------------------------
def test_a_cut_hinge_is_not_damped_and_acts_again_when_restored():
    from drake_amd import TEAR_CUTS_HINGES
    X, T, rest = sb.mesh("book")
    H = sb.hinges(T)
    g = hs.engine([(X, T)])
    g.set_tear_coupling(TEAR_CUTS_HINGES)
    g.set_shell_bending([sb.K], rest)
    g.set_shell_damping([sd.BETA])
    ids, kc, psibar = g.shell_hinges()
    bkc = _bkc(sd.BETA, sb.K, sb.cbar64(rest.astype(np.float64), H))
    x0 = sb.state("book", "perturbed")
    faces = g.mesh_hinge_faces(T, len(X))
    torn = np.zeros(len(T), np.uint8)
    torn[[3, 10]] = 1
    cut = torn[faces].any(axis=1)
    assert cut.any() and not cut.all()
    for seed, scale in ((1, 1.0), (2, 1e3)):
        v0 = (scale * np.random.default_rng(seed).normal(size=x0.shape)).astype(F)
        hs.upload(g, x0, v0)
        whole = g.shell_damping_forces()
        g.set_torn_faces(torn)
        assert np.array_equal(g.shell_cut_hinges()[0], cut)
        rec = sd.hinges32(x0, v0, H, kc, psibar, bkc, elastic=False)[0]
        rec[cut] = 0.0                                       # (a cut hinge's four records are exact zeros)
        fd = g.shell_damping_forces()
        assert np.array_equal(hs.bits(fd), hs.bits(sb.gather32(rec, H, len(x0)))) and not np.array_equal(hs.bits(fd), hs.bits(whole))
        power, pd = g.shell_damping_state()
        assert not pd[cut].any() and pd[~cut].any()
        g.rebuild_mapping(False)
        g.calc_fem_state_and_force(min(1e-5, 0.5 * g.shell_max_stable_dt()))
        g.set_torn_faces(np.zeros(len(T), np.uint8))
        assert np.array_equal(hs.bits(g.shell_damping_forces()), hs.bits(whole))
    assert g.stats()["error_flags"] == 0
    g.destroy()


# ---- 8 -------------------------------------------------------------------------------------------------------------------
def test_off_means_off():
    """40 deterministic substeps through re-sorts: never called == called with zeros == set and cleared, to the bit, with
    the same guard and the same number of re-sort check launches"""
    cloths, rest, H, ch, x0, v0 = ss.flying()
    es = [hs.engine(cloths) for _ in range(4)]
    k = ss.scale_k(es[0], lambda k: es[0].set_shell_bending([k, k], rest), tl.DT)
    for g in es[1:]:
        g.set_shell_bending([k, k], rest)
    lim = es[0].shell_max_stable_dt()
    es[1].set_shell_damping([0.0, 0.0])
    es[2].set_shell_damping([0.5 * tl.DT, 0.25 * tl.DT])
    assert es[2].shell_max_stable_dt() < lim
    hs.upload(es[2], bd.perturbed(rest, seed=7).astype(F), v0)
    assert es[2].shell_damping_forces().any()
    es[2].set_shell_damping([])
    es[3].set_shell_damping([0.5 * tl.DT, 0.0])
    es[3].set_shell_damping([0.0, 0.0])
    for g in es:
        assert not g.get_shell_damping()["beta"].any() and len(g.get_shell_damping()) == 2
        assert hs.bits(np.array([g.shell_max_stable_dt()], F))[0] == hs.bits(np.array([lim], F))[0]
    before = es[0].stats()["rebuilds"]
    for g in es:
        hs.upload(g, x0, v0)
        assert not g.shell_damping_forces().any() and not g.shell_damping_state()[0].any()
        for _ in range(4):
            g.run_substeps(10, tl.DT, -1)
        g.gpu_sync()
        assert g.stats()["error_flags"] == 0
    assert es[0].stats()["rebuilds"] - before >= 2
    for g in es[1:]:
        hs.same_bits(hs.state(es[0]), hs.state(g), "the damper off")
        assert es[0].stats()["resort_checks"] == g.stats()["resort_checks"]
        assert np.array_equal(hs.bits(es[0].shell_state()[0]), hs.bits(g.shell_state()[0]))
    for g in es:
        g.destroy()


def test_set_get_replace_and_the_table_goes_with_the_hinge_table():
    from drake_amd import SHELL_DAMPING_DTYPE
    cloths, rest, H, ch = ss.scene()
    g = hs.engine(cloths)
    g.set_shell_bending([sb.K, sb.K], rest)
    lim = g.shell_max_stable_dt()
    x0 = bd.perturbed(rest, seed=7).astype(F)
    v0 = np.random.default_rng(4).normal(size=x0.shape).astype(F)
    hs.upload(g, x0, v0)
    g.set_shell_damping([sd.BETA, 0.0])
    f1, l1 = g.shell_damping_forces(), g.shell_max_stable_dt()
    t = np.zeros(2, SHELL_DAMPING_DTYPE)
    t["beta"] = [sd.BETA, 0.0]
    assert np.array_equal(g.get_shell_damping(), t) and l1 < lim
    n0 = len(cloths[0][0])
    assert f1[:n0].any() and not f1[n0:].any()
    g.set_shell_damping([2 * sd.BETA, sd.BETA])
    f2, l2 = g.shell_damping_forces(), g.shell_max_stable_dt()
    assert f2[n0:].any() and l2 < l1 and np.abs(f2[:n0]).max() > np.abs(f1[:n0]).max()
    g.set_shell_damping(t)
    assert np.array_equal(hs.bits(g.shell_damping_forces()), hs.bits(f1)) and g.shell_max_stable_dt() == l1
    # mpm_set_shell_bending replaces the hinge table: the damper's table goes with it
    g.set_shell_bending([sb.K, sb.K], rest)
    assert not g.get_shell_damping()["beta"].any() and g.shell_max_stable_dt() == lim and not g.shell_damping_forces().any()
    g.set_shell_damping(t)
    assert np.array_equal(hs.bits(g.shell_damping_forces()), hs.bits(f1))
    g.set_shell_bending([])
    assert not g.get_shell_damping()["beta"].any() and g.shell_max_stable_dt() == np.inf
    assert g.stats()["error_flags"] == 0
    g.destroy()


# ---- 9 -------------------------------------------------------------------------------------------------------------------
def test_the_guard_and_the_refusals():
    from drake_amd import SHELL_DAMPING_DTYPE, GpuMpm
    cloths, rest, H, ch = ss.scene()
    g0 = GpuMpm(6)
    for Xc, Tc in cloths:
        g0.add_qr_cloth(Xc, np.zeros_like(Xc), Tc)
    _refused(lambda: g0.set_shell_damping([sd.BETA, sd.BETA]), says="finalize")
    g0.destroy()

    g = hs.engine(cloths, bodies=1)
    _refused(lambda: g.set_shell_damping([sd.BETA, sd.BETA]), says="shell bending")
    _refused(lambda: g.set_shell_damping([]), says="shell bending")
    k = ss.scale_k(g, lambda k: g.set_shell_bending([k, k], rest), tl.DT, share=0.5)
    lim = g.shell_max_stable_dt()
    betas = np.array([0.5 * tl.DT, 2.0 * tl.DT], F)
    g.set_shell_damping(betas)
    good, got = g.get_shell_damping(), g.shell_max_stable_dt()
    # the value: the float64 restatement on the engine's own kc and masses, rounded down.  The engine's doubles are formed
    # in another order (1e-15), so the two floats agree or, where the bound lies that close to a float, are neighbours
    mat = GpuMpm.default_material()
    mass = np.abs(hs.vertices(g, hs.ARR().VOLUMES).reshape(-1)).astype(F) * F(mat.density)
    ids, kc, psibar = g.shell_hinges()
    rates = sd.row_rates(rest.astype(np.float64), H, kc, mass.astype(np.float64))
    n0 = len(cloths[0][0])
    beta_row = np.where(np.arange(len(rest)) < n0, float(betas[0]), float(betas[1]))
    want = sd.max_stable_dt(rates, beta_row)
    assert abs(lim - sd.max_stable_dt(rates, np.zeros(len(rest)))) <= np.spacing(F(lim))
    assert abs(got - want) <= np.spacing(F(want)) and got < lim, (got, want, lim)
    print(f"guard: elastic {lim:.6g}, damped {got:.6g}")
    # one ulp above: refused in the shell's words, nothing enqueued; at the limit: accepted
    above = float(np.nextafter(F(got), F(np.inf)))
    before = g.stats()["substeps"]
    for call in (lambda: g.run_substeps(2, above, -1), lambda: g.substep(above, -1), lambda: g.particle_to_grid(above)):
        _refused(call, says=("shell bending", "mpm_shell_max_stable_dt", "dt or the stiffness"))
    assert g.stats()["substeps"] == before
    hs.upload(g, rest, np.zeros_like(rest))
    g.run_substeps(1, got, -1)
    g.gpu_sync()
    assert g.stats()["substeps"] == before + 1 and g.stats()["error_flags"] == 0
    # refusals, one by one: the table and the guard stay
    x0 = bd.perturbed(rest, seed=7).astype(F)
    hs.upload(g, x0, np.random.default_rng(4).normal(size=x0.shape).astype(F))
    f_before = g.shell_damping_forces()
    bad_reserved = np.zeros(2, SHELL_DAMPING_DTYPE)
    bad_reserved["beta"], bad_reserved["reserved"] = sd.BETA, (0.0, 1.0)
    for call, says in ((lambda: g.set_shell_damping([sd.BETA]), "n_cloths"), (lambda: g.set_shell_damping([sd.BETA] * 3), "n_cloths"),
                       (lambda: g.set_shell_damping([sd.BETA, -1e-3]), ("cloth 1", "beta")),
                       (lambda: g.set_shell_damping([np.nan, sd.BETA]), ("cloth 0", "beta")),
                       (lambda: g.set_shell_damping([sd.BETA, np.inf]), ("cloth 1", "beta")),
                       (lambda: g.set_shell_damping(bad_reserved), ("cloth 1", "reserved"))):
        _refused(call, says=says)
        assert np.array_equal(g.get_shell_damping(), good) and g.shell_max_stable_dt() == got
        assert np.array_equal(hs.bits(g.shell_damping_forces()), hs.bits(f_before))
    assert g.lib.mpm_set_shell_damping(g.h, 2, None) == -1
    # a partitioned engine is refused through shell bending: neither call goes through there
    g.set_shell_bending([])
    g.dist_init(0, 1, [0, 64 // 4], 2, 2, 2)
    _refused(lambda: g.set_shell_damping([sd.BETA, sd.BETA]), says="partitioned")
    g.destroy()


# ---- 10 ------------------------------------------------------------------------------------------------------------------
def _total(g):
    return float(g.shell_state()[0].sum()) + float(g.measure()[1]["kinetic"])


# Stiffness-proportional damping acts on a mode in proportion to its frequency, and the guard caps beta at the highest one
# (W DT^2 + 2 G DT <= 4): the bending modes that the grid carries are damped lightly, and the engine's own dissipation (the
# transfers, the membrane's viscous term) is of the same order.  Both scenes were sampled along the run before the final
# comparison was written down; the printed traces show the ordering on the way.


def test_a_bent_sheet_loses_energy_faster_the_larger_beta():
    """a flat-rest 9 x 9 sheet released from a fold of 0.8 rad, no gravity, DT a tenth of the elastic guard (beta may then be
    up to 49 DT): after the same substeps the hinge energy plus the kinetic energy is lower with the damper than without,
    and lower still with four times the beta; the dissipated power is never negative"""
    X, T = bd.sheet(9, 9)
    x0 = sb.fold(X, 0.8).astype(F)
    es = [hs.engine([(X, T)], material=dict(gravity=0.0)) for _ in range(3)]
    k = ss.scale_k(es[0], lambda k: es[0].set_shell_bending([k]), tl.DT, share=0.1)
    traces = []
    for g, beta in zip(es, (0.0, 10 * tl.DT, 40 * tl.DT)):
        g.set_shell_bending([k])
        g.set_shell_damping([beta])
        assert tl.DT <= g.shell_max_stable_dt()
        hs.upload(g, x0)
        trace = [_total(g)]
        for _ in range(10):
            g.run_substeps(30, tl.DT, -1)
            assert g.shell_damping_state()[0][0] >= 0.0
            trace.append(_total(g))
        g.gpu_sync()
        assert g.stats()["error_flags"] == 0
        traces.append(trace)
    for beta, trace in zip(("0", "10 DT", "40 DT"), traces):
        print(f"bent sheet, beta {beta}: hinge + kinetic energy every 30 substeps: " + " ".join(f"{e:.5g}" for e in trace))
    assert traces[0][0] == traces[1][0] == traces[2][0] > 0
    assert traces[2][-1] < traces[1][-1] < traces[0][-1]
    for g in es:
        g.destroy()


SHARE = 0.5          # of the elastic guard that DT is for the tube: W DT^2 = 1, so beta may be up to 1.5 DT
STRONG = 1.4         # x DT


def test_a_struck_tube_settles_while_its_undamped_twin_rings():
    """the tube about its own curved rest shape, struck into its ovalising mode (no net momentum), no gravity: at the end
    the damped tube's hinge energy and the root mean square of its psidot are below the undamped twin's"""
    X, T = sb.tube(around=12, along=6, radius=4 * sb.H0, h=2 * sb.H0)      # (about one vertex per grid cell)
    a = np.arctan2(X[:, 2] - sb.CENTER[2], X[:, 0] - sb.CENTER[0]).astype(np.float64)
    v0 = (0.05 * np.cos(2 * a))[:, None] * np.stack([np.cos(a), np.zeros_like(a), np.sin(a)], axis=1)
    es = [hs.engine([(X, T)], material=dict(gravity=0.0, gamma=0.0)) for _ in range(2)]
    k = ss.scale_k(es[0], lambda k: es[0].set_shell_bending([k]), tl.DT, share=SHARE)
    out = []
    for g, beta in zip(es, (0.0, STRONG * tl.DT)):
        g.set_shell_bending([k])
        g.set_shell_damping([beta])
        assert tl.DT <= g.shell_max_stable_dt()
        hs.upload(g, X, v0.astype(F))
        trace = []
        for _ in range(24):
            g.run_substeps(5, tl.DT, -1)
            power, pd = g.shell_damping_state()
            assert power[0] >= 0.0
            trace.append((float(g.shell_state()[0][0]), float(np.sqrt(np.mean(pd.astype(np.float64) ** 2)))))
        g.gpu_sync()
        assert g.stats()["error_flags"] == 0
        out.append(trace)
    for beta, trace in zip(("0", "1.4 DT"), out):
        print(f"struck tube, beta {beta}: (hinge energy, rms psidot) every 5 substeps: " + " ".join(f"({e:.3g}, {p:.3g})" for e, p in trace))
    assert out[1][-1][0] < out[0][-1][0] and out[1][-1][1] < out[0][-1][1] and out[0][-1][0] > 0
    for g in es:
        g.destroy()
