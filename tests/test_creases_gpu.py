"""Creases: plastic shell hinges (mpm_set_creases, mpm_set_crease_state) on the engine; the model, the bounds and the
layout scenes are in tests/creases.py, the meshes and states in tests/shell_bending.py.

1. One substep on every mesh x state: psibar from mpm_crease_state against float64 on decided hinges and against the host
   function mpm_crease_hinge to the bit; mpm_crease_measure equals what the substep then leaves; mpm_shell_forces after
   the substep equals, to the bit, a twin's without creases whose psibar was set to the same values.
2. Layouts: strips with 63 .. 65 and 255 .. 257 hinges (a wave, a block, and one lane into the next), three cloths --
   plastic, elastic, plastic with hardening and a clamp that acts.
3. Particle order: two engines with different particle orders leave the same psibar bits.
4. Paths: every substep entry point that accepts shell bending, on tests/feature_paths.py's every-feature scene with
   creases (eta = 0.5) on its two shell cloths; all paths of a family leave bit-equal psibar and states, and the coupled
   path equals the seven calls through substeps that skipped themselves.
5. Off means off; yields zero with creases present: the state is frozen and the forces use it.
6. Set, iron and reset.
7. Dynamics: a folded sheet with a flat rest keeps its fold with creases and opens without.
8. Refusals, table by table, nothing changed afterwards."""
import numpy as np
import pytest

from tests import bending as bd
from tests import creases as cr
from tests import harness as hs
from tests import shell_bending as sb

pytestmark = pytest.mark.gpu

U, F = cr.U, np.float32
DT = 2e-4
TINY_DT = 1e-5


def _table(rows):
    from drake_amd import CREASE_DTYPE
    t = np.zeros(len(rows), CREASE_DTYPE)
    for c, (ya, eta, ma) in enumerate(rows):
        t[c] = (ya, eta, ma, 0.0)
    return t


def _fem(g, dt=TINY_DT):
    """the front of a substep: the re-sort check, then the face pass and the vertex-force chain with k_crease in it"""
    g.rebuild_mapping(False)
    g.calc_fem_state_and_force(dt)


def _scale_k(g, set_with, dt, share=0.5):
    set_with(1.0)
    lim = g.shell_max_stable_dt()
    assert np.isfinite(lim) and lim > 0
    k = float(np.float32((share * lim / dt) ** 2))
    set_with(k)
    return k


def _check_step(g, x0, H, rows, hinge_cloth, what, step):
    """the state x0 uploaded, the measure taken, `step` run, and psibar against the measure, the host function and float64
    -> (psibar before, psibar after, yields of the host function)"""
    from drake_amd import crease_hinge
    hs.upload(g, x0)
    before, _ = g.crease_state()
    psi_m, dpsi_m, next_m = g.crease_measure()
    assert np.array_equal(hs.bits(g.crease_state()[0]), hs.bits(before))          # (the measure changes no state)
    step(g)
    after, count = g.crease_state()
    assert g.stats()["error_flags"] == 0
    y, eta, P = cr.hinge_records(hinge_cloth, rows)
    psi_h, dpsi_h, next_h, yields_h = crease_hinge(np.asarray(x0, F)[H].reshape(-1, 4, 3), before, y, eta, P)
    assert np.array_equal(hs.bits(next_m), hs.bits(after)), (what, int((hs.bits(next_m) != hs.bits(after)).sum()))
    assert np.array_equal(hs.bits(after), hs.bits(next_h)), (what, int((hs.bits(after) != hs.bits(next_h)).sum()))
    assert np.array_equal(hs.bits(psi_m), hs.bits(psi_h)) and np.array_equal(hs.bits(dpsi_m), hs.bits(dpsi_h)), what
    act = sb.active(x0, H)
    ref, decided = cr.verdict64(x0, H, before, y, act)
    changed = hs.bits(after) != hs.bits(before)
    assert np.array_equal(yields_h[decided], ref[decided]), what
    assert not (changed & ~yields_h).any()
    want, bound = cr.return64(x0, H, before, y, eta, P, act)
    ok = decided & (yields_h == ref)
    err = np.abs(after.astype(np.float64) - want)
    assert np.all(err[ok] <= bound[ok]), (what, float(np.max(err[ok] / np.maximum(bound[ok], 1e-300))))
    assert (~decided).sum() <= cr.CAP * max(int(act.sum()), 1)
    print(f"creases: {what}: {int(yields_h.sum())} of {len(H)} yield, {int((~decided).sum())} undecided, creased per cloth {count.tolist()}")
    return before, after, yields_h


# ---- 1 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,st", cr.CASES)
def test_one_substep_against_float64_the_host_function_and_a_twin(name, st):
    X, T, rest = sb.mesh(name)
    H = sb.hinges(T)
    if len(H) == 0:
        g = hs.engine([(X, T)])
        with pytest.raises(Exception, match="shell bending"):
            g.set_creases(_table([(0.05, 0.0, 0.0)]))
        g.destroy()
        return
    g, twin = hs.engine([(X, T)]), hs.engine([(X, T)])
    for e in (g, twin):
        e.set_shell_bending([sb.K], rest)
    x0 = sb.state(name, st)
    # (`collinear` has a face of zero area, which the membrane model cannot step: the front of the substep alone)
    step = _fem if st == "collinear" else (lambda e: (e.substep(TINY_DT, -1), e.gpu_sync()))
    for angle, eta in zip(cr.YIELD_ANGLES, (0.0, 0.5)):
        rows = [(angle, eta, 0.0)]
        g.set_crease_state(None)
        g.set_creases(_table(rows))
        before, after, yields = _check_step(g, x0, H, rows, np.zeros(len(H), int), f"{name} {st} at {angle}", step)
        assert np.array_equal(hs.bits(before), hs.bits(g.shell_hinges()[2]))
        if st in ("rest", "rigid", "collinear"):
            assert not yields.any() and g.crease_state()[1][0] == 0
        if st == "perturbed" and len(H) > 1:
            assert yields.any() and not yields.all()
        # the twin: no yield anywhere, psibar set to the same values, the same positions -> the same forces, to the bit
        x1 = hs.vertices(g, hs.ARR().POSITIONS)
        twin.set_crease_state(after)
        hs.upload(twin, x1)
        assert np.array_equal(hs.bits(twin.crease_state()[0]), hs.bits(after))
        assert np.array_equal(hs.bits(g.shell_forces()), hs.bits(twin.shell_forces())), (name, st, angle)
        assert np.array_equal(hs.bits(g.shell_state()[1]), hs.bits(twin.shell_state()[1]))
        assert np.array_equal(g.shell_state()[0].view(np.uint64), twin.shell_state()[0].view(np.uint64))
        # (mpm_shell_hinges keeps reporting the rest values)
        assert np.array_equal(hs.bits(g.shell_hinges()[2]), hs.bits(before))
    for e in (g, twin):
        assert e.stats()["error_flags"] == 0
        e.destroy()


# ---- 2 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_faces", cr.STRIPS)
def test_strips_around_a_wave_and_a_block(n_faces):
    X, T, x = cr.strip(n_faces)
    H = sb.hinges(T)
    g = hs.engine([(X, T)])
    g.set_shell_bending([sb.K])
    assert np.array_equal(g.shell_hinges()[0], H) and len(H) == n_faces - 1
    for angle in cr.YIELD_ANGLES:
        rows = [(angle, 0.0, 0.0)]
        g.set_crease_state(None)
        g.set_creases(_table(rows))
        before, after, yields = _check_step(g, x, H, rows, np.zeros(len(H), int), f"strip of {n_faces} faces at {angle}", _fem)
        assert yields.any() and not yields.all()
        assert yields[-1] == (hs.bits(after)[-1] != hs.bits(before)[-1])      # (the last lane: alone in its wave or block)
        assert g.crease_state()[1][0] == int((hs.bits(after) != hs.bits(before)).sum())
    g.destroy()


def test_three_cloths_plastic_elastic_and_clamped():
    cloths, rows, x = cr.three_cloths()
    g = hs.engine(cloths)
    g.set_shell_bending([sb.K] * 3)
    ids, _, psibar0 = g.shell_hinges()
    first = np.cumsum([0] + [len(X) for X, _ in cloths])
    hinge_cloth = np.searchsorted(first, ids[:, 0], side="right") - 1
    assert not psibar0.any() and (np.bincount(hinge_cloth) == len(ids) // 3).all()
    g.set_creases(_table(rows))
    assert np.array_equal(g.get_creases(), _table(rows))
    before, after, yields = _check_step(g, x, ids.astype(np.int64), rows, hinge_cloth, "three cloths", _fem)
    count = g.crease_state()[1]
    assert count[0] > 0 and count[1] == 0 and count[2] > 0
    assert not (hs.bits(after) != hs.bits(before))[hinge_cloth == 1].any() and not yields[hinge_cloth == 1].any()
    P = cr.chord(1.0)
    assert np.abs(after[hinge_cloth == 0]).max() > P and np.all(np.abs(after[hinge_cloth == 2]) <= P)
    # a second pass with the folds opened to 2.2 rad (on the same positions the hinges of cloth 0 would sit exactly at their
    # yield moment, undecided by construction): cloth 0 unloads and holds, cloth 2 yields again and its fold line arrives
    # at the clamp P = 2 sin(0.5)
    x2 = cr.three_cloths(2.2)[2]
    _, after2, _ = _check_step(g, x2, ids.astype(np.int64), rows, hinge_cloth, "three cloths, opened to 2.2", _fem)
    moved = hs.bits(after2) != hs.bits(after)
    assert moved[hinge_cloth == 2].any() and not moved[hinge_cloth == 1].any()
    assert (np.abs(after2[hinge_cloth == 2]) == P).any() and np.all(np.abs(after2[hinge_cloth == 2]) <= P)      # (the clamp acts)
    g.destroy()


# ---- 3 -------------------------------------------------------------------------------------------------------------------
def test_particle_order():
    """Two engines of the 12 x 12 sheet: one in Finalize's particle order, one re-sorted while every particle had a cell to
    itself (tests/rest_shape.py: spread, one_per_cell), so ordered by those cells alone; the same bent state uploaded to
    both by original id, the vertex-force chain run without a re-sort in between: different slots, the same psibar bits,
    and the same in default (non-deterministic) mode."""
    from tests import rest_shape as rs
    A = hs.ARR()
    pos, idx = rs.sheet()
    wide = rs.spread(idx)
    assert rs.one_per_cell(wide, idx)
    H = sb.hinges(idx)
    x = pos.astype(np.float64)
    x[:, 2] += 0.25 * (0.2 / rs.SHEET_RES) * np.random.default_rng(5).uniform(-1, 1, len(x))
    x = x.astype(F)
    es = [hs.engine([(pos, idx.reshape(-1))]), hs.engine([(pos, idx.reshape(-1))]), hs.engine([(pos, idx.reshape(-1))], deterministic=False)]
    hs.upload(es[1], wide)
    es[1].rebuild_mapping(True)
    assert not np.array_equal(es[0].download(A.PIDS), es[1].download(A.PIDS)), "the two engines hold the same particle order"
    out = []
    for g in es:
        g.set_shell_bending([sb.K])
        g.set_creases(_table([(0.05, 0.5, 0.0)]))
        hs.upload(g, x)
        g.calc_fem_state_and_force(TINY_DT)
        out.append((hs.bits(g.crease_state()[0]), hs.bits(g.crease_measure()[2]), hs.bits(g.shell_forces())))
    assert not np.array_equal(es[0].download(A.PIDS), es[1].download(A.PIDS))
    yields, decided = cr.verdict64(x, H, np.zeros(len(H), F), cr.chord(0.05), sb.active(x, H))
    assert yields.any() and not yields.all() and out[0][0].any()
    for k in (1, 2):
        for a, b in zip(out[0], out[k]):
            assert np.array_equal(a, b), k
    for g in es:
        assert g.stats()["error_flags"] == 0
        g.destroy()


# ---- 4 -------------------------------------------------------------------------------------------------------------------
PATH_ROWS = [(0.0, 0.0, 0.0), (0.01, 0.5, 0.0), (0.01, 0.5, 0.0), (0.0, 0.0, 0.0)]   # the scene's shell cloths are 1 and 2
_PATHS = {}


def _path_state(g):
    from tests import feature_paths as fp
    st = fp.state(g)
    psibar, count = g.crease_state()
    st["crease_psibar"], st["crease_count"] = fp.words(psibar), fp.words(count)
    return st


def _fused(name):
    from tests import feature_paths as fp
    if name not in _PATHS:
        runner, env = fp.FUSED[name]
        g = fp.engine(env=env)
        g.set_creases(_table(PATH_ROWS))
        runner(g, -1)
        skipped = g.owed_substeps()
        _PATHS[name] = (_path_state(g), g.stats(), skipped)
        g.destroy()
    return _PATHS[name]


def _same_state(a, b, what):
    assert set(a) == set(b), (what, set(a) ^ set(b))
    for k in a:
        assert a[k].size and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (what, k, int((a[k] != b[k]).sum()))


@pytest.mark.parametrize("name", ["run_substeps_sparse_checks", "substeps", "profile_substeps", "phase_calls", "phase_calls_undeferred"])
def test_fused_paths_leave_the_same_creases(name):
    from tests import feature_paths as fp
    (sa, ta, ka), (sb_, tb, kb) = _fused("run_substeps"), _fused(name)
    for st in (ta, tb):
        assert st["error_flags"] == 0 and st["substeps"] == fp.N and st["rebuilds"] > 1, st
    if name == "run_substeps_sparse_checks":
        assert kb > 0, "no substep skipped itself with k_crease in it"
    count = sa["crease_count"].view(np.uint32)
    print(f"creases, {name}: creased per cloth {count.tolist()}, skipped and run again {kb}")
    assert count[1] > 0 and count[2] > 0 and count[0] == 0 and count[3] == 0
    _same_state(sa, sb_, name)


def test_creases_change_that_run():
    """the every-feature run with and without creases differs, so the paths above compare something"""
    from tests import feature_paths as fp
    g = fp.engine()
    sp_ = fp.FUSED["run_substeps"][0]
    sp_(g, -1)
    plain = fp.state(g)
    g.destroy()
    creased = _fused("run_substeps")[0]
    assert not np.array_equal(plain["forces_shell"], creased["forces_shell"])
    assert not np.array_equal(plain["pos"], creased["pos"])


@pytest.mark.parametrize("env", [None, {"MPM_CT_GATE_ALWAYS": "1", "MPM_CT_NO_WATCH": "1"}], ids=["", "gate_always"])
def test_coupled_equals_the_seven_calls(env):
    """run_coupled_substeps against the reference's seven calls per substep; with MPM_CT_GATE_ALWAYS every re-sort is found
    by a coupled substep that skipped itself: a k_crease that had run in the skipped substep would have moved the psibar
    of the cloths with eta = 0.5 twice"""
    from tests import feature_paths as fp
    if "seven" not in _PATHS:
        g = fp.engine()
        g.set_creases(_table(PATH_ROWS))
        fp.seven_calls(g, fp.floor(), fp.N)
        _PATHS["seven"] = (_path_state(g), g.stats())
        g.destroy()
    sa, ta = _PATHS["seven"]
    g = fp.engine(env=env)
    g.set_creases(_table(PATH_ROWS))
    fp.coupled(g, fp.floor())
    sb_, tb, cb = _path_state(g), g.stats(), g.contact_counters()
    g.destroy()
    assert ta["error_flags"] == 0 and tb["error_flags"] == 0 and ta["substeps"] == tb["substeps"] == fp.N
    assert ta["rebuilds"] >= 2 and ta["rebuilds"] == tb["rebuilds"]
    if env:
        assert cb["refused_stale"] >= 1 and cb["contact_free"] == 0, cb
    count = sa["crease_count"].view(np.uint32)
    assert count[1] > 0 and count[2] > 0
    _same_state(sa, sb_, f"coupled, {env}")


def test_sums_path_with_and_without_skipped_substeps():
    """substep_begin / substep_end, the member of the sums family that is not a halo call: the same psibar and bits with a
    re-sort check in front of every substep as with the sparse checks"""
    from tests import feature_paths as fp
    from tests import substep_paths as sp
    out = []
    for env in (None, fp.SPARSE_CHECKS):
        g = fp.engine(env=env)
        g.set_creases(_table(PATH_ROWS))
        sp._begin_end(g)
        out.append((_path_state(g), g.stats()))
        g.destroy()
    for _, st in out:
        assert st["error_flags"] == 0 and st["substeps"] == fp.N and st["rebuilds"] > 1, st
    count = out[0][0]["crease_count"].view(np.uint32)
    assert count[1] > 0 and count[2] > 0
    _same_state(out[0][0], out[1][0], "substep_begin_end")


# ---- 5 -------------------------------------------------------------------------------------------------------------------
def test_off_means_off():
    """40 deterministic substeps through re-sorts on engines with shell bending: never called == creases set and cleared
    again with no hinge creased, to the bit and with the same counters of substeps, re-sorts and re-sort checks"""
    A = hs.ARR()
    X, T = bd.sheet(12, 12)
    x0 = cr.fold_state(X, 0.3, seed=1)
    v0 = np.tile(np.array([4.0, 0.3, 0.0], F), (len(X), 1))
    es = [hs.engine([(X, T)]) for _ in range(2)]
    for g in es:
        _scale_k(g, lambda k: g.set_shell_bending([k]), DT)
    es[1].set_creases(_table([(0.05, 0.5, 0.0)]))
    assert es[1].get_creases()["yield_angle"][0] == F(0.05)
    es[1].set_creases(None)
    assert not es[1].get_creases()["yield_angle"].any() and es[1].crease_state()[1][0] == 0
    before = es[0].stats()["rebuilds"]
    for g in es:
        hs.upload(g, x0, v0)
        for _ in range(4):
            g.run_substeps(10, DT, -1)
        g.gpu_sync()
        assert g.stats()["error_flags"] == 0
    assert es[0].stats()["rebuilds"] - before >= 1
    for which in (A.POSITIONS, A.VELOCITIES, A.AFFINE, A.DEFORMATION_GRADIENTS, A.PIDS):
        assert np.array_equal(es[0].download(which).view(np.uint32), es[1].download(which).view(np.uint32)), which
    for key in ("substeps", "rebuilds", "resort_checks"):
        assert es[0].stats()[key] == es[1].stats()[key], key
    assert es[0].shell_forces().any()
    assert np.array_equal(hs.bits(es[1].crease_state()[0]), hs.bits(es[1].shell_hinges()[2]))
    for g in es:
        g.destroy()


def test_yields_zero_with_creases_present_freezes_the_state():
    X, T = bd.sheet(12, 12)
    H = sb.hinges(T)
    x = cr.fold_state(X, 0.8, seed=2)
    g, twin = hs.engine([(X, T)]), hs.engine([(X, T)])
    for e in (g, twin):
        e.set_shell_bending([sb.K])
    g.set_creases(_table([(0.05, 0.0, 0.0)]))
    hs.upload(g, x)
    _fem(g)
    creased, count = g.crease_state()
    assert count[0] > 0
    g.set_creases(None)                                   # all zeros: yielding off, the creases stay
    assert not g.get_creases()["yield_angle"].any()
    assert np.array_equal(hs.bits(g.crease_state()[0]), hs.bits(creased)) and g.crease_state()[1][0] == count[0]
    x2 = cr.fold_state(X, 1.4, seed=3)
    hs.upload(g, x2)
    _fem(g)
    assert np.array_equal(hs.bits(g.crease_state()[0]), hs.bits(creased))            # frozen
    assert np.array_equal(hs.bits(g.crease_measure()[2]), hs.bits(creased))
    twin.set_crease_state(creased)
    hs.upload(twin, x2)
    f, ft = g.shell_forces(), twin.shell_forces()
    assert np.array_equal(hs.bits(f), hs.bits(ft)) and f.any()
    # ... and they are the forces of the creased psibar, not of the rest values
    kc = g.shell_hinges()[1]
    act = sb.active(x2, H)
    B, N, _ = sb.bound(x2.astype(np.float64), H, kc, creased, act)
    assert sb.margin(f - sb.force64(x2.astype(np.float64), H, kc, creased, act), B, sb.R_SHELL + N) <= 1.0
    assert sb.margin(f - sb.force64(x2.astype(np.float64), H, kc, np.zeros(len(H)), act), B, sb.R_SHELL + N) > 1.0
    for e in (g, twin):
        assert e.stats()["error_flags"] == 0
        e.destroy()


# ---- 6 -------------------------------------------------------------------------------------------------------------------
def test_set_iron_and_reset():
    X, T, rest = sb.mesh("book")
    H = sb.hinges(T)
    g, never = hs.engine([(X, T)]), hs.engine([(X, T)])
    for e in (g, never):
        e.set_shell_bending([sb.K], rest)
    psibar0 = g.shell_hinges()[2]
    assert psibar0.any()
    r = np.random.default_rng(11)
    given = (psibar0 + 0.3 * r.uniform(-1, 1, len(H))).astype(F)
    given[::5] = psibar0[::5]
    g.set_crease_state(given)                             # allowed while every yield is 0: a pre-creased cloth
    got, count = g.crease_state()
    assert np.array_equal(hs.bits(got), hs.bits(given)) and count[0] == int((hs.bits(given) != hs.bits(psibar0)).sum()) > 0
    assert np.array_equal(hs.bits(g.shell_hinges()[2]), hs.bits(psibar0))
    x = sb.state("book", "perturbed")
    for e in (g, never):
        hs.upload(e, x)
    assert not np.array_equal(hs.bits(g.shell_forces()), hs.bits(never.shell_forces()))
    g.set_crease_state(None)                              # ironing
    got, count = g.crease_state()
    assert np.array_equal(hs.bits(got), hs.bits(psibar0)) and count[0] == 0
    assert np.array_equal(hs.bits(g.shell_forces()), hs.bits(never.shell_forces()))
    assert np.array_equal(hs.bits(g.shell_state()[1]), hs.bits(never.shell_state()[1]))
    # mpm_set_shell_bending again drops the parameters and the creases with the table they belonged to
    g.set_creases(_table([(0.05, 0.25, 0.0)]))
    g.set_crease_state(given)
    g.set_shell_bending([sb.K], rest)
    assert not g.get_creases()["yield_angle"].any() and not g.get_creases()["hardening"].any()
    got, count = g.crease_state()
    assert np.array_equal(hs.bits(got), hs.bits(psibar0)) and count[0] == 0
    assert np.array_equal(hs.bits(g.shell_forces()), hs.bits(never.shell_forces()))
    _fem(g)
    assert np.array_equal(hs.bits(g.crease_state()[0]), hs.bits(psibar0))
    # ... and shell bending off leaves nothing to crease
    g.set_shell_bending([0.0])
    assert len(g.crease_state()[0]) == 0 and g.crease_state()[1][0] == 0
    for e in (g, never):
        assert e.stats()["error_flags"] == 0
        e.destroy()


# ---- 7 -------------------------------------------------------------------------------------------------------------------
FOLD_THRESHOLD = 0.5


def test_a_folded_sheet_keeps_its_fold_with_creases_and_opens_without():
    """Zero gravity, the book (a 5 x 5 sheet) with a flat rest (MPM_SHELL_REST_FLAT), added folded by 1.0 rad about its
    middle line and at rest; dt half of mpm_shell_max_stable_dt; a plastic engine (yield_angle 0.1, eta 0) and an elastic
    twin.  After the first substep the four fold-line hinges have psibar = psi - sign y / dpsi within the bound and no
    other hinge has moved (the two halves are rigid: t of the order of 1e-6).  After 400 substeps the plastic sheet keeps
    its fold and the twin has opened: the mean |psi| of the fold-line hinges, measured on an MI355X, is 0.850483 on the
    plastic engine (its psibar 0.844945) and 0.194536 on the twin, from 0.9589 at the start; the threshold 0.5 lies between.
    Without k_crease the two engines are the same and both assertions on the plastic one fail."""
    from drake_amd import SHELL_DTYPE, SHELL_REST_FLAT
    X, T, folded = sb.mesh("book")
    H = sb.hinges(T)
    line = np.all(np.abs(X[H[:, :2], 0] - sb.CENTER[0]) < 1e-9, axis=1)
    assert line.sum() == 4
    es = [hs.engine([(folded, T)], material=dict(gravity=0.0)) for _ in range(2)]

    def flat(g):
        def set_with(k):
            t = np.zeros(1, SHELL_DTYPE)
            t["stiffness"], t["rest"] = k, SHELL_REST_FLAT
            g.set_shell_bending(t)
        return set_with
    for g in es:
        _scale_k(g, flat(g), DT)
    plastic, elastic = es
    y = cr.chord(0.1)
    plastic.set_creases(_table([(0.1, 0.0, 0.0)]))
    psi0, dpsi0, next0 = plastic.crease_measure()
    assert abs(float(np.abs(psi0[line]).mean()) - 2 * np.sin(0.5)) < 1e-4
    plastic.substep(DT, -1)
    plastic.gpu_sync()
    psibar1, count = plastic.crease_state()
    want, bound = cr.return64(folded, H, np.zeros(len(H), F), y, 0.0, 2.0, sb.active(folded, H))
    assert np.all(np.abs(psibar1.astype(np.float64) - want) <= bound)
    expect = psi0[line].astype(np.float64) - np.sign(psi0[line]) * float(y) / dpsi0[line].astype(np.float64)
    assert np.all(np.abs(psibar1[line] - expect) <= bound[line]) and np.all(np.abs(psibar1[line]) > 0.8)
    assert not psibar1[~line].any() and count[0] == 4
    t0 = cr.values64(folded, H, np.zeros(len(H), F))[2]
    # (the halves are flat up to the rounding of the folded positions to float: 2^-25 at 0.5 over heights of H0 = 2^-7, angles
    # of a few 2^-18 = 3.8e-6 -- three orders below y)
    assert t0[~line].max() < 1e-4
    elastic.substep(DT, -1)
    for g in es:
        g.run_substeps(399, DT, -1)
        g.gpu_sync()
        assert g.stats()["error_flags"] == 0
    kept = float(np.abs(plastic.shell_state()[1][line]).mean())
    opened = float(np.abs(elastic.shell_state()[1][line]).mean())
    print(f"fold: mean |psi| of the fold line after 400 substeps: plastic {kept:.6f}, elastic {opened:.6f}; "
          f"psibar {np.abs(plastic.crease_state()[0][line]).mean():.6f}")
    assert kept > FOLD_THRESHOLD > opened, (kept, opened)
    for g in es:
        g.destroy()


# ---- 8 -------------------------------------------------------------------------------------------------------------------
def _refused(call, says):
    from drake_amd import MpmError
    with pytest.raises(MpmError) as err:
        call()
    assert err.value.code == -1 and says in str(err.value), (says, str(err.value))


def test_refusals():
    from drake_amd import GpuMpm
    X, T, rest = sb.mesh("book")
    Xs, Ts, _ = sb.mesh("strip")
    Xs = (Xs.astype(np.float64) + np.array([0.0, 0.2, 0.0])).astype(F)
    # before mpm_finalize
    g0 = GpuMpm(6)
    g0.add_qr_cloth(X, np.zeros_like(X), T)
    _refused(lambda: g0.set_creases(None), says="finalize")
    _refused(lambda: g0.set_crease_state(None), says="finalize")
    g0.destroy()
    g = hs.engine([(X, T), (Xs, Ts)])
    # shell bending off
    _refused(lambda: g.set_creases(None), says="shell bending")
    _refused(lambda: g.set_crease_state(None), says="shell bending")
    assert len(g.get_creases()) == 2 and not g.get_creases()["yield_angle"].any()
    g.set_shell_bending([sb.K, sb.K], np.concatenate([rest, Xs]))
    psibar0 = g.shell_hinges()[2]
    n = len(psibar0)
    good = _table([(0.05, 0.25, 0.0), (0.3, 0.0, 2.0)])
    g.set_creases(good)
    state = (psibar0 + F(0.01)).astype(F)
    g.set_crease_state(state)

    def unchanged():
        assert np.array_equal(g.get_creases(), good)
        got, count = g.crease_state()
        assert np.array_equal(hs.bits(got), hs.bits(state)) and count.sum() == n
    unchanged()
    # a wrong count, a null array
    _refused(lambda: g.set_creases(good[:1]), says="cloth count")
    _refused(lambda: g.set_creases(np.concatenate([good, good[:1]])), says="cloth count")
    assert g.lib.mpm_set_creases(g.h, 2, None) == -1 and "null" in g.lib.mpm_last_error().decode()
    with pytest.raises(ValueError):
        g.set_crease_state(state[:-1])
    unchanged()
    # the numbers, cloth by cloth
    pi32 = float(F(np.pi))
    for c in (0, 1):
        for field, vals in (("yield_angle", (-0.1, np.nan, np.inf, pi32, 3.2)), ("hardening", (-0.1, 1.0, 1.5, np.nan, np.inf)),
                            ("max_angle", (-0.5, np.nan, np.inf, 3.2))):
            for val in vals:
                bad = good.copy()
                bad[field][c] = val
                _refused(lambda bad=bad: g.set_creases(bad), says=f"cloth {c}")
                unchanged()
    # max_angle = pi as a float is allowed: P = 2
    ok = good.copy()
    ok["max_angle"][:] = pi32
    g.set_creases(ok)
    g.set_creases(good)
    unchanged()
    # a P below a rest |psibar0| of the cloth: the book's fold-line hinges rest at 2 sin(0.5) = 0.96
    small = good.copy()
    small["max_angle"][0] = 0.5
    _refused(lambda: g.set_creases(small), says="hinge")
    unchanged()
    # mpm_set_crease_state: a non-finite value, a |psibar| above its hinge's P (cloth 1's is 2 sin(1) = 1.68)
    for val in (np.nan, np.inf, -np.inf):
        bad = state.copy()
        bad[3] = val
        _refused(lambda bad=bad: g.set_crease_state(bad), says="hinge 3")
        unchanged()
    bad = state.copy()
    bad[n - 1] = 1.7
    _refused(lambda: g.set_crease_state(bad), says=f"hinge {n - 1}")
    bad[n - 1] = -1.7
    _refused(lambda: g.set_crease_state(bad), says=f"hinge {n - 1}")
    bad = state.copy()
    bad[0] = 2.5
    _refused(lambda: g.set_crease_state(bad), says="hinge 0")
    unchanged()
    assert g.stats()["error_flags"] == 0
    # a partitioned engine refuses the calls (it cannot have shell bending: the table is cleared first)
    g.set_shell_bending([0.0, 0.0])
    g.dist_init(0, 1, [0, 64 // 4], 2, 2, 2)
    _refused(lambda: g.set_creases(None), says="partitioned")
    _refused(lambda: g.set_crease_state(None), says="partitioned")
    _refused(lambda: g.crease_measure(), says="partitioned")
    g.destroy()
