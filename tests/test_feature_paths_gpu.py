"""Every cloth feature together, on every host path that enqueues a substep, to the bit (tests/feature_paths.py).

The kernels behind k_vforce -- k_bend, k_bend_damp, k_link, k_pressure_volume / k_pressure_gauge / k_pressure, k_hinge /
k_hinge_gather, k_anchor_pose / k_anchor -- and behind k_g2p -- k_pin and its clock tail -- each have a float64 test of
their own force; here they run together, with per-cloth materials (k_fem_mat), membrane damping (k_damp) and a force field,
through re-sorts, owed substeps and substeps that skip themselves:

 1. fused family: N x substep, profile_substeps, the phase calls held back and launched call by call, and run_substeps
    with sparse re-sort checks (substeps that skip themselves and are owed) leave the bits of run_substeps in every
    particle array, the bodies' accumulators, the pressure / anchor / shell states and every force
    accessor; once more with a grid body (k_grid_bodies) writing into the accumulators.
 2. every feature acts in that run.
 3. sums family: the halo calls stay refused; one substep_begin leaves the forces of RebuildMapping + CalcFemStateAndForce;
    N x (substep_begin, substep_end) advances the bodies' clocks exactly as the fused family does.
 4. coupled: run_coupled_substeps in two calls against the reference's seven calls per substep, over a floor the lower
    sheet reaches on the way -- contact-free chunks behind the watch first, then solves.
 5. the same with every re-sort found by a coupled substep that skipped itself (MPM_CT_GATE_ALWAYS, MPM_CT_NO_WATCH): the
    direct test of gated_out in the feature kernels and of k_pin's gate on that route; once more with the grid body, so
    that k_anchor, k_pin, k_grid_bodies and k_ct_impulse all write into the accumulators.
 6. coupled with a collider nothing reaches equals run_substeps.
 7. the chain's composition: engines E_0 .. E_6 with the first k stages on; every stage is added once, in launch order,
    within one rounding of the sum; no feature perturbs another's tables; the total is the float64 sum of the stages within
    compose64's bound; every accessor passes its own module's float64 check with everything on.
 8. particle order: accessors and measure() are the same bits after re-sorts.

No tolerance here is a new number: bit equality, the per-feature modules' own bounds, and U = 2^-24 per stage."""
import functools

import numpy as np
import pytest

from tests import feature_paths as fp
from tests import harness as hs

pytestmark = pytest.mark.gpu

_CACHE = {}


_record = functools.partial(hs.record, prefix="feature paths: ")


def _result(name, features=fp.EVERYTHING, grid_bodies=False):
    key = (name, frozenset(features), grid_bodies)
    if key not in _CACHE:
        _CACHE[key] = fp.run(name, features, grid_bodies)
    return _CACHE[key]


def _same_state(a, b, what):
    assert set(a) == set(b), (what, set(a) ^ set(b))
    for k in a:
        assert a[k].size and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (what, k, int((a[k] != b[k]).sum()))


def _finite(st):
    for k in ("pos", "vel", "C", "F", "tau", "f", "forces_bending", "forces_damping", "forces_links", "forces_pressure",
              "forces_shell", "forces_anchors"):
        assert np.isfinite(fp.floats(st, k)).all(), k


# ---- 1 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid_bodies", [False, True], ids=["", "grid_bodies"])
@pytest.mark.parametrize("name", ["run_substeps_sparse_checks", "substeps", "profile_substeps", "phase_calls", "phase_calls_undeferred"])
def test_fused_family_equals_run_substeps(name, grid_bodies):
    (sa, ta, ma), (sb, tb, mb) = _result("run_substeps", grid_bodies=grid_bodies), _result(name, grid_bodies=grid_bodies)
    for st, more in ((ta, ma), (tb, mb)):
        assert st["error_flags"] == 0 and st["substeps"] == fp.N, st
        assert st["rebuilds"] > 1, st             # (above Finalize's one: re-sorts on the way)
        assert more["owed"] == 0, more
    assert ta["rebuilds"] == tb["rebuilds"], (name, ta, tb)
    print(f"{name}, grid bodies {grid_bodies}: rebuilds {ta['rebuilds']}, skipped themselves and were run again: "
          f"{ma['skipped']} of run_substeps, {mb['skipped']} of {name}; state {fp.state_hash(sa)}")
    if name == "run_substeps_sparse_checks":
        # run_substeps' own gate with the features on: substeps found the re-sort pending, skipped themselves -- every
        # feature kernel and k_pin with them -- and were run again at the first synchronisation point
        assert mb["skipped"] > 0, mb
    _same_state(sa, sb, name)
    _finite(sa)


# ---- 2 -------------------------------------------------------------------------------------------------------------------
def test_every_feature_acts_in_that_run():
    """without this, 1 could pass on a scene in which a kernel does nothing"""
    s = fp.scene()
    st, stats, more = _result("run_substeps")
    bare = _result("run_substeps", features=fp.NOTHING)[0]
    assert not np.array_equal(st["vel"], bare["vel"])
    for k in ("bending", "damping", "links", "pressure", "shell", "anchors"):
        f = fp.floats(st, "forces_" + k).reshape(-1, 3)
        assert np.abs(f).max() > 0, k
        # ... on the cloths it is set on, and an exact zero elsewhere
        on = {"bending": (0, 1), "damping": (0, 1, 2, 3), "links": (0, 1, 2, 3), "pressure": (0, 2), "shell": (1, 2),
              "anchors": (1, 2)}[k]
        for c in range(4):
            a, b = s["first"][c], s["first"][c + 1]
            assert f[a:b].any() == (c in on), (k, c)
    # the cord: slack before the first substep, taut at the end
    cord = fp.floats(st, "forces_links").reshape(-1, 3)[s["cord_vertex"]]
    assert not more["cord0"].any() and cord.any(), (more["cord0"], cord)
    # the bodies: 0 felt its pins and spring anchors, 1 its cords; 2 (the contact collider's) nothing on this path
    f = fp.floats(st, "f").reshape(3, 3)
    assert f[0].any() and f[1].any() and not f[2].any(), f
    # the gas: its gauge pressure moved with the volume; the constant one did not
    from drake_amd import PRESSURE_STATE_DTYPE
    ps = np.frombuffer(st["pressure_state"].tobytes(), PRESSURE_STATE_DTYPE)
    assert ps["gauge"][2] != more["gauge0"][2] and more["gauge0"][2] > 0 and ps["gauge"][0] == more["gauge0"][0] == np.float32(20.0)
    # each writer of the accumulators alone changes them: no pins, no anchors, and the grid body
    no_pins = fp.floats(_result("run_substeps", features=fp.EVERYTHING - {"pins"})[0], "f").reshape(3, 3)
    no_anchors = fp.floats(_result("run_substeps", features=fp.EVERYTHING - {"anchors"})[0], "f").reshape(3, 3)
    with_gb = fp.floats(_result("run_substeps", grid_bodies=True)[0], "f").reshape(3, 3)
    assert not np.array_equal(no_pins[0], f[0]) and not np.array_equal(no_anchors[0], f[0])
    assert no_pins[1].any() and not no_anchors[1].any()
    assert not np.array_equal(with_gb[1], f[1])           # (k_grid_bodies pushed body 1)


# ---- 3 -------------------------------------------------------------------------------------------------------------------
def test_sums_family_refusals_and_the_forces_of_substep_begin():
    from drake_amd import GpuMpm, MpmError
    A = hs.ARR()
    x0, v0 = fp.perturbed_state()
    g, twin = fp.engine(), fp.engine()
    zones, bufs = GpuMpm.halo_zone_args([], []), GpuMpm.halo_buffer_args([])
    with pytest.raises(MpmError, match="halo substeps: not available"):
        g.substep_begin_halo(fp.DT, zones, 0)
    with pytest.raises(MpmError, match="halo substeps: not available"):
        g.substep_mid_halo(fp.DT, -1)
    with pytest.raises(MpmError, match="halo substeps: not available"):
        g.substep_end_halo(fp.DT, -1, bufs, 0)
    assert g.stats()["substeps"] == 0
    fp.upload(g, x0, v0)
    fp.upload(twin, x0, v0)
    g.substep_begin(fp.DT)
    twin.rebuild_mapping(False)
    twin.calc_fem_state_and_force(fp.DT)
    fa, fb = fp.vertices(g, A.FORCES), fp.vertices(twin, A.FORCES)
    assert fa.any() and np.array_equal(fp.words(fa), fp.words(fb)), int((fp.words(fa) != fp.words(fb)).sum())
    for (k, a), b in zip(fp.accessors(g).items(), fp.accessors(twin).values()):
        assert a.any() and np.array_equal(fp.words(a), fp.words(b)), k
    for e in (g, twin):
        assert e.stats()["error_flags"] == 0
        e.destroy()


def test_sums_family_runs_and_advances_the_clocks_once_per_substep():
    """(the two families' particle states are not compared: gather + update from sums is another order of arithmetic)"""
    from tests import substep_paths as sp
    fused = _result("run_substeps")[0]
    g = fp.engine()
    sp._begin_end(g)
    st = fp.state(g)
    stats = g.stats()
    g.destroy()
    assert stats["error_flags"] == 0 and stats["substeps"] == fp.N and stats["rebuilds"] > 1, stats
    # the attachment points are the bodies' poses at their clocks: one advance per substep on either family
    assert np.array_equal(st["anchor_point"], fused["anchor_point"])
    _finite(st)
    assert fp.floats(st, "f").reshape(3, 3)[:2].any(axis=1).all()


# ---- 4, 5 ----------------------------------------------------------------------------------------------------------------
def _rows(rs, *keys):
    return np.array([[float(r[k]) for k in keys] for r in rs])


def _same_rows(ra, rb, *keys):
    """tests/test_contact_noroundtrip_gpu._same_rows (NaN residuals -- no DoF -- compare equal)"""
    a, b = _rows(ra, *keys), _rows(rb, *keys)
    assert a.shape == b.shape, (a.shape, b.shape)
    bad = np.nonzero(~np.all((a == b) | (np.isnan(a) & np.isnan(b)), axis=1))[0]
    assert bad.size == 0, (keys, [(int(i), a[i].tolist(), b[i].tolist()) for i in bad[:6]])


def _seven(grid_bodies):
    key = ("seven calls", grid_bodies)
    if key not in _CACHE:
        g = fp.engine(grid_bodies=grid_bodies)
        rows = fp.seven_calls(g, fp.floor(), fp.N, fp.bc_of(grid_bodies))
        _CACHE[key] = (fp.state(g), g.stats(), rows)
        g.destroy()
    return _CACHE[key]


def _coupled(env, grid_bodies):
    g = fp.engine(env=env, grid_bodies=grid_bodies)
    rows = fp.coupled(g, fp.floor(), fp.bc_of(grid_bodies))
    out = fp.state(g), g.stats(), rows, g.contact_counters()
    g.destroy()
    return out


def _check_coupled(a, b, what):
    (sa, ta, ra), (sb, tb, rb, cb) = a, b
    assert ta["error_flags"] == 0 and tb["error_flags"] == 0, (ta, tb)
    assert ta["substeps"] == fp.N and tb["substeps"] == fp.N
    assert ta["rebuilds"] >= 2 and ta["rebuilds"] == tb["rebuilds"], (ta["rebuilds"], tb["rebuilds"])
    contacts = [r["contacts"] for r in ra]
    first = next((i for i, c in enumerate(contacts) if c > 0), None)
    print(f"coupled, {what}: rebuilds {ta['rebuilds']}, first contact in substep {first}, most contacts {max(contacts)}, counters {cb}")
    assert max(contacts) > 0 and min(contacts) == 0, contacts
    _same_rows(ra, rb, "iterations", "contacts", "residual")
    _same_state(sa, sb, what)
    _finite(sa)
    f = fp.floats(sa, "f").reshape(3, 3)
    assert f[0].any() and f[1].any() and f[2, 2] < 0, f      # (pins + anchors, cords, the floor pushed down)
    return cb


def test_coupled_equals_the_seven_calls():
    cb = _check_coupled(_seven(False), _coupled(None, False), "everything on")
    assert cb["contact_free"] > 0, cb             # (watch-gated chunks ran with the features on)


@pytest.mark.parametrize("grid_bodies", [False, True], ids=["", "grid_bodies"])
def test_coupled_with_every_resort_found_by_a_substep_that_skipped_itself(grid_bodies):
    """CT_DONE_GATED with the features on: the skipped substep's k_bend .. k_anchor, k_damp and k_pin must all have
    returned at once -- an anchor reaction, a pin impulse, a clock tick or a gas state applied twice would show in the
    accumulators, the attachment points or the pressure state.  With the grid body all four writers of the accumulators
    (k_anchor, k_pin, k_grid_bodies, k_ct_impulse) are active in one substep."""
    env = {"MPM_CT_GATE_ALWAYS": "1", "MPM_CT_NO_WATCH": "1"}
    a = _seven(grid_bodies)
    cb = _check_coupled(a, _coupled(env, grid_bodies), f"gate always, grid bodies {grid_bodies}")
    assert cb["refused_stale"] >= 1 and cb["contact_free"] == 0, cb
    if grid_bodies:
        plain = fp.floats(_seven(False)[0], "f").reshape(3, 3)
        assert not np.array_equal(plain[1], fp.floats(a[0], "f").reshape(3, 3)[1])     # (the grid body pushed body 1)


# ---- 6 -------------------------------------------------------------------------------------------------------------------
def test_coupled_without_contact_equals_run_substeps():
    """coupled_substep / coupled_chunk enqueue the substep through the same two functions as mpm_run_substeps, with their
    own gates and re-sort checks: with a collider nothing reaches, the same bits as run_substeps in its uneven batches"""
    sa, ta, _ = _result("run_substeps")
    g = fp.engine()
    rows = g.run_coupled_substeps(fp.N, fp.DT, fp.far_collider(), fp.MU, fp.K_CT, fp.D_CT)
    sb, tb, cb = fp.state(g), g.stats(), g.contact_counters()
    g.destroy()
    assert all(r["contacts"] == 0 and r["iterations"] == 0 for r in rows)
    assert tb["error_flags"] == 0 and tb["substeps"] == fp.N and tb["rebuilds"] == ta["rebuilds"] > 1, (ta, tb)
    assert cb["contact_free"] > 0, cb
    _same_state(sa, sb, "coupled, nothing in reach")


# ---- 7 -------------------------------------------------------------------------------------------------------------------
def _forces_of(features, x0, v0, F0, clock=False):
    """a fresh engine with `features`, the state uploaded, one RebuildMapping + CalcFemStateAndForce -> (engine, FORCES)"""
    g = fp.engine(features, clock=clock)
    fp.upload(g, x0, v0, F0)
    g.rebuild_mapping(False)
    g.calc_fem_state_and_force(fp.DT)
    return g, fp.vertices(g, hs.ARR().FORCES)


def _composition():
    if "composition" in _CACHE:
        return _CACHE["composition"]
    A = hs.ARR()
    x0, v0 = fp.perturbed_state()
    probe = fp.engine(fp.NOTHING)
    F0 = probe.download(A.DEFORMATION_GRADIENTS)       # (Finalize's F: the clock substeps of an engine with anchors move it)
    probe.destroy()
    totals, engines = [], []
    for k in range(len(fp.CHAIN) + 1):
        g, f = _forces_of(fp.chain_features(k), x0, v0, F0, clock="anchors" in fp.chain_features(k))
        totals.append(f)
        engines.append(g)
    for g in engines[:-1]:
        assert g.stats()["error_flags"] == 0
        g.destroy()
    full = engines[-1]
    acc = fp.accessors(full)
    more = dict(pressure_state=full.pressure_state(), shell_hinges=full.shell_hinges(), shell_state=full.shell_state(),
                anchor_state=full.anchor_state(), x=fp.vertices(full, A.POSITIONS), v=fp.vertices(full, A.VELOCITIES))
    assert full.stats()["error_flags"] == 0
    full.destroy()
    # the hinge damping's own force: an engine with bending and hinge damping alone (mpm_damping_forces adds the membrane's;
    # the materials stay on in every solo engine: the guards are those of the scene's masses)
    solo = fp.engine({"materials", "bending", "bend_damping"})
    fp.upload(solo, x0, v0, F0)
    bend_damp = solo.damping_forces()
    solo.destroy()
    stages = [totals[0], acc["bending"], bend_damp, acc["links"], acc["pressure"], acc["shell"], acc["anchors"]]
    _CACHE["composition"] = dict(x0=x0, v0=v0, F0=F0, totals=totals, acc=acc, stages=stages, **more)
    return _CACHE["composition"]


def test_every_stage_is_added_once_and_in_order():
    """(a) FORCES(E_k) = FORCES(E_k-1) + stage k within one rounding of the sum, at every position of the chain;
    (c) FORCES(E_6), everything on, against the float64 sum of all stages within compose64's bound"""
    c = _composition()
    names = ("fem + vforce",) + fp.CHAIN
    for k in range(1, len(names)):
        assert c["stages"][k].any() and c["totals"][k].any(), names[k]
        w = fp.sum_margin(c["totals"][k], c["totals"][k - 1], c["stages"][k])
        print(f"total forces with {names[k]} on top: {w:.3g} of one rounding of the sum")
        _record(f"total forces + {names[k]}", w)
        assert w <= 1.0, (names[k], w)
        assert not np.array_equal(c["totals"][k], c["totals"][k - 1]), names[k]
    w = fp.compose_margin(c["totals"][-1], c["stages"])
    print(f"total forces, everything on, against the float64 sum of the stages: {w:.3g} of the bound")
    _record("total forces, composition", w)
    assert w <= 1.0, w
    # (the check can fail: a stage left out or added twice is far outside the bound)
    for k in range(1, len(names)):
        assert fp.compose_margin(c["totals"][-1], c["stages"][:k] + c["stages"][k + 1:]) > 1.0, names[k]
        assert fp.compose_margin(c["totals"][-1], c["stages"][:k + 1] + c["stages"][k:]) > 1.0, names[k]


SOLO = {"bending": {"bending"}, "damping": {"damping", "bending", "bend_damping"}, "links": {"links"}, "pressure": {"pressure"},
        "shell": {"shell"}, "anchors": {"anchors"}}


@pytest.mark.parametrize("feature", list(SOLO))
def test_no_feature_perturbs_anothers_tables(feature):
    """(b) each accessor with everything on is, bit for bit, that of an engine with only that feature on (the damping
    with the bending table its hinge rows read; every engine with the scene's materials, which the damping's face pass reads
    and which set the masses behind the guards) at the same state and clocks"""
    c = _composition()
    g = fp.engine(SOLO[feature] | {"materials"}, clock=feature == "anchors")
    fp.upload(g, c["x0"], c["v0"], c["F0"])
    f = fp.accessors(g)[feature]
    assert f.any() and np.array_equal(fp.words(f), fp.words(c["acc"][feature])), int((fp.words(f) != fp.words(c["acc"][feature])).sum())
    if feature == "pressure":
        assert g.pressure_state().tobytes() == c["pressure_state"].tobytes()
    if feature == "shell":
        a, b = g.shell_state(), c["shell_state"]
        assert np.array_equal(fp.words(a[0]), fp.words(b[0])) and np.array_equal(fp.words(a[1]), fp.words(b[1])) and a[2] == b[2]
    if feature == "anchors":
        a, b = g.anchor_state(), c["anchor_state"]
        assert a["energy"] == b["energy"] and np.array_equal(a["length"], b["length"]) and np.array_equal(a["point"], b["point"])
    if feature == "damping":
        # mpm_damping_forces is the membrane's force plus the hinge rows', one float addition: the stage used above is its part
        g.set_damping(np.stack([fp.params()["betas"][:, 0], np.zeros(4, np.float32)], axis=1))
        membrane = g.damping_forces()
        assert np.array_equal(fp.words(membrane + c["stages"][2]), fp.words(f))
    assert g.stats()["error_flags"] == 0
    g.destroy()


def _margin_of(err, tol):
    err = np.abs(np.asarray(err, np.float64))
    return float(np.where(err == 0, 0.0, err / np.maximum(tol, 1e-300)).max())


def test_every_accessor_passes_its_own_float64_check_with_everything_on():
    """(d) the float64 restatements and bounds of tests/bending.py, damping.py, links.py, pressure.py, shell_bending.py and
    anchors.py, as their own GPU tests call them, on the accessors of the engine with everything on"""
    from tests import anchors as an
    from tests import bending as bd
    from tests import damping as dp
    from tests import links as lk
    from tests import pressure as pr
    from tests import shell_bending as sb
    A = hs.ARR()
    c, s, p = _composition(), fp.scene(), fp.params()
    x0, v0, acc = c["x0"], c["v0"], c["acc"]
    first, nv = s["first"], len(x0)
    assert np.array_equal(c["x"], x0) and np.array_equal(c["v"], v0)
    out = {}
    # bending (tests/test_bending_gpu._check_forces), cloth by cloth; the hinge rows of the damping with it
    single = fp.engine(fp.NOTHING, materials=False)      # (rest records: those of a single-material engine, test_damping_gpu._rest)
    nf = single.n_faces
    pids, vol = single.download(A.PIDS), single.download(A.VOLUMES)
    vf = np.zeros(nf, np.float32)
    vf[pids[pids < nf]] = vol[pids < nf]
    rest = (single.download(A.DM_INVERSES).reshape(nf, 4)[:, [0, 1, 3]].copy(), vf)
    single.destroy()
    lame = []
    for cl in range(4):
        m = fp.cloth_material(cl)
        E, nu, one, two = (np.float32(a) for a in (m.youngs_modulus, m.poisson_ratio, 1.0, 2.0))
        lame.append((E / (two * (one + nu)), E * nu / ((one + nu) * (one - two * nu))))      # (test_damping_gpu._lame32)
    mu = np.array([lame[q][0] for q in s["cf"]], np.float32)
    lam = np.array([lame[q][1] for q in s["cf"]], np.float32)
    beta = np.array([p["betas"][q][0] for q in s["cf"]], np.float32)
    fd, Bm = dp.forces64(s["X"], s["T"], x0, v0, (mu, lam), beta, rest=rest)
    tol_d = dp.U * dp.rounding_count() * Bm
    out["bending"] = 0.0
    for cl in (0, 1):
        a, b = first[cl], first[cl + 1]
        X, _, T = s["cloths"][cl]
        H = bd.hinges(X, T)
        P = bd.q_dense(len(X), H)[1]
        k = float(np.float32(p["k_bend"][cl]))
        w = bd.margin(acc["bending"][a:b] - bd.force64(k, H, x0[a:b]), bd.bound(k, H, x0[a:b]), bd.rounding_count(P))
        out["bending"] = max(out["bending"], w)
        kb = float(np.float32(p["betas"][cl][1])) * k       # (test_damping_gpu._reference)
        fd[a:b] += bd.force64(kb, H, v0[a:b])
        tol_d[a:b] += (dp.U * (bd.rounding_count(P) + 2.0) * bd.bound(kb, H, v0[a:b]))[:, None]
    assert not acc["bending"][first[2]:].any()
    out["damping"] = _margin_of(acc["damping"] - fd, tol_d)
    # links (tests/test_links_gpu._check_forces)
    ref, bound, _ = lk.vertex_forces64(p["links"], x0, v0, nv)
    out["links"] = lk.margin(acc["links"] - ref, bound)
    # pressure (tests/test_pressure_gpu._check_state, _check_forces): the volumes, the gauges, the forces on the engine's gauges
    ps = c["pressure_state"]
    for cl, (V, gq, capped, _) in enumerate(pr.cloth_states(s["pressure"], x0, s["T"], s["cf"])):
        wv = abs(float(ps["volume"][cl]) - V) / pr.volume_bound(x0, s["T"][s["cf"] == cl])
        out["pressure volume"] = max(out.get("pressure volume", 0.0), wv)
        assert abs(float(ps["gauge"][cl]) - float(gq)) <= pr.U * abs(float(gq)) * (1 + 2.0 ** -20), (cl, ps["gauge"][cl], gq)
        assert bool(ps["capped"][cl]) == capped
    ref, bound, _ = pr.vertex_forces64(s["pressure"], x0, s["T"], s["cv"], s["cf"], g_of_cloth=ps["gauge"])
    out["pressure"] = pr.margin(acc["pressure"] - ref, bound)
    assert not acc["pressure"][(s["pressure"]["mode"] == pr.OFF)[s["cv"]]].any()
    # shell bending (tests/test_shell_bending_gpu._check): the engine's own kc and psibar, the hinges of the restatement
    ids, kc, psibar = c["shell_hinges"]
    H = np.concatenate([sb.hinges(s["cloths"][cl][2]) + first[cl] for cl in range(4) if p["k_shell"][cl] > 0])
    assert np.array_equal(ids, H)                        # (the hinges of the cloths with k > 0, in cloth order)
    on = sb.active(x0, H)
    x = x0.astype(np.float64)
    B, Nn, pb = sb.bound(x, H, kc, psibar, on)
    out["shell"] = sb.margin(acc["shell"] - sb.force64(x, H, kc, psibar, on), B, sb.R_SHELL + Nn)
    _, psi, inactive = c["shell_state"]
    out["shell psi"] = sb.margin(psi - sb.hinge_forces64(x, H, kc, psibar, on)[1], pb, sb.R_PSI)
    assert inactive == int((~on).sum())
    # anchors (tests/test_anchors_gpu.test_forces_against_float64): the bodies' clocks at CLOCK
    ref, bound, y32, _ = an.vertex_forces64(p["anchors"], x0, v0, s["motions"], fp.CLOCK)
    out["anchors"] = lk.margin(acc["anchors"] - ref, bound)
    y64 = an.points(p["anchors"], s["motions"], fp.CLOCK)[0]
    point = c["anchor_state"]["point"].astype(np.float64)
    out["anchor points"] = float((np.abs(point - y64) / np.spacing(np.abs(y64).astype(np.float32)).astype(np.float64)).max())
    moved = np.abs(y64 - an.points(p["anchors"], s["motions"], 0.0)[0]).max()
    assert moved > 50 * np.spacing(np.float32(0.7))        # (the clocks are not at zero: the check would see it)
    for k, w in out.items():
        print(f"{k}, everything on: {w:.3g} of its module's bound")
        _record(f"{k}, everything on", w)
    assert all(w <= 1.0 for w in out.values()), out
    assert all(acc[k].any() for k in acc)


# ---- 8 -------------------------------------------------------------------------------------------------------------------
def test_particle_order():
    """the state with everything on, uploaded in two particle orders -- as finalised, and after substeps five cells further
    along x, their re-sorts and RebuildMapping(sort = 1): the accessors, the feature states and measure() are the same bits"""
    A = hs.ARR()
    s = fp.scene()
    c = _composition()
    x0, v0, F0 = c["x0"], c["v0"], c["F0"]
    g = fp.engine(fp.EVERYTHING - {"pins", "fields"})
    out = []
    for k in range(2):
        if k:
            before = g.stats()["rebuilds"]
            fp.upload(g, x0 + np.array([5.0 / 64, 0, 0], np.float32), v0, F0)
            g.run_substeps(3, fp.DT, -1)
            g.gpu_sync()
            assert g.stats()["rebuilds"] > before and g.stats()["error_flags"] == 0, g.stats()
            g.rebuild_mapping(True)
            g.reallocate_external_bodies(3)
            g.set_body_motions(fp._motions(s["motions"]))       # (the clocks at zero again)
        fp.upload(g, x0, v0, F0)
        pids = g.download(A.PIDS)
        rows, total = g.measure()
        a = g.anchor_state()
        E, psi, inactive = g.shell_state()
        got = dict(fp.accessors(g), measure=np.frombuffer(rows.tobytes() + total.tobytes(), np.uint8), pressure_state=g.pressure_state(),
                   anchor_length=a["length"], anchor_point=a["point"], anchor_energy=np.array([a["energy"]]), shell_energy=E,
                   shell_psi=psi, shell_inactive=np.array([inactive]))
        out.append((pids, got))
    assert not np.array_equal(out[0][0], out[1][0])
    for k in out[0][1]:
        a, b = out[0][1][k], out[1][1][k]
        assert a.size and np.array_equal(fp.words(a), fp.words(b)), k
    assert all(out[0][1][k].any() for k in ("bending", "damping", "links", "pressure", "shell", "anchors"))
    assert g.stats()["error_flags"] == 0
    g.destroy()

