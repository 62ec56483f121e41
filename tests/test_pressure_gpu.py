"""Enclosed-volume pressure per cloth (mpm_set_pressure) on the engine.

1. mpm_pressure_forces per vertex against the float64 restatement of tests/pressure.py on every scene x state, within
   R_i 2^-24 |g| / 6 sum |d_b| |d_c| (R_i = 7 + n_i, counted in mpm_pressure.h).  The same after substeps that forced a
   re-sort and after mpm_rebuild_mapping(sort = 1); on the same state, uploaded again, forces, V and g are the bits of
   the first evaluation.
2. mpm_pressure_state: the volume of every cloth against float64 within the counted bound of the double sum, the gauge
   within one float rounding of the restatement, `capped` exactly on the collapsed state and with a low p_max.
3. MPM_ARR_FORCES of an engine with pressure minus a twin's without is mpm_pressure_forces, within one rounding of the sum.
4. Scheduling: run_substeps(n), the five phase calls and run_coupled_substeps with a collider nobody touches are
   bit-equal through re-sorts.
5. Off means off, to the bit and to the launch count of the re-sort checks.
6. Refusals, the old table staying in force.
7. Dynamics: an icosphere without gravity inflates under a constant and under a gas pressure; the twin keeps its volume."""
import math

import numpy as np
import pytest

from tests import harness as hs
from tests import pressure as pr
from tests import transfer_layouts as tl

pytestmark = pytest.mark.gpu

U = pr.U
CASES = [(s, st) for s in pr.SCENES for st in pr.STATES]


def _check_state(g, table, T, cf, what):
    """mpm_pressure_state against the restatement on the engine's own positions; returns the records"""
    x = hs.vertices(g, hs.ARR().POSITIONS)
    got = g.pressure_state()
    want = pr.cloth_states(table, x, T, cf)
    assert len(got) == len(want)
    for c, (V, gq, capped, E) in enumerate(want):
        Tc = T[cf == c]
        wv = abs(float(got["volume"][c]) - V) / pr.volume_bound(x, Tc)
        print(f"pressure state: {what}: cloth {c}: V = {got['volume'][c]:.9e} ({wv:.3g} of the bound), g = {got['gauge'][c]:.7g}, "
              f"capped = {got['capped'][c]}")
        hs.record(f"pressure volume: {what} cloth {c}", wv)
        assert wv <= 1.0, (what, c, got["volume"][c], V)
        # the gauge: the restatement's V differs from the engine's within the bound above, far below a float rounding
        assert abs(float(got["gauge"][c]) - float(gq)) <= U * abs(float(gq)) * (1 + 2.0 ** -20), (what, c, got["gauge"][c], gq)
        assert bool(got["capped"][c]) == capped, (what, c)
        tol = 1e-12 * (abs(E) + 1e-300) + (abs(float(table["pv"][c]) / V) + float(table["p_ambient"][c]) + abs(float(table["p"][c]))) * \
            2 * pr.volume_bound(x, Tc) if V != 0 else 0.0
        assert abs(float(got["energy"][c]) - E) <= tol, (what, c, got["energy"][c], E)
        if int(table["mode"][c]) == pr.OFF:
            assert got["gauge"][c] == 0 and got["energy"][c] == 0 and got["capped"][c] == 0
    return got


def _check_forces(g, scene, what):
    cloths, table, X, T, cv, cf = scene
    x = hs.vertices(g, hs.ARR().POSITIONS)
    f = g.pressure_forces()
    st = g.pressure_state()
    # (the engine's own gauge pressures, checked against the restatement in _check_state: the force bound is the row's)
    ref, bound, _ = pr.vertex_forces64(table, x, T, cv, cf, g_of_cloth=st["gauge"])
    w = pr.margin(f - ref, bound)
    print(f"pressure forces: {what}: {w:.3g} of the bound")
    hs.record(f"pressure forces: {what}", w)
    assert w <= 1.0, (what, w)
    off = (table["mode"] == pr.OFF)[cv]
    assert not f[off].any() and np.isfinite(f).all()
    return x, f, st


# ---- 1, 2 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,st", CASES)
def test_forces_and_state_against_float64(name, st):
    scene = pr.scene(name)
    cloths, table, X, T, cv, cf = scene
    g = hs.engine(cloths)
    g.set_pressure(table)
    assert np.array_equal(g.get_pressure(), table)
    x0 = pr.state(st, X, cv)
    hs.upload(g, x0)
    _check_state(g, table, T, cf, f"{name} {st}")
    x, f0, s0 = _check_forces(g, scene, f"{name} {st}")
    assert np.array_equal(x, x0) and f0.any()
    gas = table["mode"] == pr.GAS
    assert np.array_equal(s0["capped"][gas] != 0, np.full(gas.sum(), st == "collapsed"))
    # substeps that force a re-sort: the state five cells further along x, two short substeps
    before = g.stats()["rebuilds"]
    hs.upload(g, x0 + np.array([5.0 / 64, 0.0, 0.0], np.float32))
    g.run_substeps(2, 1e-5, -1)
    g.gpu_sync()
    assert g.stats()["error_flags"] == 0 and g.stats()["rebuilds"] > before, g.stats()
    _check_forces(g, scene, f"{name} {st} after a re-sort")
    # the first state again, in the new particle order: the same bits
    for sort in (False, True):
        if sort:
            g.rebuild_mapping(True)
        hs.upload(g, x0)
        f1, s1 = g.pressure_forces(), g.pressure_state()
        assert np.array_equal(hs.bits(f1), hs.bits(f0)), (sort, float(np.abs(f1 - f0).max()))
        assert np.array_equal(hs.bits(s1["volume"]), hs.bits(s0["volume"])) and np.array_equal(hs.bits(s1["gauge"]), hs.bits(s0["gauge"]))
        assert np.array_equal(s1["capped"], s0["capped"]) and np.array_equal(hs.bits(s1["energy"]), hs.bits(s0["energy"]))
    assert g.stats()["error_flags"] == 0
    g.destroy()


def test_low_p_max_caps_and_an_engine_that_never_set_reports_volumes():
    scene = pr.scene("mixed")
    cloths, table, X, T, cv, cf = scene
    g = hs.engine(cloths)
    # never set: volumes alone
    got = _check_state(g, pr.make_table([(pr.OFF, 0, 0, 0, 0)] * 4), T, cf, "never set")
    assert (got["volume"][[0, 2, 3]] > 0).all() and not g.get_pressure()["mode"].any() and not g.pressure_forces().any()
    low = table.copy()
    low["p_max"][0] = 120.0                                          # below the rest state's 150
    g.set_pressure(low)
    got = _check_state(g, low, T, cf, "low p_max")
    assert got["capped"][0] == 1 and got["gauge"][0] == np.float32(20.0) and got["energy"][0] == 0.0
    _check_forces(g, (cloths, low, X, T, cv, cf), "low p_max")
    g.set_pressure(table)
    got = _check_state(g, table, T, cf, "p_max restored")
    assert got["capped"][0] == 0 and abs(got["gauge"][0] - 50.0) < 1e-3
    assert g.stats()["error_flags"] == 0
    g.destroy()


# ---- 3 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "gas_bipyramid"])
def test_total_forces_include_pressure(name):
    A = hs.ARR()
    cloths, table, X, T, cv, cf = pr.scene(name)
    a, b = hs.engine(cloths), hs.engine(cloths)
    a.set_pressure(table)
    x0 = pr.state("random", X, cv)
    out = []
    for g in (a, b):
        hs.upload(g, x0)
        g.rebuild_mapping(False)
        g.calc_fem_state_and_force(1e-5)
        out.append(hs.vertices(g, A.FORCES))
    fp = a.pressure_forces()
    assert fp.any() and out[1].any()
    tot = out[1].astype(np.float64) + fp.astype(np.float64)
    err = np.abs(out[0].astype(np.float64) - tot)
    w = float((err / np.maximum(U * np.abs(out[0]).astype(np.float64), 1e-300))[err > 0].max()) if (err > 0).any() else 0.0
    print(f"total forces: {name}: {w:.3g} of one rounding of the sum")
    hs.record(f"pressure: total forces {name}", w)
    assert w <= 1.0, w
    assert not b.pressure_forces().any()
    for g in (a, b):
        assert g.stats()["error_flags"] == 0
        g.destroy()


# ---- 4, 5 ------------------------------------------------------------------------------------------------------------
def _flying(name, seed=3):
    """the scene at rest, flying along x and y fast enough for several re-sorts in a few dozen substeps of tl.DT"""
    scene = pr.scene(name)
    x0 = scene[2].copy()
    v0 = np.array([4.0, 0.3, 0.0], np.float32) + 0.05 * np.random.default_rng(seed).normal(size=x0.shape).astype(np.float32)
    return scene, x0, v0


def test_scheduling_through_resorts():
    """the mixed scene flies through several re-sorts, deterministic: run_substeps(n), n x the five phase calls and
    run_coupled_substeps(n) with a collider nobody touches give the same bits in x, v, C and F -- a force added twice
    under the gate, or a gauge pressure left from another substep, would not -- and the same V and g"""
    from drake_amd import Collider
    (cloths, table, X, T, cv, cf), x0, v0 = _flying("mixed")
    n = 40
    es = [hs.engine(cloths, bodies=1) for _ in range(3)]
    for g in es:
        g.set_pressure(table)
        hs.upload(g, x0, v0)
    before = es[0].stats()["rebuilds"]
    es[0].run_substeps(n, tl.DT, -1)
    for _ in range(n):
        g = es[1]
        g.rebuild_mapping(False)
        g.calc_fem_state_and_force(tl.DT)
        g.particle_to_grid(tl.DT)
        g.update_grid(-1)
        g.grid_to_particle(tl.DT)
    far = [Collider(1, body=0, p_WB=(0.9, 0.1, 0.1), dims=(0.02, 0, 0))]
    res = es[2].run_coupled_substeps(n, tl.DT, far, 0.5, 1e5, 1e-4)
    assert max(r["contacts"] for r in res) == 0
    for g in es:
        g.gpu_sync()
        assert g.stats()["error_flags"] == 0, g.stats()
    assert es[0].stats()["rebuilds"] - before >= 2, es[0].stats()
    s = [hs.state(g) for g in es]
    hs.same_bits(s[0], s[1], "run_substeps(n) against the phase calls")
    hs.same_bits(s[0], s[2], "run_substeps(n) against the coupled path")
    ps = [g.pressure_state() for g in es]
    for q in ps[1:]:
        assert q.tobytes() == ps[0].tobytes()
    assert es[0].pressure_forces().any() and np.isfinite(s[0]["v"]).all()
    ph, _ = es[0].profile_substeps(2, tl.DT, -1)
    assert ph["vforce"] > 0.0, ph          # (k_vforce and the pressure kernels are timed under MPM_PHASE_VFORCE)
    for g in es:
        g.destroy()


def test_off_means_off():
    """40 deterministic substeps through re-sorts: never set == set and cleared, to the bit, and with the same number of
    re-sort check launches (the quiet-time hint is in use again)"""
    (cloths, table, X, T, cv, cf), x0, v0 = _flying("mixed")
    es = [hs.engine(cloths) for _ in range(2)]
    es[1].set_pressure(table)
    assert es[1].pressure_forces().any()
    es[1].set_pressure(table[:0])
    assert not es[1].get_pressure()["mode"].any() and len(es[1].get_pressure()) == 4 and not es[1].pressure_forces().any()
    before = es[0].stats()["rebuilds"]
    for g in es:
        hs.upload(g, x0, v0)
        for _ in range(4):
            g.run_substeps(10, tl.DT, -1)
        g.gpu_sync()
        assert g.stats()["error_flags"] == 0
    assert es[0].stats()["rebuilds"] - before >= 2, es[0].stats()
    hs.same_bits(hs.state(es[0]), hs.state(es[1]), "set and cleared")
    assert es[0].stats()["resort_checks"] == es[1].stats()["resort_checks"]
    for g in es:
        g.destroy()


# ---- 6 -------------------------------------------------------------------------------------------------------------
def test_refusals():
    from drake_amd import GpuMpm, MpmError

    def refused(call, says=()):
        with pytest.raises(MpmError) as e:
            call()
        assert e.value.code == -1, e.value
        for s in (says,) if isinstance(says, str) else says:
            assert s in str(e.value), e.value

    cloths, good, X, T, cv, cf = pr.scene("mixed")
    # before Finalize
    g0 = GpuMpm(6)
    for Xc, Tc in cloths:
        g0.add_qr_cloth(Xc, np.zeros_like(Xc), Tc)
    refused(lambda: g0.set_pressure(good), says="finalize")
    g0.destroy()

    g = hs.engine(cloths)
    g.set_pressure(good)
    hs.upload(g, pr.state("random", X, cv))
    f_before, s_before = g.pressure_forces(), g.pressure_state()

    def bad(c, **kw):
        t = good.copy()
        for key, val in kw.items():
            t[key][c] = val
        return t

    sheet_edge = pr.first_open_edge(cloths[1][1])
    off1 = len(cloths[0][0])
    tables = [
        (good[:3], "mpm_cloth_count"), (np.concatenate([good, good[:1]]), "mpm_cloth_count"),
        (bad(1, p=np.nan), "cloth 1"), (bad(3, p=np.inf), "cloth 3"), (bad(2, pv=np.nan), "cloth 2"),
        (bad(0, p_max=np.inf), "cloth 0"), (bad(0, p_ambient=-np.inf), "cloth 0"),
        (bad(1, mode=3), ("cloth 1", "mode")), (bad(2, mode=0x80000001), ("cloth 2", "mode")),
        (bad(0, pv=0.0), ("cloth 0", "pv > 0")), (bad(0, pv=-1.0), "cloth 0"), (bad(0, p_ambient=-1.0), "cloth 0"),
        (bad(0, p_max=good["p_ambient"][0]), ("cloth 0", "p_max")), (bad(0, p_max=50.0), "cloth 0"),
        # gas on the open sheet: the cloth and the first offending edge, in the numbering of all vertices
        (bad(1, mode=pr.GAS, pv=1.0, p_ambient=1.0, p_max=2.0),
         ("cloth 1", "not closed", f"{off1 + sheet_edge[0]} -> {off1 + sheet_edge[1]}")),
    ]
    for t, says in tables:
        refused(lambda t=t: g.set_pressure(t), says=says)
        assert np.array_equal(g.get_pressure(), good)
    assert np.array_equal(hs.bits(g.pressure_forces()), hs.bits(f_before)) and g.pressure_state().tobytes() == s_before.tobytes()
    # partitioned, halo, team and chain calls on an engine with pressure
    nb = 64 // 4
    refused(lambda: g.dist_init(0, 1, [0, nb], 2, 2, 2), says="pressure")
    refused(lambda: g.substep_mid_halo(tl.DT), says="pressure")
    refused(lambda: g.team_prepare(), says="pressure")
    refused(lambda: g.chain_substeps(1, tl.DT), says="pressure")
    g.run_substeps(2, tl.DT, -1)
    g.gpu_sync()
    assert g.stats()["error_flags"] == 0
    # pressure off lifts the refusals; a partitioned engine refuses the call
    g.set_pressure(good[:0])
    g.dist_init(0, 1, [0, nb], 2, 2, 2)
    refused(lambda: g.set_pressure(good), says="partitioned")
    assert not g.get_pressure()["mode"].any()
    g.destroy()

    # gas on a rest volume <= 0: the icosphere wound inside out
    Xi, Ti = pr.mesh("icosphere")
    h = hs.engine([(Xi, Ti[:, [0, 2, 1]].copy())])
    refused(lambda: h.set_pressure(pr.make_table([pr.gas_row("icosphere")])), says=("cloth 0", "reverse the winding"))
    h.set_pressure(pr.make_table([(pr.CONSTANT, 10.0, 0, 0, 0)]))    # (a constant pressure takes any mesh)
    assert h.pressure_state()["volume"][0] < 0
    h.destroy()


# ---- 7 -------------------------------------------------------------------------------------------------------------
def _inflate(table_of, what):
    """the icosphere without gravity beside an unpressurised twin, n substeps of dt through the phase calls; returns
    (V per substep, g per substep, the twin's volumes, momentum added, its bound, the last state record, the table)"""
    A = hs.ARR()
    X, T = pr.mesh("icosphere")
    cv, cf = np.zeros(len(X), int), np.zeros(len(T), int)
    a, b = (hs.engine([(X, T)], material=dict(gravity=0.0)) for _ in range(2))
    mass = a.download(A.MASSES).astype(np.float64).sum()
    x64 = X.astype(np.float64)
    area = 0.5 * np.linalg.norm(np.cross(x64[T[:, 1]] - x64[T[:, 0]], x64[T[:, 2]] - x64[T[:, 0]]), axis=1).sum()
    mt = a.default_material()
    period = 2 * math.pi * pr.ICO_R * math.sqrt(mt.density * (1 - mt.poisson_ratio) / (2 * mt.youngs_modulus))
    dt, n = 1e-4, 12
    assert n * dt < 0.25 * period, (n * dt, period)
    # a pressure that moves the surface by about 1 % of the radius in the run: 1/2 (p A / M) (n dt)^2 = 0.01 R
    p = np.float32(0.02 * pr.ICO_R * mass / (area * (n * dt) ** 2))
    table = table_of(p)
    a.set_pressure(table)
    print(f"{what}: breathing period about {period:.3e} s = {period / dt:.0f} substeps, run {n}; p = {p:.4g} Pa, M = {mass:.4g} kg")

    def momentum(g):
        mm, v = g.download(A.MASSES).astype(np.float64), g.download(A.VELOCITIES).astype(np.float64)
        return (mm[:, None] * v).sum(axis=0)

    Vs, gs, Vb, added, bound = [], [], [], np.zeros(3), 0.0
    s = a.pressure_state()
    Vs.append(float(s["volume"][0]))
    gs.append(float(s["gauge"][0]))
    Vb.append(float(b.pressure_state()["volume"][0]))
    for _ in range(n):
        a.rebuild_mapping(False)
        a.calc_fem_state_and_force(dt)
        p0 = momentum(a)
        _, bd, _ = pr.vertex_forces64(table, hs.vertices(a, A.POSITIONS), T, cv, cf)
        a.particle_to_grid(dt)
        a.update_grid(-1)
        a.grid_to_particle(dt)
        added += momentum(a) - p0
        bound += dt * float(bd.sum())
        b.substep(dt, -1)
        s = a.pressure_state()
        Vs.append(float(s["volume"][0]))
        gs.append(float(s["gauge"][0]))
        Vb.append(float(b.pressure_state()["volume"][0]))
    for g in (a, b):
        g.gpu_sync()
        assert g.stats()["error_flags"] == 0
        g.destroy()
    return np.array(Vs), np.array(gs), np.array(Vb), float(np.abs(added).max()), bound, s, table


def _check_inflation(Vs, Vb, mom, bound, what):
    rise = Vs[-1] - Vs[0]
    print(f"{what}: V {Vs[0]:.6e} -> {Vs[-1]:.6e} (+{rise / Vs[0]:.3%}); the twin's |dV| {np.abs(Vb - Vb[0]).max():.3e}; "
          f"momentum added {mom:.3e}, bound {bound:.3e}")
    assert (np.diff(Vs) > 0).all(), np.diff(Vs)
    hs.record(f"pressure: {what}: the twin's volume change over a tenth of the rise", float(np.abs(Vb - Vb[0]).max() / (0.1 * rise)))
    assert np.abs(Vb - Vb[0]).max() < 0.1 * rise
    hs.record(f"pressure: {what}: momentum added over the rounding bound", mom / bound)
    assert mom <= bound, (mom, bound)


def test_constant_pressure_inflates_the_icosphere():
    """Zero gravity, the icosphere of radius R = 1/32 at rest, a constant pressure p > 0, beside a twin without.
    Breathing period of a spherical membrane: omega^2 = 2 E / (rho R^2 (1 - nu)) (the thickness cancels: stiffness and
    mass both carry it), T = 2 pi R sqrt(rho (1 - nu) / (2 E)) = 8.2e-3 s with E = 4e5, nu = 0.3, rho = 2000.  The run is
    12 substeps of 1e-4 s = 1.2e-3 s, below T / 4 = 2.05e-3 s: the membrane is still on its way out, so V rises in every
    substep.  p is chosen so that the surface moves by about 1 % of R in the run.  The twin's |dV| stays below a tenth of
    the rise; the momentum the substeps add (measured from after the FEM call to after GridToParticle, as in
    tests/test_links_gpu.py) stays inside dt times the sum of the per-vertex rounding bounds of the pressure force."""
    Vs, gs, Vb, mom, bound, _, _ = _inflate(lambda p: pr.make_table([(pr.CONSTANT, p, 0, 0, 0)]), "constant")
    _check_inflation(Vs, Vb, mom, bound, "constant pressure")
    assert (gs == gs[0]).all()


def test_gas_inflates_the_icosphere_and_its_pressure_falls():
    """The same run (period estimate and substep count as above) with an isothermal gas whose gauge pressure at rest is
    the constant test's p: absolute 1.5 p_ambient, p_ambient = 2 p.  V rises and g falls in every substep, and the last
    reported g is the formula on the last reported V, to the bit."""
    X, T = pr.mesh("icosphere")
    V0 = pr.volume64(X, T)

    def table_of(p):
        return pr.make_table([(pr.GAS, 0.0, np.float32(3.0 * p * V0), 2.0 * p, 100.0 * p)])

    Vs, gs, Vb, mom, bound, last, table = _inflate(table_of, "gas")
    _check_inflation(Vs, Vb, mom, bound, "gas")
    assert (np.diff(gs) < 0).all(), np.diff(gs)
    assert last["capped"][0] == 0
    want = np.float32(float(table["pv"][0]) / float(last["volume"][0]) - float(table["p_ambient"][0]))
    assert float(table["pv"][0]) / float(last["volume"][0]) < float(table["p_max"][0])
    assert hs.bits(last["gauge"][:1])[0] == hs.bits(np.array([want], np.float32))[0], (last["gauge"][0], want)


# ---- with every other per-cloth feature --------------------------------------------------------------------------------
def _featured_engine(cloths, with_pressure, table):
    """per-cloth materials, pins off, a force field, bending, damping, links, fast math; deterministic (the twin must
    give the same bits where pressure does not act)"""
    from drake_amd import ClothMaterial, ForceField, GpuMpm, links
    mat = GpuMpm.default_material()
    g = GpuMpm(6, mat)
    g.set_deterministic(True)
    g.set_fast_math(True)
    for c, (X, T) in enumerate(cloths):
        m = ClothMaterial.of(mat)
        m.youngs_modulus *= 1.0 + 0.25 * c
        m.density *= 1.0 + 0.1 * c
        g.add_qr_cloth(X, np.zeros_like(X), T, m)
    g.finalize()
    g._tri = np.concatenate([T + o for (X, T), o in zip(cloths, np.cumsum([0] + [len(X) for X, _ in cloths[:-1]]))])
    g.set_force_fields([ForceField(u0=(0.3, 0.0, 0.5))])
    g.set_bending([2e-7] * len(cloths))
    g.set_damping([(1e-5, 1e-5)] * len(cloths))
    n0 = len(cloths[0][0])
    g.set_links(links([0, 1, 2], [n0, n0 + 1, n0 + 2], 0.5, 0.3, 0.001))      # icosphere to sheet
    if with_pressure:
        g.set_pressure(table)
    return g


def test_works_with_the_other_features():
    """the mixed scene on a multi-material engine with a force field, bending, damping, links and fast math: the pressure
    forces are the restatement's, the total vertex forces are the twin's plus the pressure's within one rounding of the
    sum, and substeps through every path run clean"""
    A = hs.ARR()
    scene = pr.scene("mixed")
    cloths, table, X, T, cv, cf = scene
    a, b = _featured_engine(cloths, True, table), _featured_engine(cloths, False, table)
    dt = min(1e-4, 0.5 * a.bending_max_stable_dt(), 0.5 * a.damping_max_stable_dt(), 0.5 * a.links_max_stable_dt())
    x0 = pr.state("random", X, cv)
    out = []
    for g in (a, b):
        hs.upload(g, x0)
        g.rebuild_mapping(False)
        g.calc_fem_state_and_force(dt)
        out.append(hs.vertices(g, A.FORCES))
    _check_forces(a, scene, "mixed random, every feature on")
    fp = a.pressure_forces()
    tot = out[1].astype(np.float64) + fp.astype(np.float64)
    err = np.abs(out[0].astype(np.float64) - tot)
    w = float((err / np.maximum(U * np.abs(out[0]).astype(np.float64), 1e-300))[err > 0].max()) if (err > 0).any() else 0.0
    hs.record("pressure: total forces, every feature on", w)
    assert fp.any() and w <= 1.0, w
    a.run_substeps(8, dt, -1)
    for _ in range(2):
        a.substep(dt, -1)
    ph, _ = a.profile_substeps(2, dt, -1)
    a.gpu_sync()
    assert ph["vforce"] > 0.0 and a.stats()["error_flags"] == 0, (ph, a.stats())
    assert np.isfinite(a.download(A.VELOCITIES)).all()
    _check_state(a, table, T, cf, "every feature on, after substeps")
    _check_forces(a, scene, "every feature on, after substeps")
    for g in (a, b):
        g.destroy()
