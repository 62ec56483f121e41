"""Bending stiffness (mpm_set_bending) on the engine.

1. mpm_bending_forces per vertex against the float64 restatement of tests/bending.py on every mesh x state, within
   R_i 2^-24 B_i (R_i = n_i + 3 counted from k_bend: one rounding for the float coefficient, one for the difference
   x_j - x_i, one per fused multiply-add of the row's n_i entries, one for second-order terms; tests/bending.py).  The
   same after substeps that forced a re-sort and after mpm_rebuild_mapping(sort = 1); on the same positions, uploaded
   again, the bits are those of the first evaluation.
2. MPM_ARR_FORCES of an engine with bending minus a twin's without is mpm_bending_forces, within one rounding of the sum.
3. ParticleToGrid node by node (tests/transfer_layouts.py) from the downloaded total forces, default and deterministic.
4. Scheduling: run_substeps(n), n x substep and the five phase calls are bit-equal through several re-sorts; the coupled
   path runs on a floor.
5. Off means off, to the bit and to the launch count of the re-sort checks.
6. Dynamics: a sheet wrapped onto a cylinder without membrane strain unbends; momentum stays zero; the twin stays put.
7. Refusals."""
import numpy as np
import pytest

from tests import bending as bd
from tests import harness as hs
from tests import transfer_layouts as tl

pytestmark = pytest.mark.gpu

U = bd.U
DT = 2e-4
PAIRS = [(m, s) for m in bd.MESHES for s in bd.STATES]


def _stiffness_for(g, n_cloths, dt, share=0.25, which=None):
    """[k] such that dt is `share` of mpm_bending_max_stable_dt (the limit scales with 1 / sqrt(k))"""
    on = [1.0 if which is None or c in which else 0.0 for c in range(n_cloths)]
    g.set_bending(on)
    lim = g.bending_max_stable_dt()
    assert np.isfinite(lim) and lim > 0
    k = np.float32((share * lim / dt) ** 2)
    ks = [float(k) * o for o in on]
    g.set_bending(ks)
    got = g.bending_max_stable_dt()
    assert abs(got * share / dt - 1.0) < 1e-3, (got, dt)
    return ks


def _check_forces(g, H, k, P, what):
    x = g.dump_cpu_state()[0]
    f = g.bending_forces()
    ref = bd.force64(float(np.float32(k)), H, x)
    B, R = bd.bound(float(np.float32(k)), H, x), bd.rounding_count(P)
    w = bd.margin(f - ref, B, R)
    print(f"bending forces: {what}: {w:.3g} of the bound, {bd.margin(f - ref, B, 1.0):.3g} of 2^-24 B_i")
    hs.record(f"bending forces: {what}", w)
    assert w <= 1.0, (what, w)
    return x, f, ref, B


# ---- 1 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,st", PAIRS)
def test_forces_against_float64(name, st):
    X, T = bd.mesh(name)
    H = bd.hinges(X, T)
    Q, P = bd.q_dense(len(X), H)
    k = 2.5e-5
    g = hs.engine([(X, T)])
    g.set_bending([k])
    assert np.array_equal(g.get_bending(), np.array([k], np.float32))
    x0 = bd.state(st, X)
    hs.upload(g, x0)
    x, f0, ref, B = _check_forces(g, H, k, P, f"{name} {st}")
    assert np.array_equal(x, x0)
    if st == "affine":
        pass   # (the force is what the rounding of the float positions leaves: the reference sees the same positions)
    elif H:
        assert np.abs(f0).max() > 100 * U * B.max(), "the state bends the mesh"
    else:
        assert not f0.any()
    # substeps that force a re-sort: the state five cells further along x, two short substeps
    before = g.stats()["rebuilds"]
    shift = np.array([5.0 / 64, 0.0, 0.0], np.float32)
    hs.upload(g, x0 + shift)
    g.run_substeps(2, 1e-5, -1)
    g.gpu_sync()
    assert g.stats()["error_flags"] == 0 and g.stats()["rebuilds"] > before, g.stats()
    _check_forces(g, H, k, P, f"{name} {st} after a re-sort")
    # the first positions again, in the new particle order: the same bits
    hs.upload(g, x0)
    f1 = g.bending_forces()
    assert np.array_equal(hs.bits(f1), hs.bits(f0)), float(np.abs(f1 - f0).max())
    g.rebuild_mapping(True)
    _check_forces(g, H, k, P, f"{name} {st} after sort = 1")
    f2 = g.bending_forces()
    assert np.array_equal(hs.bits(f2), hs.bits(f0)), float(np.abs(f2 - f0).max())
    assert g.stats()["error_flags"] == 0
    g.destroy()


def test_two_cloths_one_without_bending():
    """two cloths with different k, one of them 0: each cloth's rows are its own, the other gets zeros"""
    (Xa, Ta), (Xb, Tb) = bd.mesh("jittered"), bd.mesh("regular")
    Xb = (Xb + np.array([0.0, 0.0, 0.05], np.float32)).astype(np.float32)
    Ha, Hb = bd.hinges(Xa, Ta), bd.hinges(Xb, Tb)
    (_, Pa), (_, Pb) = bd.q_dense(len(Xa), Ha), bd.q_dense(len(Xb), Hb)
    g = hs.engine([(Xa, Ta), (Xb, Tb)])
    assert g.cloth_count() == 2 and not g.get_bending().any()
    xa, xb = bd.state("cylinder3", Xa), bd.state("perturbed", Xb)
    hs.upload(g, np.concatenate([xa, xb]))
    na = len(Xa)
    for ks in ((3e-5, 0.0), (0.0, 7e-5), (3e-5, 7e-5)):
        g.set_bending(ks)
        assert np.array_equal(g.get_bending(), np.array(ks, np.float32))
        f = g.bending_forces()
        for k, H, P, x, fc in ((ks[0], Ha, Pa, xa, f[:na]), (ks[1], Hb, Pb, xb, f[na:])):
            if k == 0.0:
                assert not fc.any()
                continue
            ref, B = bd.force64(float(np.float32(k)), H, x), bd.bound(float(np.float32(k)), H, x)
            w = bd.margin(fc - ref, B, bd.rounding_count(P))
            hs.record(f"bending forces: two cloths {ks}", w)
            assert w <= 1.0 and fc.any(), (ks, w)
    g.destroy()


# ---- 2 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["jittered", "fan"])
def test_total_forces_include_bending(name):
    """(the fan's hub has 12 faces: its membrane force comes from the adjacency walk, the jittered sheet's from DP::VF)"""
    A = hs.ARR()
    X, T = bd.mesh(name)
    a, b = hs.engine([(X, T)]), hs.engine([(X, T)])
    a.set_bending([4e-5])
    x0 = bd.state("cylinder3", X)
    nf = len(T)
    out = []
    for g in (a, b):
        hs.upload(g, x0)
        g.rebuild_mapping(False)
        g.calc_fem_state_and_force(DT)
        f, pids = g.download(A.FORCES), g.download(A.PIDS)
        fv = np.zeros((len(X), 3), np.float32)
        fv[pids[pids >= nf] - nf] = f[pids >= nf]
        out.append(fv)
    fb = a.bending_forces()
    assert fb.any() and out[1].any()
    tot = out[1].astype(np.float64) + fb.astype(np.float64)
    err = np.abs(out[0].astype(np.float64) - tot)
    w = float((err / np.maximum(U * np.abs(out[0]).astype(np.float64), 1e-300))[err > 0].max()) if (err > 0).any() else 0.0
    print(f"total forces: {name}: {w:.3g} of one rounding of the sum")
    hs.record(f"bending: total forces {name}", w)
    assert w <= 1.0, w
    assert not b.bending_forces().any() and b.bending_max_stable_dt() == np.inf
    for g in (a, b):
        assert g.stats()["error_flags"] == 0
        g.destroy()


# ---- 3 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["default", "deterministic"])
def test_p2g_node_by_node(mode):
    from tests import helpers
    helpers.tag_default_engine(mode == "default")
    A = hs.ARR()
    X, T = bd.mesh("jittered")
    nf = len(T)
    g = hs.engine([(X, T)], deterministic=mode == "deterministic")
    _stiffness_for(g, 1, tl.DT)
    hs.upload(g, bd.state("cylinder3", X), v=(0.3, -0.2, 0.1))
    g.rebuild_mapping(False)
    g.calc_fem_state_and_force(tl.DT)
    d = {k: g.download(a) for k, a in (("pids", A.PIDS), ("x", A.POSITIONS), ("v", A.VELOCITIES), ("C", A.AFFINE),
                                       ("m", A.MASSES), ("taus", A.TAUS), ("f", A.FORCES))}
    fb = g.bending_forces()
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
        print(f"bending p2g [{mode}] {field}: {w:.4g} of the bound")
        hs.record(f"bending: p2g [{mode}] {field}", w)
        assert w <= 1.0, (field, w)
    assert np.array_equal(flags, r["flags"])
    # bending is in the sums: without it the momentum is outside the bound
    fv = f.copy()
    fv[~face] -= fb[d["pids"][~face] - nf]
    r0 = tl.p2g64(d["x"], d["v"], d["C"], d["m"], taus, fv, 6, 2)
    assert tl.margin(np.abs(gmv - r0["mv"]), bmv) > 10


# ---- 4 -------------------------------------------------------------------------------------------------------------
def test_scheduling_through_resorts():
    """a bent sheet that flies and falls through several re-sorts, deterministic: run_substeps(n), n x substep and n x
    the five phase calls give the same bits in x, v, C and F -- a force added twice under the gate would not"""
    X, T = bd.mesh("regular")
    x0 = bd.state("cylinder30", X)
    n = 60
    es = [hs.engine([(X, T)]) for _ in range(3)]
    for g in es:
        _stiffness_for(g, 1, tl.DT)
        hs.upload(g, x0, v=(3.0, 0.4, 0.0))
    before = es[0].stats()["rebuilds"]
    es[0].run_substeps(n, tl.DT, -1)
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
    s = [hs.state(g) for g in es]
    hs.same_bits(s[0], s[1], "run_substeps(n) against n substeps")
    hs.same_bits(s[0], s[2], "run_substeps(n) against the phase calls")
    assert es[0].bending_forces().any()
    for g in es:
        g.destroy()


def test_coupled_path_runs():
    from drake_amd import Collider
    X, T = bd.mesh("regular")
    g = hs.engine([(X, T)], bodies=1)
    _stiffness_for(g, 1, tl.DT)
    x0 = bd.state("cylinder30", X)
    hs.upload(g, x0)
    floor = [Collider(0, body=0, p_WB=(0.5, 0.5, float(x0[:, 2].min()) - 0.002))]
    res = g.run_coupled_substeps(40, tl.DT, floor, 0.5, 1e5, 1e-4)
    g.gpu_sync()
    assert g.stats()["error_flags"] == 0
    assert max(r["contacts"] for r in res) > 0, "the sheet never reached the floor"
    assert np.isfinite(g.download(hs.ARR().VELOCITIES)).all()
    g.destroy()


# ---- 5 -------------------------------------------------------------------------------------------------------------
def test_off_means_off():
    """40 deterministic substeps through re-sorts: never set == all zeros == set and cleared with (h, 0, NULL), to the
    bit, and with the same number of re-sort check launches (the quiet-time hint is in use again)"""
    from drake_amd import scenes
    pos, idx = scenes.cloth_sheet(32, 0.3, 0.6, (0.3, 0.5))
    es = [hs.engine([(pos, idx.reshape(-1, 3))]) for _ in range(3)]
    es[1].set_bending([0.0])
    es[2].set_bending([1e-5])
    assert es[2].bending_max_stable_dt() < np.inf
    es[2].set_bending([])
    assert not es[2].get_bending().any() and es[2].bending_max_stable_dt() == np.inf
    vel = np.array([4.0, 0.3, 0.0], np.float32) + 0.05 * np.random.default_rng(3).normal(size=pos.shape).astype(np.float32)
    before = es[0].stats()["rebuilds"]
    for g in es:
        pids = g.download(hs.ARR().PIDS)
        allv = np.concatenate([vel[g._tri].mean(axis=1), vel]).astype(np.float32)
        g.upload_particle_state(None, allv[pids], None, None, None)
        for _ in range(4):
            g.run_substeps(10, tl.DT, -1)
        g.gpu_sync()
        assert g.stats()["error_flags"] == 0
    assert es[0].stats()["rebuilds"] - before >= 2, es[0].stats()
    s = [hs.state(g) for g in es]
    hs.same_bits(s[0], s[1], "all zeros")
    hs.same_bits(s[0], s[2], "set and cleared")
    assert es[0].stats()["resort_checks"] == es[1].stats()["resort_checks"] == es[2].stats()["resort_checks"]
    for g in es:
        g.destroy()


# ---- 6 -------------------------------------------------------------------------------------------------------------
def _inscribed_cylinder(X, radius):
    """the regular sheet folded along its grid lines onto a cylinder: column i at angle i * 2 asin(h / 2 R), so that
    every triangle is congruent to its rest triangle (no membrane strain)"""
    X = np.asarray(X, np.float64)
    i = np.rint((X[:, 0] - X[:, 0].min()) / bd.H0)
    th = (i - 0.5 * i.max()) * 2.0 * np.arcsin(bd.H0 / (2.0 * radius))
    return np.stack([bd.CENTER[0] + radius * np.sin(th), X[:, 1], bd.CENTER[2] + radius * (1.0 - np.cos(th))], 1)


def _frames(x, T):
    x = np.asarray(x, np.float64)
    d1, d2 = x[T[:, 1]] - x[T[:, 0]], x[T[:, 2]] - x[T[:, 0]]
    n = np.cross(d1, d2)
    n /= np.linalg.norm(n, axis=1)[:, None]
    return np.stack([d1, d2, n], axis=2)          # columns


def test_bent_sheet_unbends():
    """Zero gravity, the 13 x 13 sheet at rest on a cylinder of radius 6 spacings, every face a rigid image of its rest
    face with F = (rotation) x (rest F), so that the membrane force is zero.  dt is a quarter of
    mpm_bending_max_stable_dt, 20 substeps -- well inside the first quarter period of the lowest mode.
    * The float64 bending energy of the downloaded positions is below its initial value.
    * Total momentum.  CalcFemStateAndForce replaces every face particle's velocity by the mean of its corners'
      (the engine's model with or without bending), which changes sum m v by what the two interpolations of the grid
      velocity differ by: from rest, sum m v over all particles reached 5.8e-4 of a gross sum m |v| of 4.2e-3 after
      20 substeps on an MI355X, all of it entering at the FEM calls (per substep: -6.5811e-6 after the FEM call,
      -6.5807e-6 after GridToParticle).  What the forces add is the change from after the FEM call -- the momentum
      ParticleToGrid transfers -- to after GridToParticle of the same substep: summed over the substeps it stays
      within steps x (128 u sum m |v| + dt u sum_i (R_i B_i + 16 |f_i|)) of zero: per substep, ParticleToGrid and
      GridToParticle each round a particle's 27 contributions (the P2G bound of tests/transfer_layouts.py is
      K (L + 16) u, the G2P one 27 u: 128 u covers both on this sheet), the bending force sums to zero within its own
      bound, the membrane force within a few roundings of its terms.
    * The twin without bending moves at most 1/2 a T^2, a = 16 (lambda + 2 mu) / rho s / h: its only force comes from
      the rounding of the positions, a strain of at most s = 8 u max|x| / h per face."""
    A = hs.ARR()
    X, T = bd.mesh("regular")
    H = bd.hinges(X, T)
    Q, P = bd.q_dense(len(X), H)
    h, steps = bd.H0, 20
    x0 = _inscribed_cylinder(X, 6 * h).astype(np.float32)
    rot = _frames(x0, T) @ np.linalg.inv(_frames(X, T))
    mat = dict(gravity=0.0)
    a, b = hs.engine([(X, T)], material=mat), hs.engine([(X, T)], material=mat)
    ks = _stiffness_for(a, 1, DT)
    for g in (a, b):
        F0 = g.download(A.DEFORMATION_GRADIENTS).reshape(-1, 3, 3).astype(np.float64)
        hs.upload(g, x0, F=(rot @ F0).astype(np.float32).reshape(-1, 9))
    E0 = bd.energy64(ks[0], H, x0)
    f0 = a.bending_forces().astype(np.float64)
    B0 = bd.bound(ks[0], H, x0)
    def momentum(g):
        m, v = g.download(A.MASSES).astype(np.float64), g.download(A.VELOCITIES).astype(np.float64)
        return (m[:, None] * v).sum(axis=0), float((m[:, None] * np.abs(v)).sum(axis=0).max())

    added, gross = np.zeros(3), 0.0
    for _ in range(steps):
        a.rebuild_mapping(False)
        a.calc_fem_state_and_force(DT)
        p0, _ = momentum(a)
        a.particle_to_grid(DT)
        a.update_grid(-1)
        a.grid_to_particle(DT)
        p1, g1 = momentum(a)
        added += p1 - p0
        gross = max(gross, g1)
    b.run_substeps(steps, DT, -1)
    for g in (a, b):
        g.gpu_sync()
        assert g.stats()["error_flags"] == 0
    x1 = a.dump_cpu_state()[0]
    E1 = bd.energy64(ks[0], H, x1)
    print(f"unbending: E {E0:.6e} -> {E1:.6e}, max displacement {np.abs(x1 - x0).max():.3e}")
    assert E1 < E0, (E0, E1)
    mom = float(np.abs(added).max())
    bound = steps * (128 * U * gross + DT * U * float((bd.rounding_count(P) * B0 + 16 * np.abs(f0).max(axis=1)).sum()))
    print(f"unbending: momentum added by the substeps {mom:.3e}, bound {bound:.3e}, gross {gross:.3e}; "
          f"sum m v at the end {np.abs(momentum(a)[0]).max():.3e}")
    hs.record("bending: momentum of the unbending sheet", mom / bound)
    assert gross > 0 and mom <= bound, (mom, bound)
    # the twin
    mt = b.default_material()
    mu = mt.youngs_modulus / (2 * (1 + mt.poisson_ratio))
    lam = mt.youngs_modulus * mt.poisson_ratio / ((1 + mt.poisson_ratio) * (1 - 2 * mt.poisson_ratio))
    s = 8 * U * float(np.abs(x0).max()) / h
    still = 0.5 * (16 * (lam + 2 * mu) / mt.density * s / h) * (steps * DT) ** 2
    moved = float(np.abs(b.dump_cpu_state()[0] - x0).max())
    print(f"unbending: the twin moved {moved:.3e}, bound {still:.3e}; the bent sheet {np.abs(x1 - x0).max():.3e}")
    hs.record("bending: the twin without bending", moved / still)
    assert moved <= still, (moved, still)
    assert float(np.abs(x1 - x0).max()) > still, "the bending force moves the sheet"
    for g in (a, b):
        g.destroy()


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
    refused(lambda: g0.set_bending([1e-5]), says="finalize")
    g0.destroy()
    # a face of zero rest area in a cloth with k > 0; with k = 0 nobody asks
    Xd = X.copy()
    i, j, k = T[7]
    Xd[k] = 0.5 * (Xd[i] + Xd[j])
    gd = hs.engine([(Xd, T), (X + np.array([0, 0, 0.05], np.float32), T)])
    refused(lambda: gd.set_bending([1e-5, 1e-5]), says="face 7")
    assert not gd.get_bending().any() and gd.bending_max_stable_dt() == np.inf
    gd.set_bending([0.0, 1e-5])
    gd.destroy()

    g = hs.engine([(X, T)], bodies=1)
    good = _stiffness_for(g, 1, tl.DT, share=0.9)
    lim = g.bending_max_stable_dt()
    x0 = bd.state("cylinder30", X)
    hs.upload(g, x0)
    f_before = g.bending_forces()
    for bad in ([-1e-5], [np.nan], [np.inf], [1e-5, 1e-5]):
        refused(lambda bad=bad: g.set_bending(bad))
    assert np.array_equal(g.get_bending(), np.array(good, np.float32)) and g.bending_max_stable_dt() == lim
    assert np.array_equal(hs.bits(g.bending_forces()), hs.bits(f_before))
    # partitioned, halo, team and chain calls on an engine with bending
    nb = 64 // 4
    refused(lambda: g.dist_init(0, 1, [0, nb], 2, 2, 2), says="bending")
    refused(lambda: g.substep_mid_halo(tl.DT), says="bending")
    refused(lambda: g.team_prepare(), says="bending")
    refused(lambda: g.chain_substeps(1, tl.DT), says="bending")
    # a dt above the limit: every entry point that takes one, nothing enqueued
    before = g.stats()["substeps"]
    big = 1.01 * lim
    floor = [Collider(0, body=0, p_WB=(0.5, 0.5, 0.3))]
    for call in (lambda: g.run_substeps(2, big, -1), lambda: g.substep(big, -1), lambda: g.particle_to_grid(big),
                 lambda: g.profile_substeps(2, big, -1), lambda: g.run_coupled_substeps(2, big, floor, 0.5, 1e5, 1e-4),
                 lambda: g.substep_begin(big)):
        refused(call, says="mpm_bending_max_stable_dt")
    assert g.stats()["substeps"] == before
    g.run_substeps(2, tl.DT, -1)
    ph, _ = g.profile_substeps(2, tl.DT, -1)
    assert ph["vforce"] > 0.0, ph          # (k_vforce and k_bend are timed under MPM_PHASE_VFORCE)
    g.gpu_sync()
    assert g.stats()["error_flags"] == 0
    # off lifts the refusals; a partitioned engine refuses the call
    g.set_bending([0.0])
    g.run_substeps(1, big, -1)
    g.dist_init(0, 1, [0, nb], 2, 2, 2)
    refused(lambda: g.set_bending(good), says="partitioned")
    assert not g.get_bending().any()
    g.destroy()
