"""HIP engine vs CPU oracle through the C ABI, phase by phase and over short
trajectories.  Runs on the GPU box only (pytest -m gpu)."""
import numpy as np
import pytest

from tests.helpers import RTOL, build_pair, close, natural_scales
from tests import harness as hs

pytestmark = pytest.mark.gpu

DT = 1e-3


def test_finalize_matches_initialize_fem_state():
    A = hs.ARR()
    o, g = build_pair()
    close(g.download(A.VOLUMES), o.vol, what="volumes")
    close(g.download(A.DEFORMATION_GRADIENTS), o.F, scale=1.0, what="F0")
    close(g.download(A.DM_INVERSES), o.DmInv, what="DmInv")
    close(g.download(A.POSITIONS), o.pos, scale=1.0, what="pos")
    close(g.download(A.VELOCITIES), o.vel, what="vel")
    assert np.array_equal(g.download(A.INDICES).reshape(-1), o.indices)
    assert np.array_equal(g.download(A.PIDS), o.pids)
    p, i = g.dump_cpu_state()
    po, io = o.dump_cpu_state()
    assert np.array_equal(i, io)
    assert np.array_equal(p, po)


def test_keys_bit_exact_and_sort_maps():
    A = hs.ARR()
    o, g = build_pair()
    o.rebuild_mapping(False)
    g.rebuild_mapping(False)
    assert np.array_equal(g.download(A.SORT_KEYS), o.sort_keys)
    # RebuildMapping(sort=true): slot permutation must be the reference's stable 16-bit sort
    o.rebuild_mapping(True)
    g.rebuild_mapping(True)
    assert np.array_equal(g.download(A.PIDS), o.pids)
    assert np.array_equal(g.download(A.INDEX_MAPPINGS), o.index_mappings)
    assert np.array_equal(g.download(A.SORT_KEYS), o.sort_keys)
    close(g.download(A.POSITIONS), o.pos, scale=1.0, what="sorted pos")
    close(g.download(A.VOLUMES), o.vol, what="sorted vol")


@pytest.mark.parametrize("bc", [-1, 0, 1, 2, 3])
def test_phase_by_phase(bc):
    A = hs.ARR()
    # place the sheets where the analytic colliders of that scene live
    z0 = {-1: 0.5, 0: 0.56, 1: 0.75, 2: 0.11, 3: 0.5}[bc]
    side = {-1: 0.3, 0: 0.3, 1: 0.34, 2: 0.3, 3: 0.5}[bc]
    o, g = build_pair(z0=z0, side=side)
    for step in range(3):
        sc = natural_scales(o, DT, bc)
        # same inputs on both sides for every step, so each kernel is judged on one step's rounding
        # (the stiff cloth amplifies differences from step to step; trajectories are tested below)
        g.upload_particle_state(o.pos, o.vel, o.C, None, o.F)
        o.rebuild_mapping(False)
        g.rebuild_mapping(False)
        assert np.array_equal(g.download(A.SORT_KEYS), o.sort_keys)
        o.calc_fem_state_and_force(DT)
        g.calc_fem_state_and_force(DT)
        close(g.download(A.DEFORMATION_GRADIENTS), o.F, scale=1.0, what="F")
        # Stress is E * (F - R): one ulp of F (1e-7) is already E * 1e-7 of stress, so the natural
        # scale of tau is vol * E (unit strain) and of a nodal force vol * E / edge; an undeformed
        # cloth has tau = rounding noise far below that.
        s_tau = max(float(np.abs(o.taus).max()), sc["vol"] * 4e5)
        close(g.download(A.TAUS), o.taus, scale=s_tau, what="taus")
        close(g.download(A.FORCES), o.forces, scale=max(float(np.abs(o.forces).max()), s_tau * (1 << o.domain_bits)),
              what="forces")
        close(g.download(A.POSITIONS), o.pos, scale=1.0, what="pos after fem")
        close(g.download(A.VELOCITIES), o.vel, scale=sc["vel"], what="vel after fem")
        o.particle_to_grid(DT)
        g.particle_to_grid(DT)
        gm = g.download(A.GRID_MASSES)
        close(gm, o.g_m, what="grid mass")
        # momentum is a sum with cancellation: scale by |v|max * m_max
        close(g.download(A.GRID_MOMENTUM), o.g_mv, scale=sc["vel"] * float(o.g_m.max()), what="grid mv")
        assert np.array_equal(g.download(A.GRID_TOUCHED_FLAGS), o.g_flags)
        o.update_grid(bc)
        g.update_grid(bc)
        assert g.grid_touched_cnt() == o.g_cnt
        assert np.array_equal(g.download(A.GRID_TOUCHED_IDS), o.touched_blocks())
        vsc = sc["vel"]
        # A node's velocity is a quotient of two sums that are both tiny on the stencil fringe; what
        # reaches the particles is w * v with the same tiny w, so nodes are compared mass-weighted.
        wgt = (o.g_m / o.g_m.max())[:, None]
        close(g.download(A.GRID_MOMENTUM) * wgt, o.g_mv * wgt, scale=vsc, what="grid v")
        close(g.download(A.GRID_V_STAR) * wgt, o.g_vstar * wgt, scale=vsc, what="grid v*")
        o.grid_to_particle(DT)
        g.grid_to_particle(DT)
        sc = natural_scales(o)
        close(g.download(A.POSITIONS), o.pos, scale=1.0, what="pos")
        close(g.download(A.VELOCITIES), o.vel, scale=vsc, what="vel")
        close(g.download(A.AFFINE), o.C, scale=4.0 * (1 << o.domain_bits) * vsc, what="C")
    g.gpu_sync()


def test_trajectory_with_sorts_and_rebuilds():
    """20 substeps; the reference-style sort every 4th step on both sides; the engine's
    own block re-sort triggers by itself.  Compared in original particle order."""
    A = hs.ARR()
    o, g = build_pair(layers=4, res=24, vel_amp=1.0)
    for step in range(20):
        srt = step % 4 == 0
        o.substep(DT, -1, sort=srt)
        g.rebuild_mapping(srt)
        g.calc_fem_state_and_force(DT)
        g.particle_to_grid(DT)
        g.update_grid(-1)
        g.grid_to_particle(DT)
    g.gpu_sync()
    st = g.stats()
    assert st["error_flags"] == 0
    pid_g = g.download(A.PIDS)
    so = o.state_in_original_order()
    sc = natural_scales(o)

    def orig(a):
        out = np.empty_like(a)
        out[pid_g] = a
        return out

    # after 20 steps rounding differences have been amplified by the stiff cloth: against the plain max|v| (1 m/s
    # here), 3e-4 = the order the float-vs-double oracle distance reaches on the benchmark scenes in 10 substeps
    # (tests/test_precision_gpu.py); observed 6e-5
    close(orig(g.download(A.POSITIONS)), so["pos"], scale=1.0, rtol=1e-5, what="traj pos")
    close(orig(g.download(A.VELOCITIES)), so["vel"], rtol=3e-4, what="traj vel")
    close(orig(g.download(A.VOLUMES)), so["vol"], what="traj vol")
    # index maps, per original particle: equal unless the particle sits within rounding of a cell face
    o.rebuild_mapping(False)  # keys of the current positions (the engine derives them on demand)
    ko = np.empty_like(o.sort_keys)
    ko[o.pids] = o.sort_keys
    assert (orig(g.download(A.SORT_KEYS)) == ko).mean() > 0.995
    # pids / index_mappings stay mutually inverse permutations
    im = g.download(A.INDEX_MAPPINGS)
    assert np.array_equal(im[pid_g], np.arange(pid_g.size))


def _fan_sheet(n_rim, radius, centre, z, seed):
    """A disc of n_rim triangles around a hub vertex: the hub has n_rim faces around it."""
    ang = 2.0 * np.pi * np.arange(n_rim) / n_rim
    pos = np.zeros((n_rim + 1, 3), np.float32)
    pos[0] = (centre[0], centre[1], z)
    pos[1:, 0] = centre[0] + radius * np.cos(ang)
    pos[1:, 1] = centre[1] + radius * np.sin(ang)
    pos[1:, 2] = z
    idx = np.stack([np.zeros(n_rim, np.int32), 1 + np.arange(n_rim, dtype=np.int32),
                    1 + (np.arange(n_rim, dtype=np.int32) + 1) % n_rim], -1).reshape(-1)
    rng = np.random.default_rng(seed)
    vel = (0.3 * rng.standard_normal(pos.shape)).astype(np.float32)
    return pos, vel, idx


def test_vertex_with_more_than_eight_faces():
    """The vertex-force gather keeps eight adjacent (face, corner) records per vertex; a vertex with more walks the
    adjacency CSR (vertex_force_from).  Such a mesh also takes a different route through a batched substep: the forces
    of its vertices are not summed inside k_p2g from the per-vertex records k_fem scatters (DP::VF), k_vforce is launched
    (fused_forces, mpm_engine.hip), and the faces around the hub write their triples to G3.  A fan of 12 faces next to a
    regular sheet, against the oracle, phase by phase and batched, across re-sorts."""
    from drake_amd import scenes
    A = hs.ARR()
    dx = 1.0 / 64

    def sheets():
        reg = scenes.cloth_stack(1, 14, 6, z0=0.5, side=0.2, seed=3, vel_amp=0.3)
        return list(reg) + [_fan_sheet(12, 0.9 * dx, (0.5, 0.5), 0.5 + 3 * dx, 5), _fan_sheet(8, 0.8 * dx, (0.42, 0.55), 0.5 + 3 * dx, 6)]

    o, g1 = build_pair(sheets=sheets())
    _, g2 = build_pair(sheets=sheets())
    vel = o.vel.copy()
    vel[:, 0] += 6.0           # a cell every third substep: re-sorts on the way
    o.vel[:] = vel
    for g in (g1, g2):
        g.upload_particle_state(None, vel)
    n = 9
    for _ in range(n):
        o.substep(DT, -1, sort=False)
        g2.rebuild_mapping(False)
        g2.calc_fem_state_and_force(DT)
        g2.particle_to_grid(DT)
        g2.update_grid(-1)
        g2.grid_to_particle(DT)
    g1.run_substeps(4, DT, -1)
    g1.run_substeps(n - 4, DT, -1)
    so = o.state_in_original_order()
    sc = natural_scales(o, DT)
    for g, what in ((g1, "batched"), (g2, "phase calls")):
        st = g.stats()
        assert st["error_flags"] == 0 and st["rebuilds"] >= 2, st
        pid = g.download(A.PIDS)
        x, v = np.empty_like(so["pos"]), np.empty_like(so["vel"])
        x[pid], v[pid] = g.download(A.POSITIONS), g.download(A.VELOCITIES)
        close(x, so["pos"], scale=1.0, what=f"fan mesh, {what}: pos")
        close(v, so["vel"], scale=max(sc["vel"], 6.0), rtol=3 * RTOL, what=f"fan mesh, {what}: vel")
    # the forces a caller downloads after CalcFemStateAndForce, hub and rim, on a state one substep old
    # (one substep in: the rest state has no forces to compare)
    o3, g3 = build_pair(sheets=sheets())
    o3.substep(DT, -1, sort=False)
    g3.substep(DT, -1)
    o3.rebuild_mapping(False)
    o3.calc_fem_state_and_force(DT)
    g3.rebuild_mapping(False)
    g3.calc_fem_state_and_force(DT)
    pid = g3.download(A.PIDS)
    f = np.empty_like(o3.forces)
    f[pid] = g3.download(A.FORCES)
    fo = np.empty_like(o3.forces)
    fo[o3.pids] = o3.forces
    assert np.abs(fo).max() > 0
    # (the natural scale of a nodal force is vol * E / edge -- unit strain --, as in test_phase_by_phase)
    close(f, fo, scale=max(float(np.abs(fo).max()), float(np.max(o3.vol)) * 4e5 * 64), what="fan mesh: vertex forces")


def test_double_and_fixed_point_tiles_of_p2g_agree(monkeypatch):
    """ParticleToGrid accumulates the node sums of a work item in LDS in double precision (the default) or in 64-bit
    fixed point (deterministic mode; MPM_P2G_FIXED=1 selects it alone).  Both sum the float contributions of the waves
    exactly and round once.  (The contributions themselves are float sums over the particles of a cell in the order the
    re-sort left them, which differs between two engines outside deterministic mode: that is the rounding noise the
    comparison allows for.)"""
    from drake_amd import GpuMpm, scenes
    A = hs.ARR()

    def grid(fixed):
        if fixed:
            monkeypatch.setenv("MPM_P2G_FIXED", "1")
        else:
            monkeypatch.delenv("MPM_P2G_FIXED", raising=False)
        g = GpuMpm(6)
        scenes.populate(g, scenes.cloth_stack(3, 40, 6, z0=0.5, side=0.5, seed=21, vel_amp=1.0))
        g.rebuild_mapping(False)
        g.calc_fem_state_and_force(DT)
        g.particle_to_grid(DT)
        g.gpu_sync()
        assert g.stats()["error_flags"] == 0
        return g.download(A.GRID_MASSES), g.download(A.GRID_MOMENTUM)

    (m_d, p_d), (m_f, p_f) = grid(False), grid(True)
    assert float(m_d.sum()) > 0
    for a, b, what in ((m_d, m_f, "mass"), (p_d, p_f, "momentum")):
        close(a, b, rtol=2e-6, what=f"double vs fixed-point tile: grid {what}")


@pytest.mark.parametrize("deterministic", [True, False])
def test_substep_equals_phase_calls(deterministic):
    """mpm_substep against the reference's five calls, five substeps.
    deterministic (mpm_set_deterministic from Finalize's first sort on: canonical particle order inside every cell,
    fixed-point tile sums): the two call patterns run the same arithmetic in the same order -- BITWISE equal positions,
    velocities and affine matrices (VERDICT r5 item 2 / ADVICE r5: the tight gate where it can be made exact).
    Otherwise (the smoke variant on the default engine): the order of the particles inside a cell comes out of atomics at
    every re-sort, and the per-cell partial sums of ParticleToGrid are float sums in that order -- last-bit differences
    of the grid, which stay at a few hundredths of the measured one-substep float noise for almost every particle.
    Almost: the reference's return mapping (cuda_mpm_kernels.cuh:183-294) BRANCHES on the normal stretch, and a face
    that sits on a branch point takes one side or the other with the last bit of its input (scratch/substep_repeat.py,
    40 runs of this scene: in 30 the largest difference is 0.02-0.04 noises; in 8 face 2439 flips at substep 3 and ends
    6.3-6.9 noises apart, in 2 face 2664 at substep 5).  Hence there: nine in ten particles within 0.4 noises, all but
    2 % within 4, nobody beyond 40."""
    A = hs.ARR()
    o, g1 = build_pair(seed=11, deterministic=deterministic)
    _, g2 = build_pair(seed=11, deterministic=deterministic)
    sc = natural_scales(o, DT)
    for _ in range(5):
        g1.substep(DT, -1)
        g2.rebuild_mapping(False)
        g2.calc_fem_state_and_force(DT)
        g2.particle_to_grid(DT)
        g2.update_grid(-1)
        g2.grid_to_particle(DT)
    v1, v2 = g1.download(A.VELOCITIES), g2.download(A.VELOCITIES)
    if deterministic:
        assert np.array_equal(g1.download(A.POSITIONS), g2.download(A.POSITIONS))
        assert np.array_equal(v1, v2)
        assert np.array_equal(g1.download(A.AFFINE), g2.download(A.AFFINE))
        assert np.abs(v1).max() > 0
        return
    close(g1.download(A.POSITIONS), g2.download(A.POSITIONS), scale=1.0, rtol=1e-6, what="substep pos")
    # (a flip disturbs its neighbourhood through the grid in the substeps that follow: 71 - 177 of the scene's 3,400
    # particles beyond 0.4 noises, 6 - 7 of them beyond 4, in the four runs of forty that had one)
    order = np.argsort(np.abs(v1 - v2).max(axis=1))
    n = len(order)
    for share, rtol, what in ((0.90, 1e-6, "nine in ten particles"), (0.98, 1e-5, "all but 2 % of the particles"), (1.0, 1e-4, "every particle")):
        sel = order[: max(1, int(n * share))]
        close(v1[sel], v2[sel], scale=sc["vel"], rtol=rtol, what=f"substep vel ({what}; default engine)")


def test_batched_substeps_with_resorts_in_between_equal_phase_calls():
    """mpm_run_substeps enqueues the four re-sort launches only in front of every fourth substep; a substep
    without them that finds a re-sort pending does nothing and is run again, with the re-sort, at the next
    synchronisation point (Ctl::skipped / settle).  Sheets that cross a cell every other substep force
    re-sorts inside the batch: the result must be the one of phase-by-phase calls, which re-sort on demand
    before every substep."""
    A = hs.ARR()
    o, g1 = build_pair(seed=5, vel_amp=0.1)
    _, g2 = build_pair(seed=5, vel_amp=0.1)
    vel = o.vel.copy()
    vel[:, 0] += 9.0           # 9 m/s * 1e-3 s * 64 cells = 0.58 cells per substep
    for g in (g1, g2):
        g.upload_particle_state(None, vel)
    n = 14
    g1.run_substeps(5, DT, -1)
    g1.run_substeps(n - 5, DT, -1)      # (a second batch while substeps of the first may still be owed)
    for _ in range(n):
        g2.rebuild_mapping(False)
        g2.calc_fem_state_and_force(DT)
        g2.particle_to_grid(DT)
        g2.update_grid(-1)
        g2.grid_to_particle(DT)
    s1, s2 = g1.stats(), g2.stats()
    assert s1["error_flags"] == 0 and s2["error_flags"] == 0
    assert s1["rebuilds"] >= 3 and s2["rebuilds"] >= 3, (s1, s2)
    sc = natural_scales(o, DT)
    x1, x2 = g1.download(A.POSITIONS), g2.download(A.POSITIONS)
    assert np.abs(x1[:, 0] - o.pos[:, 0]).min() > 0.9 * 9.0 * n * DT      # everybody made all n substeps
    close(x1, x2, scale=1.0, rtol=1e-6, what="batched substeps pos")
    # (the two runs re-sort at different substeps: different particle order inside the cells, last-bit
    # differences of the grid sums; the same 1e-5 as everywhere)
    close(g1.download(A.VELOCITIES), g2.download(A.VELOCITIES), scale=max(sc["vel"], 9.0), rtol=RTOL, what="batched substeps vel")


def test_free_fall_and_conservation_large():
    """Size-independent properties at a size the oracle is not run on: 250k particles on 128^3."""
    from drake_amd import ARR as A, GpuMpm, scenes
    g = GpuMpm(7)
    scenes.populate(g, scenes.cloth_stack(8, 102, 7, z0=0.6, vel_amp=0.0, jitter=0.0))
    vol = g.download(A.VOLUMES)
    n = 20
    for _ in range(n):
        g.rebuild_mapping(False)
        g.calc_fem_state_and_force(DT)
        g.particle_to_grid(DT)
        m = g.download(A.GRID_MASSES)
        mv = g.download(A.GRID_MOMENTUM)
        g.update_grid(-1)
        g.grid_to_particle(DT)
    g.gpu_sync()
    assert g.stats()["error_flags"] == 0
    mass = float(vol.astype(np.float64).sum() * 2000.0)
    assert abs(float(m.astype(np.float64).sum()) - mass) <= 2e-5 * mass
    v = g.download(A.VELOCITIES)
    np.testing.assert_allclose(v[:, 2], -9.8 * DT * n, rtol=5e-5)
    assert np.max(np.abs(v[:, :2])) < 1e-4
    # grid momentum of the last scatter = particle momentum before it + gravity impulse
    pz = float(mv[:, 2].astype(np.float64).sum())
    expect = mass * (-9.8 * DT * n)
    assert abs(pz - expect) <= 1e-4 * abs(expect)


def test_slot_sort_is_the_stable_16_bit_sort_at_full_size():
    """RebuildMapping(sort=true) at the benchmark size (1M particles): the slot permutation must be
    the stable sort on the low 16 key bits (cuda_mpm_solver.cu:47-68), applied twice (a second sort
    permutes an already permuted slot order)."""
    from drake_amd import ARR as A, GpuMpm, scenes
    bits, layers, res = scenes.CONFIGS["cloth_1m"]
    g = GpuMpm(bits)
    scenes.populate(g, scenes.cloth_stack(layers, res, bits))
    pids = np.arange(g.n_particles, dtype=np.int32)
    for rounds in range(2):
        g.run_substeps(7, DT, -1)
        g.rebuild_mapping(False)
        keys = g.download(A.SORT_KEYS)          # key of the particle in each slot, before the sort
        assert np.array_equal(g.download(A.PIDS), pids)
        order = np.argsort(keys & np.uint32(0xFFFF), kind="stable")
        g.rebuild_mapping(True)
        pids = pids[order]
        assert np.array_equal(g.download(A.PIDS), pids)
        imap = np.empty_like(pids)
        imap[pids] = np.arange(pids.size, dtype=np.int32)
        assert np.array_equal(g.download(A.INDEX_MAPPINGS), imap)
        assert np.array_equal(g.download(A.SORT_KEYS), keys[order])
    assert g.stats()["error_flags"] == 0


def test_error_paths_and_edge_cases():
    from drake_amd import GpuMpm, MpmError
    g = GpuMpm(6)
    with pytest.raises(MpmError):
        g.finalize()  # no particles
    g = GpuMpm(6)
    with pytest.raises(MpmError):
        g.add_qr_cloth(np.zeros((3, 3), np.float32), np.zeros((3, 3), np.float32), np.array([0, 1, 5], np.int32))
    # a single triangle, and vertices without faces, are legal inputs
    g = GpuMpm(6)
    pos = np.array([[0.5, 0.5, 0.5], [0.52, 0.5, 0.5], [0.5, 0.52, 0.5], [0.6, 0.6, 0.6]], np.float32)
    g.add_qr_cloth(pos, np.zeros_like(pos), np.array([0, 1, 2], np.int32))
    g.finalize()
    with pytest.raises(MpmError):
        g.update_grid(-1)  # before ParticleToGrid
    for _ in range(3):
        g.substep(DT, -1)
    g.gpu_sync()
    assert g.n_particles == 5 and g.n_faces == 1


def test_domain_error_and_fast_particles():
    """A particle outside the grid (undefined behaviour in the reference) is reported at the next
    sync as MPM_ERR_DOMAIN; fast particles are not an error."""
    from drake_amd import GpuMpm, MpmError, scenes

    def small():
        g = GpuMpm(6)
        scenes.populate(g, scenes.cloth_stack(2, 12, 6, z0=0.5))
        return g

    g = small()
    pos = g.sync_particle_state_to_cpu()
    bad = pos.copy()
    bad[5, 2] = -0.25                       # below the grid
    g.upload_particle_state(bad)
    g.rebuild_mapping(False)
    with pytest.raises(MpmError) as ei:
        g.gpu_sync()
    assert ei.value.code == -6
    # fast motion is legal: the re-sort is requested by G2P for exactly the particles that left their
    # tile and runs before the next transfer, so 3.8 cells per substep is as good as 0.1
    # (re-sorts: the one the upload asks for, then one per substep unless the anticipatory binning --
    # particles are binned up to 1.75 cells ahead of where they are -- happens to keep everybody inside)
    g = small()
    vel = np.zeros((g.n_particles, 3), np.float32)
    vel[:, 2] = -60.0                       # 60 m/s * 1e-3 s = 3.8 cells of 1/64 per substep
    g.upload_particle_state(None, vel)
    z0 = g.sync_particle_state_to_cpu()[:, 2].copy()
    for _ in range(3):
        g.substep(DT, -1)
    g.gpu_sync()
    assert g.stats()["error_flags"] == 0 and g.stats()["rebuilds"] >= 2
    dz = g.sync_particle_state_to_cpu()[:, 2] - z0
    np.testing.assert_allclose(dz, -(60.0 * 3 * DT + 9.8 * DT * DT * 6), rtol=1e-3)


def test_deterministic_mode_is_bitwise_reproducible():
    """mpm_set_deterministic: two engines fed the same scene agree to the bit after a run with many
    re-sorts (without the switch they agree to rounding only)."""
    from drake_amd import ARR as A, GpuMpm, scenes

    def run(det):
        g = GpuMpm(7)
        g.set_deterministic(det)
        sheets = scenes.cloth_stack(6, 64, 7, z0=0.6, vel_amp=0.3)
        for pos, vel, idx in sheets:
            vel[:, 0] += 1.5          # cross cells quickly: a re-sort every few substeps
        scenes.populate(g, sheets)
        g.run_substeps(60, DT, -1)
        out = (g.sync_particle_state_to_cpu(), g.download(A.VELOCITIES), g.download(A.AFFINE),
               g.download(A.DEFORMATION_GRADIENTS))
        st = g.stats()
        assert st["error_flags"] == 0 and st["rebuilds"] >= 3
        return out

    a, b = run(True), run(True)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    c = run(False)
    np.testing.assert_allclose(c[0], a[0], rtol=0, atol=2e-5)


def test_rigid_translation_is_preserved_at_full_size():
    """Size-independent property at the benchmark size (1M particles, many re-sorts): without
    gravity a cloth stack that moves with one velocity keeps it exactly (the B-spline weights are a
    partition of unity), develops no affine field and no strain."""
    from drake_amd import ARR as A, GpuMpm, scenes
    bits, layers, res = scenes.CONFIGS["cloth_1m"]
    m = GpuMpm.default_material()
    m.gravity = 0.0
    g = GpuMpm(bits, m)
    v0 = np.array([1.1, -0.7, 0.4], np.float32)
    sheets = scenes.cloth_stack(layers, res, bits, z0=0.45, vel_amp=0.0, jitter=0.05)
    for pos, vel, idx in sheets:
        vel[:] = v0
    scenes.populate(g, sheets)
    x0 = g.sync_particle_state_to_cpu().astype(np.float64)
    n = 120
    g.run_substeps(n, DT, -1)
    st = g.stats()
    assert st["error_flags"] == 0 and st["rebuilds"] >= 6
    v = g.download(A.VELOCITIES)
    # (rounding noise in the strain is amplified by the stiff cloth: 1e-4 m/s after 120 substeps)
    np.testing.assert_allclose(v, np.broadcast_to(v0, v.shape), rtol=0, atol=2e-4)
    x = g.sync_particle_state_to_cpu().astype(np.float64)
    np.testing.assert_allclose(x - x0, np.broadcast_to(v0.astype(np.float64) * n * DT, x.shape), rtol=0, atol=2e-5)
    assert abs(float(v.astype(np.float64).mean(0)[0]) - 1.1) < 2e-6   # momentum itself does not drift
    C = g.download(A.AFFINE)
    assert np.abs(C).max() < 0.2           # 1/s; 4/dx * 2e-4 m/s
    F = g.download(A.DEFORMATION_GRADIENTS).reshape(-1, 3, 3)
    # the cloth model keeps F = Q R with the in-plane block of R at rest: columns stay orthonormal
    gram = np.einsum("nij,nik->njk", F, F)
    np.testing.assert_allclose(gram, np.broadcast_to(np.eye(3, dtype=np.float32), gram.shape), rtol=0, atol=2e-3)
