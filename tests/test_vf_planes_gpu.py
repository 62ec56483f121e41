"""How many planes of the vertex-side force records (DP::VF) the kernels that sum a vertex's force read is a property of
the launched instance: six where no vertex of any cloth of the engine has more than six faces, eight otherwise
(vf_planes_of, mpm_device.h; launch_p2g and launch_fem_vertices pick the instance from the largest valence mpm_finalize
found), and a vertex with more than eight faces walks the adjacency.  Four small scenes reach all of it:

  regular      a sheet of 12 x 12 vertices, one diagonal direction: valence <= 6, the six-plane instances
  alternating  the same sheet with alternating diagonals: valences 4 and 8, the eight-plane instances
  fan          ten triangles around a hub: the mark in plane 0 and the walk over the adjacency (k_vforce)
  mixed        the regular sheet and, six blocks away, a patch of 3 x 3 vertices with alternating diagonals: the whole
               engine reads eight planes

What is asserted:
* `regular` and the sheet of `mixed` follow the same trajectory to the bit in deterministic mode -- through
  mpm_run_substeps (the vertex forces summed inside k_p2g) and through the phase calls (k_vforce), whose downloaded
  vertex forces agree too.  Nothing couples the two cloths of `mixed`: they share no grid block, and the patch is light
  enough to leave the fixed-point scale of the node sums (a power of two from the total mass) where it was, which the
  test checks on the scenes it builds.
* the vertex forces mpm_calc_fem_state_and_force leaves are, bit for bit, the float32 sum of the faces' per-corner records
  in ascending face id.  The records come from a second engine with the same faces in the same order, every face on
  three vertices of its own ("soup": a vertex with one face has 0 + (-record) as its force).
* two ranks of the regular sheet, sliding across the cut, stay equal to a single engine at the tolerance of
  tests/test_world_gpu.py.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BITS = 6
DX = 1.0 / (1 << BITS)
DT = 5e-4
RES = 12
SIDE = RES * 0.44 * DX   # the benchmark's lattice: 0.44 cells between vertices


def _alternating_indices(res, phase=0):
    """two triangles per quad, the diagonal flipped from one quad to the next: an inner vertex (i, j) has 4 faces where
    i + j + phase is even and 8 where it is odd"""
    tri = []
    for i in range(res - 1):
        for j in range(res - 1):
            a, b, c, d = i * res + j, (i + 1) * res + j, i * res + j + 1, (i + 1) * res + j + 1
            tri += [a, b, c, d, c, b] if (i + j + phase) % 2 == 0 else [a, b, d, a, d, c]
    return np.asarray(tri, np.int32)


def _sheet(res, side, centre, z, seed, alternating=False, vx=0.0, phase=0):
    """-> (pos, vel, idx): a jittered lattice with hashed velocities of 0.3 m/s (drake_amd.scenes), moving at vx along x"""
    from drake_amd import scenes
    pos, idx = scenes.cloth_sheet(res, side, z, centre)
    n = len(pos)
    jit = np.stack([scenes.hash_uniform(seed, n, c) for c in range(3)], -1)
    vel = np.stack([scenes.hash_uniform(seed, n, 3 + c) for c in range(3)], -1)
    pos = (pos + np.float32(0.05 * side / res) * jit).astype(np.float32)
    vel = (np.float32(0.3) * vel).astype(np.float32)
    vel[:, 0] += np.float32(vx)
    return pos, vel, (_alternating_indices(res, phase) if alternating else idx)


def _fan(n_rim=10):
    from tests.test_parity_gpu import _fan_sheet
    return _fan_sheet(n_rim, 0.9 * DX, (0.5, 0.5), 0.5, 5)


def _regular(vx=0.0, centre=(0.3, 0.5)):
    return _sheet(RES, SIDE, centre, 0.5, 21, vx=vx)


def _patch(vx=0.0):
    return _sheet(3, 3 * 0.44 * DX, (0.7, 0.5), 0.5, 22, alternating=True, vx=vx, phase=1)   # (its middle vertex has 8 faces)


def _valence(idx):
    return int(np.bincount(idx).max())


def _engine(sheets, deterministic=True):
    from drake_amd import GpuMpm, scenes
    g = GpuMpm(BITS)
    if deterministic:
        g.set_deterministic(True)
    scenes.populate(g, [(p.copy(), v.copy(), i.copy()) for p, v, i in sheets])
    return g


def _by_id(g, which):
    """an array of the engine by original particle id ([faces | vertices] of the cloths in order), as uint32 words"""
    from drake_amd import ARR
    a = g.download(which)
    out = np.empty_like(a)
    out[g.download(ARR.PIDS)] = a
    return np.ascontiguousarray(out).view(np.uint32)


def _sheet_ids(nf_engine):
    """original ids of the regular sheet's particles in an engine with nf_engine faces whose first cloth it is"""
    nf = 2 * (RES - 1) ** 2
    return np.concatenate([np.arange(nf), nf_engine + np.arange(RES * RES)])


def _total_mass_exponent(g):
    from drake_amd import ARR, GpuMpm
    m = float(np.abs(g.download(ARR.VOLUMES).astype(np.float64)).sum()) * float(GpuMpm.default_material().density)
    return int(np.ceil(np.log2(m)))


def test_scenes_reach_both_instances_and_the_walk():
    """the valences the four scenes are built for (what mpm_finalize finds in its adjacency)"""
    assert _valence(_regular()[2]) == 6
    alt = np.bincount(_sheet(RES, SIDE, (0.3, 0.5), 0.5, 21, alternating=True)[2])
    assert alt.max() == 8 and set(alt.reshape(RES, RES)[1:-1, 1:-1].reshape(-1)) == {4, 8}
    assert _valence(_fan()[2]) == 10
    assert _valence(_patch()[2]) == 8 and abs(0.7 - 0.3) / (4 * DX) > 3 + SIDE / (4 * DX)


def _pair():
    """`regular` alone (six planes) and `mixed` (eight), both deterministic, with the same fixed-point scale"""
    a, b = _engine([_regular(vx=2.0)]), _engine([_regular(vx=2.0), _patch(vx=2.0)])
    assert _total_mass_exponent(a) == _total_mass_exponent(b)   # (the scale of the node sums: 2^(61 - this))
    return a, b


def _assert_sheet_equal(a, b, what):
    from drake_amd import ARR
    ia, ib = _sheet_ids(a.n_faces), _sheet_ids(b.n_faces)
    for name, arr in (("pos", ARR.POSITIONS), ("vel", ARR.VELOCITIES), ("C", ARR.AFFINE)):
        xa, xb = _by_id(a, arr)[ia], _by_id(b, arr)[ib]
        assert xa.size and np.array_equal(xa, xb), (what, name, int((xa != xb).sum()))
    Fa, Fb = a.download(ARR.DEFORMATION_GRADIENTS).view(np.uint32), b.download(ARR.DEFORMATION_GRADIENTS).view(np.uint32)
    assert np.array_equal(Fa, Fb[:len(Fa)]), (what, "F")


def test_regular_sheet_is_the_same_with_six_planes_and_with_eight_batched():
    """mpm_run_substeps: k_p2g<1, 1, 0, 6> against k_p2g<1, 1, 0, 8>, a re-sort on the way (2 m/s: a cell in 16 substeps)"""
    a, b = _pair()
    x0 = _by_id(a, 0).copy()
    for g in (a, b):
        g.run_substeps(4, DT, -1)
        g.run_substeps(8, DT, -1)
        g.gpu_sync()
        assert g.stats()["error_flags"] == 0
    _assert_sheet_equal(a, b, "run_substeps")
    assert not np.array_equal(_by_id(a, 0), x0)
    a.destroy(), b.destroy()


def test_regular_sheet_is_the_same_with_six_planes_and_with_eight_phase_calls():
    """the phase calls: k_vforce<6> against k_vforce<8>; the forces of the second substep (the first starts at rest)"""
    from drake_amd import ARR
    a, b = _pair()
    forces = []
    for g in (a, b):
        for k in range(2):
            g.rebuild_mapping(False)
            g.calc_fem_state_and_force(DT)
            if k == 1:
                forces.append(_by_id(g, ARR.FORCES)[_sheet_ids(g.n_faces)])
            g.particle_to_grid(DT)
            g.update_grid(-1)
            g.grid_to_particle(DT)
        g.gpu_sync()
        assert g.stats()["error_flags"] == 0
    nf = 2 * (RES - 1) ** 2
    assert forces[0][nf:].view(np.float32).any()
    assert np.array_equal(forces[0], forces[1]), int((forces[0] != forces[1]).sum())
    _assert_sheet_equal(a, b, "phase calls")
    a.destroy(), b.destroy()


def _soup(sheet):
    """the faces of `sheet` in order, each on three vertices of its own (vertex 3 f + c = corner c of face f)"""
    pos, vel, idx = sheet
    return pos[idx].copy(), vel[idx].copy(), np.arange(len(idx), dtype=np.int32)


def _forces_of_displaced(sheet, shift_of_vertex):
    """vertex forces by original vertex id after mpm_calc_fem_state_and_force on the mesh at rest with every vertex moved
    by its row of `shift_of_vertex` (the faces' centroids are CalcFemStateAndForce's own to write)"""
    from drake_amd import ARR
    g = _engine([sheet])
    nf = g.n_faces
    pid = g.download(ARR.PIDS)
    x = g.download(ARR.POSITIONS)
    vert = pid >= nf
    x[vert] = x[vert] + shift_of_vertex[pid[vert] - nf]
    g.upload_particle_state(x, None)
    g.rebuild_mapping(False)
    g.calc_fem_state_and_force(DT)
    g.gpu_sync()
    assert g.stats()["error_flags"] == 0
    f = np.empty((g.n_particles, 3), np.float32)
    f[pid] = g.download(ARR.FORCES)
    g.destroy()
    return f[nf:]


@pytest.mark.parametrize("scene", ["regular", "alternating", "fan"])
def test_vertex_forces_are_the_float32_sum_of_the_corner_records_in_face_order(scene):
    sheet = {"regular": lambda: _regular(), "fan": _fan,
             "alternating": lambda: _sheet(RES, SIDE, (0.3, 0.5), 0.5, 21, alternating=True)}[scene]()
    idx = sheet[2]
    nv = len(sheet[0])
    assert _valence(idx) == {"regular": 6, "alternating": 8, "fan": 10}[scene]
    rng = np.random.default_rng(7)
    shift = (0.05 * DX * rng.standard_normal((nv, 3))).astype(np.float32)
    f = _forces_of_displaced(sheet, shift)
    rec = _forces_of_displaced(_soup(sheet), shift[idx])   # row 3 f + c: 0 + (-record of corner c of face f)
    want = np.zeros((nv, 3), np.float32)
    for k, v in enumerate(idx):                            # ascending face id; a face has a vertex once
        want[v] = want[v] + rec[k]
    assert np.abs(want).max() > 0 and want.dtype == np.float32
    bad = f.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), (scene, int(bad.sum()), float(np.abs(f - want).max()))


def test_two_ranks_of_the_regular_sheet_match_a_single_engine():
    """a partitioned engine takes the same instance as a single one: the sheet slides across the cut between two ranks
    (0.19 cells per substep, vertices migrate with their face ids), against a single engine"""
    from drake_amd import ARR, GpuMpm
    from tests.helpers import close
    from tests.test_world_gpu import DT as WDT, _collect, _populate, _run_world
    steps = 16
    sheets = [_regular(vx=3.0, centre=(0.48, 0.5))]
    ref = _populate(GpuMpm(BITS), sheets)
    ref.run_substeps(steps, WDT, -1)
    ref.gpu_sync()
    assert ref.stats()["error_flags"] == 0
    rp, rv, rF = ref.download(ARR.POSITIONS), ref.download(ARR.VELOCITIES), ref.download(ARR.DEFORMATION_GRADIENTS)
    n, nf = ref.n_particles, ref.n_faces
    geo = dict(cuts=[0, 8, 16], zone_blocks=2, ghost_cells=0, ghost_margin_cells=0, migrate_every=0)
    roles0, w = _run_world(BITS, sheets, geo, steps, capacity_blocks=512, migrate_capacity=8192)
    pos, vel, F, per_rank = _collect(w, roles0, n, nf)
    owned0 = [int(np.count_nonzero(r == 1)) for r in roles0]
    owned1 = [int(np.count_nonzero(pr[0] == 1)) for pr in per_rank]
    assert owned1[1] > owned0[1] and w.migrations >= 1, (owned0, owned1, w.migrations)
    vs = max(float(np.abs(rv).max()), 1.0)
    close(pos, rp, scale=1.0, rtol=1e-5, what="two ranks, six planes: positions vs single engine")
    close(vel, rv, scale=vs, rtol=1e-4, what="two ranks, six planes: velocities vs single engine")
    close(F, rF, scale=1.0, rtol=1e-4, what="two ranks, six planes: F vs single engine")
    ref.destroy()
