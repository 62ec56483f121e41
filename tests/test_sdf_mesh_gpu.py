"""Mesh colliders on the device (mpm_sdf_shape_from_mesh, mpm_set_sdf_colliders): the lattice against the float64
brute force, the query against the documented interpolant of the downloaded lattice, the pairs against the host rule,
a slab against the half-space it equals, the partitioned world, the refusals, and an engine whose mesh colliders were
cleared against one that never had any.  Float64 reference: tests/sdf_mesh_reference.py."""
import numpy as np
import pytest

from tests import sdf_mesh_reference as ref
from tests.test_contact_pairs_gpu import _rot

pytestmark = pytest.mark.gpu
DT = 1e-3
F = np.float32

MESHES = {"icosphere": (ref.icosphere, 0.005), "box": (lambda: ref.box((0.04, 0.03, 0.02)), 0.005),
          "torus": (ref.torus, 0.004), "slab": (ref.slab, 1.0 / 64)}


def _engine(bits=6, bodies=1, layers=1, res=8, z0=0.5, side=0.1):
    from drake_amd import GpuMpm, scenes
    g = GpuMpm(bits)
    scenes.populate(g, scenes.cloth_stack(layers, res, bits, z0=z0, side=side, seed=3))
    g.reallocate_external_bodies(bodies)
    return g


def _shape(g, name, pad=2):
    make, cell = MESHES[name]
    v, f = make()
    sid = g.sdf_shape_from_mesh(v, f, cell, pad)
    n, lo, c = g.sdf_shape_info(sid)
    return sid, v, f, n, lo, c, g.sdf_shape_download(sid)


# ---- 1. the lattice ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(MESHES))
def test_lattice_matches_the_float64_reference(name):
    g = _engine()
    sid, v, f, n, lo, cell, vals = _shape(g, name)
    n_ref, lo_ref = ref.lattice_layout(v, MESHES[name][1], 2)
    assert np.array_equal(n, n_ref) and np.array_equal(lo, lo_ref) and cell == F(MESHES[name][1]), (n, n_ref, lo, lo_ref)
    assert vals.shape == (n[2], n[1], n[0])
    want = ref.mesh_sdf(ref.lattice_nodes(n, lo, cell).reshape(-1, 3), v, f).reshape(vals.shape)
    ext = ref.mesh_extent(v)
    assert np.abs(vals - want).max() <= 1e-5 * ext, (name, np.abs(vals - want).max(), ext)
    decided = np.abs(want) > 1e-4 * ext
    assert np.array_equal(np.sign(vals[decided]), np.sign(want[decided])), name
    assert np.sum(want < 0) > 0 and np.sum(want > 0) > 0
    # deterministic: a second build is the same to the bit
    assert np.array_equal(_shape(g, name)[-1], vals)


def test_large_mesh_split_over_launches_matches_the_reference():
    """20,480 triangles on a 682k-node lattice: the build runs in several launches along the nodes AND the triangles
    (each node's running minimum and solid-angle sum carried between them); a sample of nodes against the brute force"""
    g = _engine()
    v, f = ref.torus(0.05, 0.02, 160, 64)
    cell = 0.14 / 123
    sid = g.sdf_shape_from_mesh(v, f, cell)
    n, lo, c = g.sdf_shape_info(sid)
    assert np.prod(n.astype(np.int64)) > 2048 * 256 and len(f) > 2 * 7424      # (more bricks and triangles than one launch takes)
    vals = g.sdf_shape_download(sid)
    rng = np.random.default_rng(11)
    idx = rng.choice(vals.size, 1500, replace=False)
    nodes = ref.lattice_nodes(n, lo, c).reshape(-1, 3)[idx]
    want = ref.mesh_sdf(nodes, v, f, chunk=64)
    got = vals.reshape(-1)[idx]
    ext = ref.mesh_extent(v)
    assert np.abs(got - want).max() <= 1e-5 * ext
    decided = np.abs(want) > 1e-4 * ext
    assert np.array_equal(np.sign(got[decided]), np.sign(want[decided]))
    assert np.sum(want < 0) > 20


# ---- 2. the query --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["icosphere", "torus", "box"])
def test_query_matches_the_interpolant_of_the_downloaded_lattice(name):
    from drake_amd import SdfCollider
    g = _engine()
    sid, v, f, n, lo, cell, vals = _shape(g, name)
    hi = lo.astype(np.float64) + (n - 1) * np.float64(cell)
    rng = np.random.default_rng(7)
    span = hi - lo
    inside = lo + rng.random((4000, 3)) * span
    outside = lo - 0.5 * span + rng.random((4000, 3)) * 2 * span
    face = lo + rng.random((600, 3)) * span
    for a in range(3):
        face[a * 200:a * 200 + 100, a] = lo[a]
        face[a * 200 + 100:a * 200 + 200, a] = hi[a]
    xb = np.concatenate([inside, outside, face])
    for R, p in ((np.eye(3), (0.5, 0.5, 0.5)), (_rot((1, 2, 3), 0.9), (0.3, 0.6, 0.45)), (_rot((0, 1, 0), 2.5), (0.7, 0.4, 0.5))):
        col = SdfCollider(sid, p_WB=p, R_WB=R, v=(0.1, 0, 0), w=(0, 1.0, 0))
        Rf = np.array(col.R_WB[:], F).astype(np.float64).reshape(3, 3)
        x = (xb @ Rf.T + np.array(col.p_WB[:], F)).astype(F)
        phi, grad = g.sdf_collider_signed_distance(col, x)
        phi_h, grad_h, t = ref.world_sdf(vals, n, lo, cell, col, x)
        ext = float(span.max())
        # (float32 body coordinates: a rounding of the point, |grad phi| <= ~1 times it)
        assert np.abs(phi - phi_h).max() < 2e-6 * max(1.0, ext), (name, np.abs(phi - phi_h).max())
        np.testing.assert_allclose(np.linalg.norm(grad, axis=1), 1.0, atol=1e-5)
        # the gradient jumps across cell faces and at the box: compare away from them
        frac = np.abs(t - np.round(t)).min(1)
        xbh = (x.astype(np.float64) - np.array(col.p_WB[:], F)) @ Rf
        gap = np.linalg.norm(np.clip(xbh, lo, hi) - xbh, axis=1)            # outside the box
        depth = np.minimum(xbh - lo, hi - xbh).min(1)                          # inside it
        smooth = (gap > 1e-5) | ((depth > 1e-5) & (frac > 1e-3))
        assert smooth.sum() > 0.7 * len(x)
        assert np.abs(grad[smooth] - grad_h[smooth]).max() < 1e-3, (name, np.abs(grad[smooth] - grad_h[smooth]).max())


# ---- 3. the pairs --------------------------------------------------------------------------------------------------------

PHI_BAND = 2e-6   # |phi_host| below it: the float32 pose and coordinates may decide either way


def _mesh_scene(g):
    from drake_amd import SdfCollider
    shapes = {name: _shape(g, name) for name in ("icosphere", "torus", "box")}
    mesh = [SdfCollider(shapes["icosphere"][0], body=0, p_WB=(0.42, 0.5, 0.52), R_WB=_rot((1, 2, 0), 0.4), v=(0, 0, -0.2),
                        w=(0, 1.0, 0)),
            SdfCollider(shapes["torus"][0], body=0, p_WB=(0.58, 0.48, 0.5), R_WB=_rot((1, 0, 0), 0.3), w=(0, 0, 2.0)),
            SdfCollider(shapes["box"][0], body=0, p_WB=(0.5, 0.6, 0.5), R_WB=_rot((0, 1, 1), 0.7), v=(0.1, 0.1, 0))]
    return shapes, mesh


@pytest.mark.parametrize("n_analytic", [14, 17])
def test_pairs_with_analytic_and_mesh_colliders_match_the_host_rule(n_analytic):
    from drake_amd import Collider, GpuMpm, scenes
    from tests.test_collider_shapes_gpu import world_sdf as analytic_sdf
    g = GpuMpm(7)
    scenes.populate(g, scenes.cloth_stack(4, 60, 7, z0=0.49, vel_amp=0.2))
    n_all = n_analytic + 3
    g.reallocate_external_bodies(n_all)
    g.run_substeps(3, DT, -1)
    g.rebuild_mapping(True)
    rng = np.random.default_rng(5)
    cols = [Collider(0, body=0, p_WB=(0.5, 0.5, 0.492), R_WB=_rot((1, 0, 0), 0.05))]
    for j in range(1, n_analytic):
        x, y = 0.3 + 0.4 * rng.random(), 0.3 + 0.4 * rng.random()
        if j % 2:
            cols.append(Collider(2, body=j, p_WB=(x, y, 0.5), R_WB=_rot(rng.normal(size=3), 1.0), dims=(0.02, 0.015, 0.01),
                                 v=(0.1, 0, 0)))
        else:
            cols.append(Collider(1, body=j, p_WB=(x, y, 0.5), dims=(0.02, 0, 0), w=(0, 0, 1.0)))
    shapes, mesh = _mesh_scene(g)
    for m, c in enumerate(mesh):
        c.body = n_analytic + m                 # (the body names the collider)
    g.set_sdf_colliders(mesh)
    n = g.generate_contact_pairs(cols)
    pos = g.sync_particle_state_to_cpu()
    got = g.download_contact_pairs()
    assert n == got[0].size and n > 1000
    per, rows, amb = [], [], set()
    for j, c in enumerate(cols):
        per.append(analytic_sdf(c, pos))
    names = ("icosphere", "torus", "box")
    for m, c in enumerate(mesh):
        _, _, _, ns, los, cell, vals = shapes[names[m]]
        phi, gw, _ = ref.world_sdf(vals, ns, los, cell, c, pos)
        per.append((phi, gw))
    for j, (phi, _) in enumerate(per):
        s = np.nonzero(phi < 0)[0]
        rows.append(np.stack([s, np.full_like(s, j)], 1))
        amb |= {(int(k), j) for k in np.nonzero(np.abs(phi) <= PHI_BAND)[0]}
    order = np.concatenate(rows)
    order = order[np.lexsort((order[:, 1], order[:, 0]))]
    gk = [(int(a), int(b)) for a, b in zip(got[0], got[1])]
    want = [(int(a), int(b)) for a, b in order]
    # the same pairs in the same order, but for the undecidable ones -- counted
    assert [k for k in gk if k not in amb] == [k for k in want if k not in amb]
    n_amb = len(set(gk) ^ set(want))
    assert n_amb <= max(5, n // 1000), n_amb
    for m in range(3):                         # every mesh collider took part
        assert np.sum(got[1] == n_analytic + m) > 50, m
    ids = got[0].astype(np.int64) * 64 + got[1]
    assert np.all(np.diff(ids) > 0)
    assert np.all(got[2] < 0)
    decided = np.array([k not in amb for k in gk])
    mesh_pair = got[1] >= n_analytic
    phi_ref = np.array([per[b][0][a] for a, b in gk])
    nrm_ref = np.array([-per[b][1][a] for a, b in gk])
    sel = decided & mesh_pair
    assert np.abs(got[2][sel] - phi_ref[sel]).max() < PHI_BAND
    nd = np.abs(got[3][mesh_pair] - nrm_ref[mesh_pair]).max(1)
    assert np.mean(nd > 1e-3) < 5e-3             # (the gradient jumps across cell faces)
    np.testing.assert_array_equal(got[4], pos[got[0]])
    allc = cols + mesh
    for k in np.nonzero(mesh_pair)[0][::13]:
        a, b = gk[k]
        c = allc[b]
        np.testing.assert_allclose(got[5][k], ref.rigid_v(c, pos[a]), atol=1e-6)
        np.testing.assert_array_equal(got[6][k], np.array(c.p_WB[:], F))


# ---- 4. a slab is the half-space at its top face ------------------------------------------------------------------------

def test_slab_mesh_equals_the_half_space_at_its_top_face():
    """Inside the slab near its top face the lattice is z_B to the bit (dyadic corners and cell: the nodes' distances are
    exact), and trilinear interpolation of a linear field is exact up to the rounding of (q - lo) / cell: phi differs
    from the half-space's z_B by at most half an ulp of |lo_z| = 0.14 (7.5e-9) plus the final rounding.  Coordinates near
    z = 0.5 are multiples of 3e-8, so every particle is a pair of both or of neither, the normals are (0, 0, 1) in both,
    and only dist differs (<= 1e-8).  Tolerances of the run, fixed before it: those of the in-process world against the
    single engine (tests/test_team_gpu.py), a perturbation of the same order -- positions 1e-5 of the domain, velocities
    the solver's stopping tolerance, per-body impulses IMPULSE_RTOL, Newton iterations within max(1, its / 8)."""
    from drake_amd import Collider, SdfCollider, scenes
    from tests.helpers import IMPULSE_RTOL, close, solve_tolerance
    from tests.test_contact_noroundtrip_gpu import DT as CDT, D, K, MU, _engine as det_engine, _state
    sheets = scenes.cloth_stack(1, 36, 6, z0=0.5 + 0.006, side=0.3, seed=9, vel_amp=0.02)
    for pos, vel, idx in sheets:
        vel[:, 2] -= 1.0
    floor = [Collider(0, body=0, p_WB=(0.5, 0.5, 0.5))]
    a, b = det_engine(None, sheets), det_engine(None, sheets)
    v, f = ref.slab()
    sid = b.sdf_shape_from_mesh(v, f, 1.0 / 128, 2)
    b.set_sdf_colliders([SdfCollider(sid, body=0, p_WB=(0.5, 0.5, 0.5))])
    n = 90
    ra = a.run_coupled_substeps(n, CDT, floor, MU, K, D)
    rb = b.run_coupled_substeps(n, CDT, [], MU, K, D)      # (mesh colliders only: not contact-free)
    a.gpu_sync()
    b.gpu_sync()
    assert a.stats()["error_flags"] == 0 and b.stats()["error_flags"] == 0
    first = next(i for i, r in enumerate(ra) if r["contacts"] > 0)
    assert 5 < first < n - 20 and max(r["contacts"] for r in ra) > 300, first
    # up to the first contact substep the states are the same to the bit, so are its pairs
    assert [r["contacts"] for r in ra[:first + 1]] == [r["contacts"] for r in rb[:first + 1]]
    for s in range(n):
        ia, ib = ra[s]["iterations"], rb[s]["iterations"]
        assert abs(ia - ib) <= max(1, ia // 8), (s, ra[s], rb[s])
    assert b.contact_counters()["contact_free"] >= first // 2     # the watch decided those substeps
    sa, sb = _state(a), _state(b)
    dofs = max(a.contact_stats()["dofs"], 1)
    close(sb["pos"], sa["pos"], scale=1.0, rtol=1e-5, what="slab vs half-space: positions")
    close(sb["vel"], sa["vel"], scale=1.0, rtol=solve_tolerance(dofs), what="slab vs half-space: velocities")
    fs = float(np.abs(sa["f"]).max())
    assert fs > 0
    close(sb["f"], sa["f"], scale=fs, rtol=IMPULSE_RTOL, what="slab vs half-space: impulse")
    close(sb["tau"], sa["tau"], scale=max(float(np.abs(sa["tau"]).max()), fs), rtol=IMPULSE_RTOL,
          what="slab vs half-space: angular impulse")


def test_slab_pairs_equal_the_half_space_pairs():
    from drake_amd import Collider, SdfCollider, scenes
    from tests.test_contact_noroundtrip_gpu import _engine as det_engine
    sheets = scenes.cloth_stack(2, 36, 6, z0=0.5 - 0.004, side=0.3, seed=9, vel_amp=0.02)
    g = det_engine(None, sheets)
    g.rebuild_mapping(True)
    v, f = ref.slab()
    sid = g.sdf_shape_from_mesh(v, f, 1.0 / 128, 2)
    half = g.generate_contact_pairs([Collider(0, body=0, p_WB=(0.5, 0.5, 0.5), v=(0, 0.2, 0.1))])
    pa = g.download_contact_pairs()
    g.set_sdf_colliders([SdfCollider(sid, body=0, p_WB=(0.5, 0.5, 0.5), v=(0, 0.2, 0.1))])
    mesh = g.generate_contact_pairs([])
    pb = g.download_contact_pairs()
    assert half == mesh and half > 300
    for k in (0, 1, 3, 4, 5, 6):
        np.testing.assert_array_equal(pa[k], pb[k], err_msg=str(k))
    assert np.abs(pa[2] - pb[2]).max() <= 1e-8


# ---- 5. the partitioned world --------------------------------------------------------------------------------------------

def _team_mesh(t, shape_ids):
    from drake_amd import SdfCollider
    from tests.test_team_gpu import FLOOR_Z
    return [SdfCollider(shape_ids[0], body=1, p_WB=(0.485 + 2.0 * t, 0.5, FLOOR_Z + 0.04), v=(2.0, 0, 0)),
            SdfCollider(shape_ids[1], body=2, p_WB=(0.64 - 1.5 * t, 0.5, FLOOR_Z + 0.012), R_WB=_rot((0, 0, 1), 0.3),
                        v=(-1.5, 0, 0), w=(0, 0, 0.5))]


def _team_shapes(g):
    v, f = ref.icosphere(0.045)
    a = g.sdf_shape_from_mesh(v, f, 0.005, 2)
    v, f = ref.torus(0.05, 0.015)
    b = g.sdf_shape_from_mesh(v, f, 0.004, 2)
    return a, b


def test_in_process_world_with_mesh_colliders_matches_single_engine():
    import torch
    from drake_amd import ARR, Collider
    from drake_amd.dist import LocalWorld
    from tests.test_team_gpu import CHUNKS, D, DT as TDT, FLOOR_Z, K, MU, _check_against_single_engine, \
        _engine as team_engine, _scene
    floor = [Collider(0, body=0, p_WB=(0.5, 0.5, FLOOR_Z))]
    sheets = _scene()
    g = team_engine(sheets)
    ids = _team_shapes(g)
    res, logs, done = [], [], 0
    for k in CHUNKS:
        g.set_sdf_colliders(_team_mesh(done * TDT, ids))
        res += g.run_coupled_substeps(k, TDT, floor, MU, K, D)
        done += k
        logs.append(g.contact_log().copy())
    g.gpu_sync()
    assert g.stats()["error_flags"] == 0
    tau, f = g.external_body_force_to_host()
    ref_run = dict(res=res, logs=logs, pos=g.download(ARR.POSITIONS), vel=g.download(ARR.VELOCITIES), tau=tau, f=f,
                   dofs=g.contact_stats()["dofs"], n=g.n_particles)
    world = 2
    engines = [team_engine(sheets) for _ in range(world)]
    eids = [_team_shapes(e) for e in engines]
    w = LocalWorld(engines, [0, 8, 16], zone_blocks=2, ghost_cells=0, ghost_margin_cells=0, capacity_blocks=512,
                   migrate_every=0, migrate_capacity=1 << 14, device=torch.device("cuda", 0))
    w.enable_team(512)
    res = [[] for _ in range(world)]
    logs = [[] for _ in range(world)]
    done = 0
    for k in CHUNKS:
        for e, i in zip(engines, eids):
            e.set_sdf_colliders(_team_mesh(done * TDT, i))
        out = w.coupled_substeps(k, TDT, floor, MU, K, D)
        done += k
        for r in range(world):
            res[r] += out[r]
            logs[r].append(engines[r].contact_log().copy())
    w.sync()
    n = ref_run["n"]
    owned = np.zeros(n, np.int32)
    pos, vel = np.full((n, 3), np.nan, np.float32), np.full((n, 3), np.nan, np.float32)
    f_sum, tau_sum = np.zeros_like(ref_run["f"]), np.zeros_like(ref_run["tau"])
    for e in engines:
        assert e.stats()["error_flags"] == 0
        own = e.dist_roles() == 1
        owned += own
        pos[own], vel[own] = e.download(ARR.POSITIONS)[own], e.download(ARR.VELOCITIES)[own]
        tau, f = e.external_body_force_to_host()
        f_sum += f
        tau_sum += tau
    _check_against_single_engine(ref_run, res, logs, owned, pos, vel, f_sum, tau_sum, "world of 2, mesh colliders")


# ---- 6. refusals, and a cleared set changes nothing ---------------------------------------------------------------------

def test_refusals_leave_nothing_enqueued():
    from drake_amd import Collider, MpmError, SdfCollider, scenes, GpuMpm
    g = GpuMpm(6)
    scenes.populate(g, scenes.cloth_stack(1, 24, 6, z0=0.5 - 0.002, side=0.2, seed=1, vel_amp=0.0))
    g.reallocate_external_bodies(1)
    g.rebuild_mapping(False)
    v, f = ref.box((0.04, 0.03, 0.02))
    nan = float("nan")
    bad_v = v.copy()
    bad_v[3, 1] = nan
    bad_calls = [
        lambda: g.sdf_shape_from_mesh(v, np.where(f == 5, 8, f), 0.005),          # index out of range
        lambda: g.sdf_shape_from_mesh(v, np.where(f == 5, -1, f), 0.005),
        lambda: g.sdf_shape_from_mesh(bad_v, f, 0.005),                           # non-finite vertex
        lambda: g.sdf_shape_from_mesh(v, np.zeros((0, 3), np.int32), 0.005),      # no triangles
        lambda: g.sdf_shape_from_mesh(v, f, 0.0), lambda: g.sdf_shape_from_mesh(v, f, -0.01),
        lambda: g.sdf_shape_from_mesh(v, f, nan), lambda: g.sdf_shape_from_mesh(v, f, float("inf")),
        lambda: g.sdf_shape_from_mesh(v, f, 0.005, pad_cells=1),
        lambda: g.sdf_shape_from_mesh(v, f, 0.0001),                              # > 2^24 nodes
        lambda: g.sdf_shape_from_mesh(v, np.zeros(((1 << 21) + 1, 3), np.int32), 0.005),   # > 2^21 triangles
        lambda: g.set_sdf_colliders([SdfCollider(0)]),                            # no shape yet
    ]
    for call in bad_calls:
        with pytest.raises(MpmError) as e:
            call()
        assert e.value.code == -1
    sid = g.sdf_shape_from_mesh(v, f, 0.005)
    assert sid == 0
    with pytest.raises(MpmError) as e:
        g.set_sdf_colliders([SdfCollider(sid + 1)])
    assert e.value.code == -1
    with pytest.raises(MpmError) as e:
        g.sdf_collider_signed_distance(SdfCollider(7), np.zeros((2, 3), F))
    assert e.value.code == -1
    # a body out of range: refused by the generating calls, before anything is enqueued
    g.set_sdf_colliders([SdfCollider(sid, body=1, p_WB=(0.5, 0.5, 0.5))])
    good = [Collider(0, p_WB=(0.5, 0.5, 0.5))]
    for call in (lambda: g.generate_contact_pairs(good), lambda: g.generate_contact_pairs([]),
                 lambda: g.run_coupled_substeps(2, DT, good, 0.5, 1e5, 1e-3),
                 lambda: g.run_coupled_substeps(2, DT, [], 0.5, 1e5, 1e-3)):
        with pytest.raises(MpmError) as e:
            call()
        assert e.value.code == -1
        assert g.contact_pair_count() == 0
    assert g.stats()["substeps"] == 0
    # the next valid call solves normally
    g.set_sdf_colliders([SdfCollider(sid, body=0, p_WB=(0.5, 0.5, 0.5))])
    g.rebuild_mapping(False)
    g.calc_fem_state_and_force(DT)
    g.particle_to_grid(DT)
    g.update_grid(-1)
    n_good = g.generate_contact_pairs(good)
    assert n_good > 0 and g.download_contact_pairs()[1].size == n_good
    r = g.update_contact(DT, 0.5, 1e5, 1e-3)
    assert r["iterations"] >= 1 and g.stats()["error_flags"] == 0


def test_cleared_mesh_colliders_leave_no_trace():
    """b poses mesh colliders that cut the cloth, makes pairs with them, clears them; c leaves them in place.  c must
    diverge from a (the set matters), b must equal a to the bit (the clear leaves nothing behind)."""
    from drake_amd import Collider, SdfCollider, scenes
    from tests.test_contact_noroundtrip_gpu import DT as CDT, D, K, MU, _engine as det_engine, _same, _same_rows, _state
    sheets = scenes.cloth_stack(1, 36, 6, z0=0.5 + 0.006, side=0.3, seed=9, vel_amp=0.02)
    for pos, vel, idx in sheets:
        vel[:, 2] -= 1.0
    floor = [Collider(0, body=0, p_WB=(0.5, 0.5, 0.5))]
    a, b, c = det_engine(None, sheets), det_engine(None, sheets), det_engine(None, sheets)
    v, f = ref.torus()
    for e in (b, c):
        sid = e.sdf_shape_from_mesh(v, f, 0.004)
        # one torus whose tube holds the sheet, 19 more out of reach (a table of 20)
        cutting = [SdfCollider(sid, body=0, p_WB=(0.5, 0.5, 0.506), w=(0, 0, 1.0))] + \
            [SdfCollider(sid, body=0, p_WB=(0.5, 0.5, 0.3))] * 19
        e.set_sdf_colliders(cutting)
    for e in (a, b, c):
        e.rebuild_mapping(True)
    n_a = a.generate_contact_pairs(floor)
    n_b = b.generate_contact_pairs(floor)
    assert n_b > n_a + 100, (n_a, n_b)                                      # (the torus is in reach)
    b.set_sdf_colliders([])
    c.generate_contact_pairs(floor)
    ra = a.run_coupled_substeps(60, CDT, floor, MU, K, D)
    rb = b.run_coupled_substeps(60, CDT, floor, MU, K, D)
    rc = c.run_coupled_substeps(60, CDT, floor, MU, K, D)
    for e in (a, b, c):
        e.gpu_sync()
    assert max(r["contacts"] for r in ra) > 100
    assert rc[0]["contacts"] > ra[0]["contacts"] + 100                      # (left in place, the set makes pairs ...)
    assert not np.array_equal(_state(a)["pos"], _state(c)["pos"])          # (... and changes the motion)
    _same_rows(ra, rb, "iterations", "contacts", "residual")
    _same(_state(a), _state(b))
