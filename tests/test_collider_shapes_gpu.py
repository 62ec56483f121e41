"""Cylinder (kind 4) and ellipsoid (kind 5) colliders: mpm_collider_signed_distance against float64 restatements written
from Drake's conventions (distance_to_point_callback.cc: the cylinder's (r, z) cross-section box) and from D. Eberly,
"Distance from a Point to an Ellipse, an Ellipsoid, or a Hyperellipsoid" (the ellipsoid); the pairs made on the device
against a host loop; the table, coupled, oracle and team paths; the refusals."""
import numpy as np
import pytest

from tests.helpers import IMPULSE_RTOL
from tests.pair_layouts import CYL_TOL, sdf_cylinder, sdf_ellipsoid
from tests.test_contact_pairs_gpu import _rot, sdf as sdf_0123

pytestmark = pytest.mark.gpu
DT = 1e-3
F = np.float32


def world_sdf(c, pos):
    """phi and world gradient of collider c at world points pos, from the float32 pose (float64 arithmetic for the new
    kinds, the float32 restatement of tests/test_contact_pairs_gpu.py for kinds 0-3)."""
    R = np.array(c.R_WB[:], F).reshape(3, 3)
    p = np.array(c.p_WB[:], F)
    if c.kind <= 3:
        xb = ((pos.astype(F) - p) @ R).astype(F)
        phi, gb = sdf_0123(c.kind, xb, c.dims[:])
        return phi.astype(np.float64), (gb @ R.T).astype(np.float64)
    xb = (np.asarray(pos, np.float64) - p.astype(np.float64)) @ R.astype(np.float64)
    phi, gb = sdf_cylinder(xb, c.dims[0], c.dims[1]) if c.kind == 4 else sdf_ellipsoid(xb, c.dims[:])
    return phi, gb @ R.T.astype(np.float64)


def _engine(bits=6, bodies=1):
    from drake_amd import GpuMpm, scenes
    g = GpuMpm(bits)
    scenes.populate(g, scenes.cloth_stack(1, 8, bits, z0=0.5, side=0.1, seed=3))
    g.reallocate_external_bodies(bodies)
    return g


def _axis_angle_R(axis, angle):
    return _rot(axis, angle).astype(np.float64)


# ---- 1. ellipsoid: the reference's known answers -------------------------------------------------------------------

def test_ellipsoid_known_answers_of_the_reference():
    from drake_amd import Collider
    g = _engine()
    Rd = _axis_angle_R((1, 2, 3), np.pi / 5)
    p = np.array([0.5, 1.25, -2.0])
    a, b, c = 1.5, 0.75, 1.25
    col = Collider(5, p_WB=p, R_WB=Rd, dims=(a, b, c))
    R = np.array(col.R_WB[:], np.float64).reshape(3, 3)
    pts, want_d, want_n = [], [], []
    for th, ph in ((0, 0), (7 * np.pi / 5, np.pi / 6), (3 * np.pi / 7, 4 * np.pi / 5)):
        N = np.array([a * np.cos(th) * np.sin(ph), b * np.sin(th) * np.sin(ph), c * np.cos(ph)])
        n = N / np.array([a, b, c]) ** 2
        n /= np.linalg.norm(n)
        for d in (-0.125, 0.0, 0.2):
            pts.append(R @ (N + n * d) + p)
            want_d.append(d)
            want_n.append(R @ n)
    phi, grad = g.collider_signed_distance(col, np.array(pts))
    np.testing.assert_allclose(phi, want_d, atol=2e-5)
    np.testing.assert_allclose(grad, np.array(want_n), atol=2e-4)
    # the centre: on the medial set, the nearest points are the ends of the shortest axis (y_B)
    phi, grad = g.collider_signed_distance(col, np.array([col.p_WB[:]]))
    assert abs(phi[0] + 0.75) < 2e-5
    assert np.abs(np.abs(grad[0] @ R[:, 1]) - 1) < 2e-4 and np.abs(grad[0] @ R[:, [0, 2]]).max() < 2e-4


# ---- 2. the query against the restatements, all regions --------------------------------------------------------------

CYLINDERS = [(0.05, 0.3, (1, 2, 0.5), 0.7), (0.3, 0.04, (0.2, 1, 1), 2.1)]                     # slender, squat
ELLIPSOIDS = [(0.3, 0.299, 0.298), (0.4, 0.1, 0.1), (0.3, 0.3, 0.08), (0.5, 0.05, 0.2)]         # near-sphere, prolate, oblate, 10:1


def _cloud(rng, extent, n=100000):
    """points around a shape: a box around it, plus a shell close to the surface is covered by the box's density"""
    return rng.uniform(-1.3, 1.3, size=(n, 3)) * np.asarray(extent)


@pytest.mark.parametrize("shape", range(len(CYLINDERS)))
def test_cylinder_query_matches_the_restatement(shape):
    from drake_amd import Collider
    g = _engine()
    R_, h, axis, ang = CYLINDERS[shape]
    col = Collider(4, p_WB=(0.2, -0.1, 0.3), R_WB=_axis_angle_R(axis, ang), dims=(R_, h, 0))
    R = np.array(col.R_WB[:], np.float64).reshape(3, 3)
    p = np.array(col.p_WB[:], np.float64)
    rng = np.random.default_rng(5 + shape)
    xb = _cloud(rng, (R_, R_, h))
    pts = (xb @ R.T + p).astype(F)
    phi, grad = g.collider_signed_distance(col, pts)
    want_phi, want_grad = world_sdf(col, pts)
    assert np.abs(phi - want_phi).max() < 2e-6
    np.testing.assert_allclose(np.linalg.norm(grad, axis=1), 1.0, atol=1e-5)
    # away from the rims, the axis and the inside's barrel / cap tie (where the nearest feature jumps), and from the
    # thresholds of the boundary class, which float and double coordinates may put on different sides
    q = (np.asarray(pts, np.float64) - p) @ R
    r, az = np.hypot(q[:, 0], q[:, 1]), np.abs(q[:, 2])
    band = 1e-3 * R_
    inside = (r < R_) & (az < h)
    rim = (np.abs(r - R_) < band) & (np.abs(az - h) < band)
    tie = inside & (np.abs((R_ - r) - (h - az)) < band)
    on_axis = inside & (r < band)
    tr, tz = CYL_TOL * max(1.0, R_), CYL_TOL * max(1.0, h)
    undecided = (np.abs(np.abs(r - R_) - tr) < 1e-6) | (np.abs(np.abs(az - h) - tz) < 1e-6)
    ok = ~(rim | tie | on_axis | undecided)
    assert ok.mean() > 0.95 and inside.mean() > 0.1 and (~inside).mean() > 0.1
    assert np.abs(grad[ok] - want_grad[ok]).max() < 1e-4


@pytest.mark.parametrize("shape", range(len(ELLIPSOIDS)))
def test_ellipsoid_query_matches_the_restatement(shape):
    from drake_amd import Collider
    g = _engine()
    radii = ELLIPSOIDS[shape]
    col = Collider(5, p_WB=(-0.1, 0.2, 0.05), R_WB=_axis_angle_R((1, -1, 2), 0.9 + shape), dims=radii)
    R = np.array(col.R_WB[:], np.float64).reshape(3, 3)
    p = np.array(col.p_WB[:], np.float64)
    rng = np.random.default_rng(11 + shape)
    xb = _cloud(rng, radii)
    pts = (xb @ R.T + p).astype(F)
    phi, grad = g.collider_signed_distance(col, pts)
    want_phi, want_grad = world_sdf(col, pts)
    assert np.abs(phi - want_phi).max() < 2e-6
    np.testing.assert_allclose(np.linalg.norm(grad, axis=1), 1.0, atol=1e-5)
    # away from the medial set: inside, near the plane of the shortest axis (the long axis when the two short ones agree)
    q = (np.asarray(pts, np.float64) - p) @ R
    a = np.asarray(radii, np.float64)
    inside = ((q / a) ** 2).sum(1) < 1
    srt = np.argsort(-a)
    band = 1e-3 * a.min()
    if np.isclose(a[srt[1]], a[srt[2]]):
        near = np.hypot(q[:, srt[1]], q[:, srt[2]]) < band
    else:
        near = np.abs(q[:, srt[2]]) < band
    ok = ~(inside & near)
    assert ok.mean() > 0.95 and inside.mean() > 0.1
    assert np.abs(grad[ok] - want_grad[ok]).max() < 1e-4


def test_cylinder_conventions_on_the_axis_and_on_ties():
    from drake_amd import Collider
    g = _engine()
    # on the axis of a rotated squat cylinder, nearer the barrel than a cap: the radial direction is +x_B
    col = Collider(4, p_WB=(0.1, 0.2, 0.3), R_WB=_axis_angle_R((1, 1, 0), 0.8), dims=(0.1, 0.3, 0))
    R = np.array(col.R_WB[:], np.float64).reshape(3, 3)
    pts = np.array([np.array(col.p_WB[:]) + R[:, 2] * z for z in (0.0, 0.05, -0.15)])
    phi, grad = g.collider_signed_distance(col, pts)
    np.testing.assert_allclose(phi, -0.1, atol=2e-6)
    np.testing.assert_allclose(grad, np.broadcast_to(R[:, 0], grad.shape), atol=1e-6)
    # barrel against cap at the same depth (exact in float: identity pose, dyadic coordinates): the barrel wins
    col = Collider(4, dims=(0.5, 0.5, 0))
    phi, grad = g.collider_signed_distance(col, np.array([[0.125, 0, 0.125], [0, -0.25, -0.25], [0, 0.375, 0.375]]))
    np.testing.assert_array_equal(phi, np.array([-0.375, -0.25, -0.125], F))
    np.testing.assert_array_equal(grad, np.array([[1, 0, 0], [0, -1, 0], [0, 1, 0]], F))
    # the centre of a cylinder whose barrel and caps are equally far: the barrel, +x_B; Sign(0) = +1 for the caps
    phi, grad = g.collider_signed_distance(Collider(4, dims=(0.5, 0.5, 0)), np.zeros((1, 3)))
    assert phi[0] == -0.5 and np.array_equal(grad[0], np.array([1, 0, 0], F))
    phi, grad = g.collider_signed_distance(Collider(4, dims=(0.5, 0.25, 0)), np.zeros((1, 3)))
    assert phi[0] == -0.25 and np.array_equal(grad[0], np.array([0, 0, 1], F))


def test_round_ellipsoid_is_the_sphere():
    from drake_amd import Collider
    g = _engine()
    rng = np.random.default_rng(2)
    pts = rng.uniform(-0.5, 0.5, size=(50000, 3)).astype(F)
    ell = Collider(5, p_WB=(0.05, -0.02, 0.01), R_WB=_axis_angle_R((0, 1, 1), 0.3), dims=(0.25, 0.25, 0.25))
    sph = Collider(1, p_WB=(0.05, -0.02, 0.01), dims=(0.25, 0, 0))
    pe, ge = g.collider_signed_distance(ell, pts)
    ps, gs = g.collider_signed_distance(sph, pts)
    assert np.abs(pe - ps).max() < 2e-6
    far = np.linalg.norm(pts - np.array(sph.p_WB[:], F), axis=1) > 1e-2
    assert np.abs(ge[far] - gs[far]).max() < 1e-4


# ---- 3. pairs made on the device against the host loop ---------------------------------------------------------------

def reference_pairs(pos, colliders, tol=2e-6):
    """(slot, collider) with phi < 0 in ascending order, from the restatements; plus the set of the undecidable ones"""
    rows, amb, per = [], set(), []
    for j, c in enumerate(colliders):
        phi, gw = world_sdf(c, pos)
        per.append((phi, gw))
        s = np.nonzero(phi < 0)[0]
        rows.append(np.stack([s, np.full_like(s, j)], 1))
        amb |= {(int(k), j) for k in np.nonzero(np.abs(phi) <= tol)[0]}
    order = np.concatenate(rows)
    order = order[np.lexsort((order[:, 1], order[:, 0]))]
    return order, per, amb


def _scene_colliders(t=0.0):
    from drake_amd import Collider
    return [
        Collider(0, body=0, p_WB=(0.5, 0.5, 0.493), R_WB=_rot((1, 0, 0), 0.05)),
        Collider(4, body=1, p_WB=(0.42 + 0.1 * t, 0.5, 0.5), R_WB=_rot((1, 0.3, 0), 1.4), dims=(0.02, 0.08, 0),
                 v=(0.1, 0, 0), w=(0, 0, 2.0)),
        Collider(5, body=2, p_WB=(0.6, 0.55, 0.5), R_WB=_rot((0.2, 0.5, 1), 0.8), dims=(0.07, 0.03, 0.045),
                 v=(0, 0.1, -0.2), w=(1.0, 0, 0.5)),
        Collider(3, body=3, p_WB=(0.5, 0.35, 0.5), R_WB=_rot((0, 1, 0), 1.2), dims=(0.03, 0.08, 0), v=(0, 0, 0.2)),
    ]


def test_generated_pairs_with_cylinder_and_ellipsoid_match_the_host_loop():
    from drake_amd import GpuMpm, scenes
    g = GpuMpm(7)
    scenes.populate(g, scenes.cloth_stack(4, 60, 7, z0=0.49, vel_amp=0.2))
    g.reallocate_external_bodies(4)
    g.run_substeps(3, DT, -1)
    g.rebuild_mapping(True)
    cols = _scene_colliders()
    n = g.generate_contact_pairs(cols)
    pos = g.sync_particle_state_to_cpu()
    got = g.download_contact_pairs()
    assert n == got[0].size
    order, per, amb = reference_pairs(pos, cols)
    # the collider of a pair: its body here
    gk = [(int(a), int(b)) for a, b in zip(got[0], got[1])]
    assert {k for k in gk if k not in amb} == {(int(a), int(b)) for a, b in order if (int(a), int(b)) not in amb}
    assert n > 1000 and set(int(b) for b in got[1]) == {0, 1, 2, 3}
    # ascending (slot, collider); a slot's pairs are contiguous
    ids = got[0].astype(np.int64) * 8 + got[1]
    assert np.all(np.diff(ids) > 0)
    assert np.all(got[2] < 0)
    np.testing.assert_allclose(np.linalg.norm(got[3], axis=1), 1.0, atol=1e-5)
    phi_ref = np.array([per[b][0][a] for a, b in gk])
    nrm_ref = np.array([-per[b][1][a] for a, b in gk])
    decided = np.array([k not in amb for k in gk])
    assert np.abs(got[2][decided] - phi_ref[decided]).max() < 2e-6
    nd = np.abs(got[3] - nrm_ref).max(1)
    assert np.mean(nd > 1e-4) < 2e-3
    for body in (1, 2):          # the new kinds took part
        assert np.sum(got[1] == body) > 50
    np.testing.assert_array_equal(got[4], pos[got[0]])
    for k, (a, b) in enumerate(gk):
        if k % 97:
            continue
        c = cols[b]
        d = pos[a].astype(np.float64) - np.array(c.p_WB[:])
        rv = np.array(c.v[:]) + np.cross(np.array(c.w[:]), d)
        np.testing.assert_allclose(got[5][k], rv, atol=1e-6)
        np.testing.assert_array_equal(got[6][k], np.array(c.p_WB[:], F))


# ---- 4. more than 16 colliders (the device table) --------------------------------------------------------------------

def test_twenty_colliders_equal_two_calls_of_ten():
    from drake_amd import Collider, GpuMpm, scenes
    g = GpuMpm(7)
    scenes.populate(g, scenes.cloth_stack(3, 60, 7, z0=0.49, vel_amp=0.2))
    g.reallocate_external_bodies(20)
    g.rebuild_mapping(True)
    rng = np.random.default_rng(4)
    cols = []
    for j in range(20):
        x, y = 0.3 + 0.4 * rng.random(), 0.3 + 0.4 * rng.random()
        R = _rot(rng.normal(size=3), rng.uniform(0, np.pi))
        if j % 2:
            cols.append(Collider(5, body=j, p_WB=(x, y, 0.5), R_WB=R, dims=tuple(rng.uniform(0.01, 0.05, 3)), w=(0, 0, 1.0)))
        else:
            cols.append(Collider(4, body=j, p_WB=(x, y, 0.5), R_WB=R, dims=(rng.uniform(0.01, 0.03), rng.uniform(0.02, 0.06), 0),
                                 v=(0.1, 0, 0)))
    n = g.generate_contact_pairs(cols)
    allp = g.download_contact_pairs()
    parts = []
    for half in (cols[:10], cols[10:]):
        g.generate_contact_pairs(half)
        parts.append(g.download_contact_pairs())
    merged = [np.concatenate([a, b]) for a, b in zip(*parts)]
    order = np.lexsort((merged[1], merged[0]))
    assert n > 200 and n == merged[0].size
    for k in range(7):
        np.testing.assert_array_equal(allp[k], merged[k][order], err_msg=str(k))


# ---- 5. one call equals the seven calls, through contact-free stretches ----------------------------------------------

def _rod_and_ellipsoid():
    from drake_amd import Collider
    Ry = _rot((1, 0, 0), np.pi / 2)        # z_B along world y
    return [Collider(5, body=0, p_WB=(0.44, 0.5, 0.5), R_WB=_rot((0, 0, 1), 0.7), dims=(0.06, 0.04, 0.03), w=(0, 0, 3.0)),
            Collider(4, body=1, p_WB=(0.58, 0.5, 0.517), R_WB=Ry, dims=(0.015, 0.1, 0), v=(0, 0, 0.1), w=(0, 2.0, 0))]


@pytest.mark.parametrize("exact", [False, True])
def test_coupled_substeps_over_cylinder_and_ellipsoid_equal_the_seven_calls(exact):
    from drake_amd import scenes
    from tests.test_contact_noroundtrip_gpu import DT as CDT, D, K, MU, _coupled_with, _engine as det_engine, _same, \
        _same_rows, _state
    cols = _rod_and_ellipsoid()
    sheets = scenes.cloth_stack(1, 36, 6, z0=0.5 + 0.03 + 0.006, side=0.3, seed=9, vel_amp=0.02)
    for pos, vel, idx in sheets:
        vel[:, 2] -= 1.0
    n = 90
    a, b = det_engine(None, sheets, bodies=2), det_engine(None, sheets, bodies=2)
    ra = _coupled_with(a, cols, n, exact)
    rb = b.run_coupled_substeps(n, CDT, cols, MU, K, D, exact_line_search=exact)
    b.gpu_sync()
    assert a.stats()["error_flags"] == 0 and b.stats()["error_flags"] == 0
    first = next(i for i, r in enumerate(ra) if r["contacts"] > 0)
    assert 5 < first < n - 20 and max(r["contacts"] for r in ra) > 30, first
    _same_rows(ra, rb, "iterations", "contacts", "residual")
    sa, sb = _state(a), _state(b)
    _same(sa, sb)
    cb = b.contact_counters()
    assert cb["contact_free"] >= first // 2, (cb, first)     # the watch decided those substeps
    assert np.abs(sb["f"][0]).max() > 0 and np.abs(sb["f"][1]).max() > 0


# ---- 6. per-body impulses against the oracle -------------------------------------------------------------------------

def test_moving_cylinders_and_ellipsoids_impulses_per_body_match_the_oracle():
    from drake_amd import ARR as A, Collider
    from oracle import oracle as orc
    from tests.helpers import build_pair, close, solve_tolerance
    o, g = build_pair(layers=3, res=24, z0=0.5, vel_amp=0.2)
    links = [
        Collider(4, body=0, p_WB=(0.42, 0.45, 0.497), R_WB=_rot((0, 1, 0), 1.5708), dims=(0.012, 0.05, 0), v=(0, 0, 0.3)),
        Collider(5, body=1, p_WB=(0.58, 0.45, 0.499), R_WB=_rot((1, 0, 0), 0.6), dims=(0.04, 0.015, 0.02), v=(0.2, 0, 0.2),
                 w=(0, 0, 3.0)),
        Collider(4, body=2, p_WB=(0.50, 0.58, 0.515), R_WB=_rot((1, 1, 0), 1.2), dims=(0.015, 0.04, 0), v=(0, -0.1, -0.4)),
        Collider(5, body=3, p_WB=(0.45, 0.56, 0.49), R_WB=_rot((0, 1, 1), 0.4), dims=(0.02, 0.03, 0.025), v=(0, 0, 0.5)),
    ]
    for s in (o, g):
        s.reallocate_external_bodies(4)
        s.rebuild_mapping(False)
        s.calc_fem_state_and_force(DT)
        s.particle_to_grid(DT)
        s.update_grid(-1)
    n = g.generate_contact_pairs(links)
    pairs = g.download_contact_pairs()
    assert n > 60 and set(int(b) for b in pairs[1]) == {0, 1, 2, 3}
    o.copy_contact_pairs(orc.ContactPairs(*pairs))
    ro = o.update_contact(DT, 0.5, 1e5, 1e-3)
    rg = g.update_contact(DT, 0.5, 1e5, 1e-3)
    assert abs(rg["iterations"] - ro["iterations"]) <= max(3, ro["iterations"] // 4), (rg, ro)
    close(g.download(A.CONTACT_VEL), o.c_vel, scale=1.0, rtol=solve_tolerance(g.contact_stats()["dofs"]),
          what="contact vel (cylinders, ellipsoids)")
    tau_g, f_g = g.external_body_force_to_host()
    close(f_g, o.F_f, scale=float(np.abs(o.F_f).max()), rtol=IMPULSE_RTOL, what="per-body impulse")
    close(tau_g, o.F_tau, scale=float(np.abs(o.F_tau).max()), rtol=IMPULSE_RTOL, what="per-body angular impulse")
    assert np.all(np.abs(o.F_f).max(1) > 0)


# ---- 7. the partitioned domain (team) path ---------------------------------------------------------------------------

def _team_colliders(t):
    """body 0: the floor; body 1 a cylinder, body 2 an ellipsoid, lying on the cloth and moving along x across the cut"""
    from drake_amd import Collider
    from tests.test_team_gpu import FLOOR_Z
    Ry = (0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 1.0, 0.0, 0.0)    # world y = body z (the cylinder's axis)
    return [Collider(0, body=0, p_WB=(0.5, 0.5, FLOOR_Z)),
            Collider(4, body=1, p_WB=(0.485 + 2.0 * t, 0.5, FLOOR_Z + 0.028), R_WB=Ry, dims=(0.02, 0.12, 0.0), v=(2.0, 0, 0)),
            Collider(5, body=2, p_WB=(0.64 - 1.5 * t, 0.5, FLOOR_Z + 0.028), R_WB=Ry, dims=(0.03, 0.05, 0.12), v=(-1.5, 0, 0))]


def test_in_process_world_with_cylinder_and_ellipsoid_matches_single_engine():
    import torch
    from drake_amd import ARR
    from drake_amd.dist import LocalWorld
    from tests.test_team_gpu import CHUNKS, D, DT as TDT, K, MU, _check_against_single_engine, _engine as team_engine, _scene
    sheets = _scene()
    g = team_engine(sheets)
    res, logs, done = [], [], 0
    for k in CHUNKS:
        res += g.run_coupled_substeps(k, TDT, _team_colliders(done * TDT), MU, K, D)
        done += k
        logs.append(g.contact_log().copy())
    g.gpu_sync()
    assert g.stats()["error_flags"] == 0
    tau, f = g.external_body_force_to_host()
    ref = dict(res=res, logs=logs, pos=g.download(ARR.POSITIONS), vel=g.download(ARR.VELOCITIES), tau=tau, f=f,
               dofs=g.contact_stats()["dofs"], n=g.n_particles)
    world = 2
    engines = [team_engine(sheets) for _ in range(world)]
    w = LocalWorld(engines, [0, 8, 16], zone_blocks=2, ghost_cells=0, ghost_margin_cells=0, capacity_blocks=512,
                   migrate_every=0, migrate_capacity=1 << 14, device=torch.device("cuda", 0))
    w.enable_team(512)
    res = [[] for _ in range(world)]
    logs = [[] for _ in range(world)]
    done = 0
    for k in CHUNKS:
        out = w.coupled_substeps(k, TDT, _team_colliders(done * TDT), MU, K, D)
        done += k
        for r in range(world):
            res[r] += out[r]
            logs[r].append(engines[r].contact_log().copy())
    w.sync()
    n = ref["n"]
    owned = np.zeros(n, np.int32)
    pos, vel = np.full((n, 3), np.nan, np.float32), np.full((n, 3), np.nan, np.float32)
    f_sum, tau_sum = np.zeros_like(ref["f"]), np.zeros_like(ref["tau"])
    for e in engines:
        assert e.stats()["error_flags"] == 0
        own = e.dist_roles() == 1
        owned += own
        pos[own], vel[own] = e.download(ARR.POSITIONS)[own], e.download(ARR.VELOCITIES)[own]
        tau, f = e.external_body_force_to_host()
        f_sum += f
        tau_sum += tau
    _check_against_single_engine(ref, res, logs, owned, pos, vel, f_sum, tau_sum, "world of 2, cylinder and ellipsoid")


# ---- 8. refusals -------------------------------------------------------------------------------------------------------

def test_bad_dimensions_and_unknown_kinds_are_refused():
    from drake_amd import Collider, MpmError, scenes
    from drake_amd import GpuMpm
    g = GpuMpm(6)
    sheets = scenes.cloth_stack(1, 24, 6, z0=0.5 - 0.002, side=0.2, seed=1, vel_amp=0.0)
    scenes.populate(g, sheets)
    g.reallocate_external_bodies(1)
    g.rebuild_mapping(False)
    good = [Collider(0, p_WB=(0.5, 0.5, 0.5))]
    n_good = g.generate_contact_pairs(good)
    assert n_good > 0
    nan = float("nan")
    bad = [Collider(4, dims=(0.0, 0.1, 0)), Collider(4, dims=(0.1, -0.1, 0)), Collider(4, dims=(nan, 0.1, 0)),
           Collider(4, dims=(0.1, float("inf"), 0)), Collider(5, dims=(0.1, 0.1, 0.0)), Collider(5, dims=(0.1, -1, 0.1)),
           Collider(5, dims=(nan, 0.1, 0.1)), Collider(6, dims=(0.1, 0.1, 0.1))]
    pts = np.zeros((4, 3), F)
    for c in bad:
        for call in (lambda: g.generate_contact_pairs(good + [c]),
                     lambda: g.collider_signed_distance(c, pts),
                     lambda: g.run_coupled_substeps(2, DT, good + [c], 0.5, 1e5, 1e-3)):
            with pytest.raises(MpmError) as e:
                call()
            assert e.value.code == -1
        # nothing generated
        assert g.contact_pair_count() == 0
    assert g.stats()["substeps"] == 0
    # the next valid call solves normally
    g.rebuild_mapping(False)
    g.calc_fem_state_and_force(DT)
    g.particle_to_grid(DT)
    g.update_grid(-1)
    assert g.generate_contact_pairs(good + [Collider(4, p_WB=(0.5, 0.5, 0.5), dims=(0.02, 0.03, 0)),
                                            Collider(5, p_WB=(0.55, 0.5, 0.5), dims=(0.02, 0.03, 0.01))]) > n_good
    r = g.update_contact(DT, 0.5, 1e5, 1e-3)
    assert r["iterations"] >= 1 and g.stats()["error_flags"] == 0
