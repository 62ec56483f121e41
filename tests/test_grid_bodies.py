"""Rigid bodies of the grid update (mpm_set_grid_bodies), the part that needs no GPU: the binding against the header, the
float64 reference of tests/grid_bodies.py against answers it cannot get wrong by construction, and the conditions of the
per-node comparison for every scene tests/test_grid_bodies_gpu.py uses -- a scene that cannot meet them is found here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import grid_bodies as gb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_binding_matches_the_header():
    from drake_amd import BC_BODIES, GB_NO_MESH, Collider, GridBody, capi
    text = open(os.path.join(ROOT, "include", "mpm_hip.h")).read()
    assert int(re.search(r"#define MPM_BC_BODIES (\d+)", text).group(1)) == BC_BODIES
    assert int(re.search(r"#define MPM_GB_NO_MESH (0x[0-9A-Fa-f]+)u", text).group(1), 16) == GB_NO_MESH
    # mpm_grid_body_t: the collider, then three 4-byte fields
    assert C.sizeof(GridBody) == C.sizeof(Collider) + 12 and GridBody.shape.offset == 0
    assert [f[0] for f in GridBody._fields_] == ["shape", "sdf_shape", "mode", "friction"]
    for name in ("mpm_set_grid_bodies", "mpm_get_grid_bodies"):
        assert name in capi.SYMBOLS and hasattr(capi.load_library(), name)
    b = gb.Body(gb.BOX, body=3, p=(0.1, 0.2, 0.3), R=gb.rot((1, 2, 3), 0.5), dims=(1, 2, 3), v=(4, 5, 6), w=(7, 8, 9),
                mode=gb.SLIP, friction=0.25).capi()
    assert (b.shape.kind, b.shape.body, b.sdf_shape, b.mode, b.friction) == (2, 3, GB_NO_MESH, 2, 0.25)
    assert np.array_equal(np.array(b.shape.R_WB[:], np.float32).reshape(3, 3), gb.rot((1, 2, 3), 0.5))


def _nodes(n=4000, seed=5):
    rng = np.random.default_rng(seed)
    x = 0.5 + 0.2 * (rng.random((n, 3)) - 0.5)
    v = rng.normal(size=(n, 3))
    return x, v


@pytest.mark.parametrize("kind", range(6))
def test_reference_modes_against_known_answers(kind):
    x, v_in = _nodes()
    b = gb._kind_body(kind, gb.FIXED)
    phi, n = gb.body_sdf(b, x)
    sel = phi < 0
    assert sel.sum() > 50
    x, v_in, n = x[sel], v_in[sel], n[sel]
    assert np.allclose(np.linalg.norm(n, axis=1), 1.0, rtol=0, atol=1e-6)
    vc = gb.rigid_velocity(b, x)
    # FIXED: the body's velocity, exactly
    assert np.array_equal(gb.apply_mode(b, v_in, vc, n), vc)
    # SLIP with friction 1 is FIXED
    b.mode, b.friction = gb.SLIP, np.float32(1.0)
    assert np.allclose(gb.apply_mode(b, v_in, vc, n), vc, rtol=0, atol=1e-14)
    # SLIP with friction 0 keeps the tangential part of v_in - v_c and removes the normal part
    b.friction = np.float32(0.0)
    out = gb.apply_mode(b, v_in, vc, n)
    rel_in, rel_out = v_in - vc, out - vc
    tang = rel_in - n * (n * rel_in).sum(-1)[:, None]
    # (to the orthogonality of a rotation rounded to float32: |n| is 1 within ~1e-7, and the engine takes R_WB as given)
    assert np.allclose((n * rel_out).sum(-1), 0.0, atol=1e-6)
    assert np.allclose(rel_out, tang, atol=1e-6)
    # SLIP_APPROACHING leaves a separating node alone, and is SLIP for an approaching one
    b.mode, b.friction = gb.SLIP_APPROACHING, np.float32(0.3)
    out = gb.apply_mode(b, v_in, vc, n)
    approaching = (n * (vc - v_in)).sum(-1) > 0
    assert approaching.any() and (~approaching).any()
    assert np.array_equal(out[~approaching], v_in[~approaching])
    b.mode = gb.SLIP
    assert np.array_equal(out[approaching], gb.apply_mode(b, v_in, vc, n)[approaching])


def test_reference_distances_against_independent_forms():
    """phi of the closed forms against the distance to a dense sample of each surface, and the gradient against the
    finite difference of phi"""
    x, _ = _nodes(1500, seed=9)
    for kind in (gb.SPHERE, gb.BOX, gb.CAPSULE, gb.CYLINDER):
        b = gb._kind_body(kind, gb.FIXED)
        phi, n = gb.body_sdf(b, x)
        h = 1e-6
        fd = np.stack([(gb.body_sdf(b, x + h * np.eye(3)[a])[0] - gb.body_sdf(b, x - h * np.eye(3)[a])[0]) / (2 * h)
                       for a in range(3)], -1)
        smooth = np.abs(fd - n).max(-1) < 1e-3          # (all but the nodes next to a medial surface)
        assert smooth.mean() > 0.97, (kind, smooth.mean())
    # the ellipsoid: the gradient is normal to the surface at the nearest point N = x - phi_true n, which lies on it
    # (in an unrotated frame: a rotation rounded to float32 is orthogonal to ~1e-7 only)
    b = gb.Body(gb.ELLIPSOID, p=(0.5, 0.5, 0.5), dims=(0.10, 0.06, 0.045))
    _, n = gb.body_sdf(b, x)
    xb = (x - b.p.astype(float)) @ b.R.astype(float)
    nb = n @ b.R.astype(float)
    a = b.dims.astype(float)
    # N = a^2 nb s with s > 0 on the surface: s = 1 / |a nb|; then x_B - N is parallel to nb
    N = a ** 2 * nb / np.linalg.norm(a * nb, axis=1)[:, None]
    d = xb - N
    assert np.allclose(np.cross(d, nb), 0.0, atol=1e-12)
    # a sphere-like ellipsoid has the sphere's normal
    s = gb.Body(gb.ELLIPSOID, p=b.p, R=b.R, dims=(0.08, 0.08, 0.08))
    _, n = gb.body_sdf(s, x)
    r = x - b.p.astype(float)
    assert np.allclose(n, r / np.linalg.norm(r, axis=1)[:, None], atol=1e-9)


def test_reference_first_body_decides_and_reaction_balances():
    sheets, tables = gb.overlap_scene()
    bodies = tables["overlap"]
    on = gb.massive_nodes(sheets, gb.BITS)
    n_cells = 1 << (3 * gb.BITS)
    rng = np.random.default_rng(3)
    m = np.zeros(n_cells)
    m[on] = 1e-6 * (1 + rng.random(len(on)))
    mv = np.zeros((n_cells, 3))
    mv[on] = m[on, None] * rng.normal(size=(len(on), 3))
    r = gb.reference(m, mv, gb.BITS, bodies, gb.N_ACC)
    for k, b in enumerate(bodies):
        mine = r["decider"] == k
        assert mine.sum() > 0, k
        assert (gb.body_sdf(b, r["x"][mine], normals=False)[0] < 0).all()
        for j in range(k):      # no earlier body contains the node
            assert (gb.body_sdf(bodies[j], r["x"][mine], normals=False)[0] >= 0).all()
    free = r["decider"] < 0
    assert np.array_equal(r["v"][free], r["v_in"][free])
    # the cloth's momentum change is the opposite of what the in-range bodies received
    in_range = np.isin(r["decider"], [k for k, b in enumerate(bodies) if b.body < gb.N_ACC])
    dp = (m[r["on"]][in_range, None] * (r["v"] - r["v_in"])[in_range]).sum(0)
    assert np.allclose(dp, -r["imp"][:, 3:].sum(0), rtol=1e-12, atol=1e-18)
    assert r["imp"].shape == (gb.N_ACC, 6) and np.abs(r["imp"][3]).sum() > 0


@pytest.mark.parametrize("name", sorted(gb.SCENES))
def test_scene_meets_the_conditions_of_the_comparison(name):
    """at most 1 % of the massive nodes inside some body undecided, at least 100 compared nodes per kind and mode"""
    sheets, tables = gb.SCENES[name]()
    on = gb.massive_nodes(sheets, gb.BITS)
    x = gb.node_positions(gb.BITS, on)
    for key, bodies in tables.items():
        for b in bodies:
            if b.kind == gb.MESH:
                b.cpu_lattice()
        decider = np.full(len(on), -1)
        for k, b in enumerate(bodies):
            free = np.nonzero(decider < 0)[0]
            decider[free[gb.body_sdf(b, x[free], normals=False)[0] < 0]] = k
        und = gb.undecided(bodies, x, decider)
        share, counts = gb.check_scene_conditions(bodies, x, decider, und)
        print(name, key, "inside", int((decider >= 0).sum()), "undecided share", share, counts)
        assert share <= gb.MAX_UNDECIDED_SHARE, (name, key, share)
        assert all(c >= gb.MIN_COMPARED for c in counts.values()), (name, key, counts)
        if key == gb.FIXED or name == "overlap":
            break    # (the three modes of a kind scene share the body's pose: the conditions are the same)
