"""Rest shape apart from the pose (mpm_set_rest_shape) without a GPU: the three entry points exist in the library, the
binding and the C++ facade; the host function mpm_rest_shape_check (no handle, no device) gives float64's verdict on
slivers, near-degenerate, zero-edge, zero-area and NaN faces and names the first bad face; the refusals that need no
device; and the conditions tests/rest_shape.py states about its own cases."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import rest_meshes as rm
from tests import rest_shape as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_rest_shape_entry_points():
    import drake_amd
    from drake_amd import capi
    lib = capi.load_library()
    for name in ("mpm_set_rest_shape", "mpm_get_rest_shape", "mpm_rest_shape_check"):
        assert hasattr(lib, name), name
        assert name in capi.SYMBOLS
    for name in ("set_rest_shape", "get_rest_shape", "rest_shape_check"):
        assert hasattr(capi.GpuMpm, name), name
    assert drake_amd.rest_shape_check is capi.rest_shape_check
    text = open(os.path.join(ROOT, "include", "gpu_mpm.hpp")).read()
    for name in ("SetRestShape", "ClearRestShape", "GetRestShape"):
        assert name in text, name
    header = open(os.path.join(ROOT, "include", "mpm_hip.h")).read()
    for name in ("mpm_set_rest_shape", "mpm_get_rest_shape", "mpm_rest_shape_check", "THE MASS RULE", "THE ORDERING RULE"):
        assert name in header, name


def _first_bad64(pos, idx):
    """float64's verdict from the float32 positions: the first face whose |e0|^2 or |e0 x e1|^2 is not a positive finite
    number, or -1"""
    x = np.asarray(pos, np.float32).astype(np.float64)
    e0, e1 = x[idx[:, 1]] - x[idx[:, 0]], x[idx[:, 2]] - x[idx[:, 0]]
    n = np.cross(e0, e1)
    with np.errstate(invalid="ignore"):
        l2, n2 = (e0 * e0).sum(axis=1), (n * n).sum(axis=1)
        good = (l2 > 0) & np.isfinite(l2) & (n2 > 0) & np.isfinite(n2)
    bad = np.flatnonzero(~good)
    return int(bad[0]) if bad.size else -1


@pytest.mark.parametrize("name", ["slivers", "scales", "orientations", "valence"])
def test_check_accepts_every_mesh_however_thin(name):
    """no conditioning threshold: kappa up to 1e4 and edges down to 1e-3 dx pass, as they pass mpm_finalize"""
    from drake_amd import rest_shape_check
    mesh, ref = rm.meshes()[name]
    assert _first_bad64(mesh.pos, mesh.idx) == -1
    assert rest_shape_check(mesh.pos, mesh.idx) == (True, -1)
    if name == "slivers":
        assert ref["kappa"].max() > 5e3


def _tampered():
    """the slivers mesh (disjoint triangles) with faces made bad in place: {what: (pos, expected first bad face)}"""
    mesh = rm.meshes()["slivers"][0]
    h = np.float32(2.0 ** -7)
    out = {}

    def with_faces(faces):
        p = mesh.pos.copy()
        for f, kind in faces:
            a = np.array([0.5, 0.5, 0.5], np.float32)
            if kind == "zero edge":            # e0 = 0, the area with it
                p[3 * f], p[3 * f + 1], p[3 * f + 2] = a, a, a + np.array([0, h, 0], np.float32)
            elif kind == "zero area":          # three points on a line, exactly
                p[3 * f], p[3 * f + 1], p[3 * f + 2] = a, a + np.array([h, 0, 0], np.float32), a + np.array([2 * h, 0, 0], np.float32)
            elif kind == "second edge zero":   # e1 = 0: e0 is fine, the area is zero
                p[3 * f], p[3 * f + 1], p[3 * f + 2] = a, a + np.array([h, 0, 0], np.float32), a
            elif kind == "nan":
                p[3 * f + 2, 1] = np.nan
            elif kind == "inf":
                p[3 * f + 1, 0] = np.inf
            elif kind == "one ulp of area":    # the line again with one corner moved by one ulp: thin, not degenerate
                p[3 * f], p[3 * f + 1] = a, a + np.array([h, 0, 0], np.float32)
                p[3 * f + 2] = a + np.array([2 * h, 0, 0], np.float32)
                p[3 * f + 2, 1] = np.nextafter(np.float32(0.5), np.float32(1.0))
        return p

    out["zero edge"] = (with_faces([(17, "zero edge")]), 17)
    out["zero area"] = (with_faces([(400, "zero area")]), 400)
    out["second edge zero"] = (with_faces([(3, "second edge zero")]), 3)
    out["nan"] = (with_faces([(0, "nan")]), 0)
    out["inf"] = (with_faces([(659, "inf")]), 659)
    out["first of several"] = (with_faces([(500, "nan"), (120, "zero area"), (121, "zero edge"), (300, "inf")]), 120)
    out["last face"] = (with_faces([(mesh.nf - 1, "zero edge")]), mesh.nf - 1)
    out["one ulp of area"] = (with_faces([(50, "one ulp of area")]), -1)
    return mesh, out


def test_check_names_the_first_bad_face_as_float64_does():
    from drake_amd import rest_shape_check
    mesh, cases = _tampered()
    for what, (pos, expect) in cases.items():
        assert _first_bad64(pos, mesh.idx) == expect, what          # (the test's own construction)
        ok, bad = rest_shape_check(pos, mesh.idx)
        assert bad == expect and ok == (expect < 0), (what, ok, bad)


def test_check_refuses_what_is_not_a_face_list():
    from drake_amd import capi, rest_shape_check
    lib = capi.load_library()
    mesh = rm.meshes()["valence"][0]
    idx = mesh.idx.copy()
    idx[5, 1] = mesh.nv
    assert rest_shape_check(mesh.pos, idx) == (False, -1)
    assert b"index out of range" in lib.mpm_last_error()
    idx[5, 1] = -1
    assert rest_shape_check(mesh.pos, idx) == (False, -1)
    # a NaN at a vertex in no face: no face is bad, the shape is refused all the same
    pos = mesh.pos.copy()
    pos[mesh.info["isolated"], 2] = np.nan
    assert rest_shape_check(pos, mesh.idx) == (False, -1)
    assert b"not finite" in lib.mpm_last_error()
    # nothing at all is a valid (empty) shape; null arrays with counts are not
    assert rest_shape_check(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)) == (True, -1)
    bad = C.c_int32(7)
    assert lib.mpm_rest_shape_check(None, 3, None, 1, C.byref(bad)) == -1
    assert b"null array" in lib.mpm_last_error()
    assert lib.mpm_rest_shape_check(mesh.pos.ctypes.data, mesh.nv, mesh.idx.ctypes.data, mesh.nf, None) == 0


def test_null_handle_is_refused_without_a_device():
    from drake_amd import capi
    lib = capi.load_library()
    r = np.zeros((4, 3), np.float32)
    flag = C.c_int(5)
    assert lib.mpm_set_rest_shape(None, r.ctypes.data) == -1
    assert b"null handle" in lib.mpm_last_error()
    assert lib.mpm_set_rest_shape(None, None) == -1
    assert lib.mpm_get_rest_shape(None, r.ctypes.data, C.byref(flag)) == -1
    assert b"null handle" in lib.mpm_last_error()
    assert flag.value == 5 and not r.any()


@pytest.mark.parametrize("name,kind", rs.CASES)
def test_the_cases_own_conditions(name, kind):
    from drake_amd import rest_shape_check
    c = rs.case(name, kind)
    rest, pose, ref, m = c["rest"], c["pose"], c["ref"], c["base"]
    assert rest.nv == pose.nv == m.nv and np.array_equal(rest.idx, pose.idx) and np.array_equal(rest.idx, m.idx)
    for x in (rest.pos, pose.pos):
        assert x.dtype == np.float32 and x.min() >= rs.DOMAIN[0] and x.max() <= rs.DOMAIN[1], (float(x.min()), float(x.max()))
    assert rest_shape_check(rest.pos, rest.idx) == (True, -1) and rest_shape_check(pose.pos, pose.idx) == (True, -1)
    assert ref["nf"] == rest.nf and ref["kappa"].max() <= rm.KAPPA_MAX
    r64, p64 = rest.pos.astype(np.float64), pose.pos.astype(np.float64)
    if kind == "double":
        assert np.array_equal(2.0 * r64, p64)
    elif kind == "shift":
        assert np.array_equal(r64 + rs.SHIFT, p64)
    else:
        assert rest is m and not np.array_equal(rest.pos, pose.pos)
    # the pose is another shape (or the same one elsewhere): its own float64 rest state says by how much
    if kind in ("scale", "double"):
        vp = rm.rest_state(pose)["vol"][:rest.nf]
        assert np.abs(vp / ref["vol"][:rest.nf] - 1.0).min() > 1e-3
    if kind in ("noise", "shear"):     # (a shear keeps the area of a face whose normal lies along its invariant direction)
        vp = rm.rest_state(pose)["vol"][:rest.nf]
        assert np.median(np.abs(vp / ref["vol"][:rest.nf] - 1.0)) > 1e-3
    if c["parts"] is not None:
        assert sum(r.nv for r, _ in c["parts"]) == rest.nv and sum(r.nf for r, _ in c["parts"]) == rest.nf
        assert np.array_equal(np.concatenate([p.pos for _, p in c["parts"]]), pose.pos)


def test_the_sheets_own_conditions():
    pos, idx = rs.sheet()
    assert pos.shape == (144, 3) and idx.shape == (242, 3)
    assert len(rs.boundary()) == 44
    assert abs(rs.mean_edge(rs.scaled(pos, 1.25), idx) / rs.mean_edge(pos, idx) - 1.25) < 1e-6
    # the state that gives two engines one particle order: every particle in a cell of its own, inside the walls
    wide = rs.spread(idx)
    assert rs.one_per_cell(wide, idx) and not rs.one_per_cell(pos, idx)
    assert wide.min() >= 0.15 and wide.max() <= 0.85
    # the closed mesh of the pressure test and its mirror image
    X, T = rs.octahedron()
    from drake_amd import mesh_is_closed
    assert mesh_is_closed(T, len(X)) == (True, None)
    mirror = X.copy()
    mirror[:, 0] = np.float32(1.0) - X[:, 0]
    assert rs.signed_volume(X, T) > 0 > rs.signed_volume(mirror, T)
    # the rolled sheet keeps its arc length
    bent = rs.arc(pos, 0.15)
    assert abs(rs.mean_edge(bent, idx) / rs.mean_edge(pos, idx) - 1.0) < 0.01 and np.ptp(bent[:, 2]) > 0.02
