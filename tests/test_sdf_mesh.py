"""Mesh colliders without a GPU: the entry points are declared, bound and exported, the ctypes struct is the C struct, and
the float64 reference of tests/sdf_mesh_reference.py agrees with closed forms (box exactly, sphere to chord error)."""
import os
import re
import subprocess

import numpy as np

from tests import sdf_mesh_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["mpm_sdf_shape_from_mesh", "mpm_sdf_shape_info", "mpm_sdf_shape_download", "mpm_set_sdf_colliders",
                "mpm_sdf_collider_signed_distance"]


def _header():
    return open(os.path.join(ROOT, "include", "mpm_hip.h")).read()


def test_entry_points_are_declared_bound_and_exported():
    from drake_amd import capi
    h = _header()
    lib = capi.load_library()
    for name in ENTRY_POINTS:
        assert re.search(r"MPM_API\s+int\s+" + name + r"\s*\(", h), name
        assert name in capi.SYMBOLS, name
        assert hasattr(lib, name), name
    for m in ("sdf_shape_from_mesh", "sdf_shape_info", "sdf_shape_download", "set_sdf_colliders",
              "sdf_collider_signed_distance"):
        assert hasattr(capi.GpuMpm, m), m


def test_ctypes_struct_matches_the_c_struct(tmp_path):
    from drake_amd import SdfCollider
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mpm_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(mpm_sdf_collider_t), offsetof(mpm_sdf_collider_t, shape),\n'
                   '         offsetof(mpm_sdf_collider_t, body), offsetof(mpm_sdf_collider_t, p_WB),\n'
                   '         offsetof(mpm_sdf_collider_t, R_WB), offsetof(mpm_sdf_collider_t, v), offsetof(mpm_sdf_collider_t, w));\n'
                   '  return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    want = [__import__("ctypes").sizeof(SdfCollider)] + [getattr(SdfCollider, f).offset
                                                         for f in ("shape", "body", "p_WB", "R_WB", "v", "w")]
    assert got == want, (got, want)
    assert got[0] == 4 * (2 + 3 + 9 + 3 + 3)


def test_reference_matches_the_analytic_box():
    half = (0.04, 0.03, 0.02)
    v, f = ref.box(half)
    rng = np.random.default_rng(1)
    pts = rng.uniform(-0.08, 0.08, (3000, 3))
    # (the half extents the float32 corners carry)
    np.testing.assert_allclose(ref.mesh_sdf(pts, v, f), ref.analytic_box_sdf(pts, v.astype(np.float64).max(0)), atol=1e-12)


def test_reference_matches_the_sphere_to_chord_error():
    r = 0.05
    v, f = ref.icosphere(r, 3)
    # chord error: the inscribed polyhedron lies between the sphere and the sphere of its nearest face plane
    V = v.astype(np.float64)
    n = np.cross(V[f[:, 1]] - V[f[:, 0]], V[f[:, 2]] - V[f[:, 0]])
    h = np.abs(np.einsum("ij,ij->i", n, V[f[:, 0]])) / np.linalg.norm(n, axis=1)
    sag = r - h.min()
    rng = np.random.default_rng(2)
    d = rng.normal(size=(2000, 3))
    pts = d / np.linalg.norm(d, axis=1)[:, None] * rng.uniform(0.2 * r, 2 * r, (2000, 1))
    got = ref.mesh_sdf(pts, v, f)
    want = np.linalg.norm(pts, axis=1) - r
    assert np.abs(got - want).max() <= sag + 1e-6 * r, (np.abs(got - want).max(), sag)
    assert np.all(np.sign(got) == np.sign(want))   # (no point within the chord error of the surface here: rare)


def test_winding_number_ignores_the_orientation_and_a_missing_triangle():
    v, f = ref.torus()
    inside = np.array([[0.05, 0.0, 0.0], [0.0, -0.05, 0.005]])
    outside = np.array([[0.0, 0.0, 0.0], [0.1, 0.0, 0.0], [0.05, 0.0, 0.03]])
    for tris in (f, f[:, ::-1], f[1:], f[::-1][1:]):
        phi = ref.mesh_sdf(np.concatenate([inside, outside]), v, tris)
        assert np.all(phi[:2] < 0) and np.all(phi[2:] > 0), phi
