"""Per-cloth materials (include/mpm_hip.h: mpm_add_qr_cloth_with_material) without a GPU: the C ABI declares, binds and
exports the new calls, the ctypes layout of mpm_cloth_material_t matches the header, and the C++ facade's AddQRCloth
overload compiles against the header alone."""
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mpm_add_qr_cloth_with_material", "mpm_get_cloth_info", "mpm_cloth_count")


def _header():
    return open(os.path.join(ROOT, "include", "mpm_hip.h")).read()


def _cxx():
    cc = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cc is None:
        pytest.skip("no host C++ compiler")
    return cc


def test_material_calls_are_declared_bound_and_exported():
    from drake_amd import ARR, ClothMaterial, capi  # noqa: F401
    text = _header()
    for name in NEW:
        assert re.search(r"MPM_API\s+int\s+" + name + r"\s*\(", text), name
        assert name in capi.SYMBOLS, name
    assert re.search(r"MPM_ARR_MASSES\s*=\s*20\b", text)
    assert ARR.MASSES == 20
    lib = capi.load_library()
    for name in NEW:
        assert hasattr(lib, name), name
    for m in ("add_qr_cloth", "cloth_info", "cloth_count"):
        assert hasattr(capi.GpuMpm, m), m
    import inspect
    assert "material" in inspect.signature(capi.GpuMpm.add_qr_cloth).parameters


def test_ctypes_layout_matches_the_header():
    from drake_amd import ClothMaterial
    fields = [f for f, _ in ClothMaterial._fields_]
    assert fields == ["youngs_modulus", "poisson_ratio", "density", "gamma", "K", "c_F"]
    src = "#include <cstddef>\n#include <cstdio>\n#include \"mpm_hip.h\"\nint main() {\n"
    src += '  std::printf("%zu\\n", sizeof(mpm_cloth_material_t));\n'
    for f in fields:
        src += f'  std::printf("{f} %zu\\n", offsetof(mpm_cloth_material_t, {f}));\n'
    src += "  return 0;\n}\n"
    with tempfile.TemporaryDirectory() as d:
        c, exe = os.path.join(d, "l.cc"), os.path.join(d, "l")
        open(c, "w").write(src)
        subprocess.check_call([_cxx(), "-std=c++17", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        out = subprocess.check_output([exe]).decode().split("\n")
    assert C.sizeof(ClothMaterial) == int(out[0])
    for ln in out[1:]:
        if ln.strip():
            f, off = ln.split()
            assert getattr(ClothMaterial, f).offset == int(off), f


def test_ctypes_material_of_an_engine_material():
    from drake_amd import ClothMaterial, Material
    m = Material(youngs_modulus=1e5, poisson_ratio=0.25, density=500.0, gamma=2.0, K=3e4, V=0.5, c_F=7.0)
    c = ClothMaterial.of(m)
    assert c.as_dict() == dict(youngs_modulus=1e5, poisson_ratio=0.25, density=500.0, gamma=2.0, K=3e4, c_F=7.0)


def test_facade_overload_compiles_header_only():
    src = r"""
#include "gpu_mpm.hpp"
using drake::multibody::gmpm::GpuMpmState;
void add(GpuMpmState<float>& s, const mpm_cloth_material_t& m) {
    std::vector<typename std::decay<decltype(s.positions_host()[0])>::type> pos(3), vel(3);
    std::vector<int> idx{0, 1, 2};
    s.AddQRCloth(pos, vel, idx, m);
    s.AddQRCloth(pos, vel, idx);
    const size_t n = s.n_cloths();
    const mpm_cloth_material_t back = s.cloth_material(n - 1);
    (void)back;
}
"""
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "f.cc")
        open(c, "w").write(src)
        subprocess.check_call([_cxx(), "-std=c++17", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), c])
