"""The C++ facade (include/gpu_mpm.hpp) without a GPU.

The facade is a class template: a member nobody calls is never instantiated, and what the ctypes binding proves about the
C ABI proves nothing about the C++ marshalling in front of it.  Three checks:

  instantiate   every member of GpuMpmState<float> and GpuMpmSolver<float>, with the driver, under -Wall -Wextra -Werror.
  sizes         tests/facade_sizes.cc calls every method that allocates a buffer for the C ABI or forwards a caller's size,
                in front of tests/facade_stub.cc -- a stub of the C ABI that models an engine by its counts alone and writes
                every output over exactly the extent include/mpm_hip.h documents.  A stand-alone host program with its own
                main under the address and undefined-behaviour sanitizers (the FLAGS of tests/test_features.py); nothing
                is loaded into Python.  It prints one "ok <Method>" per method; the full list is asserted here.
  layouts       sizeof and every field's offset of every struct the facade passes through, compiled from the header,
                against the binding's ctypes structures and numpy records (tests/facade_scene.layouts): the GPU replay
                (tests/test_facade_gpu.py) hands the C++ side the raw bytes of the binding's tables.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
INCLUDES = ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "drake_amd", "host")]
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]

# the sixteen evaluators that take their extent from the caller
EVALUATORS = ("BendingForces", "DampingForces", "WeaveForces", "LinkForces", "AnchorForces", "PressureForces", "ShellForces",
              "ShellDampingForces", "WeaveAxes", "WeaveStrain", "TearState", "TearMeasure", "FaceStrain", "ShellCutHinges",
              "ShellDampingPower", "ShellEnergy")
# the two-call getters
TABLES = ("GetPins", "GetGridBodies", "GetForceFields", "GetBending", "GetDamping", "GetWeave", "GetLinks", "GetLinkLimits",
          "GetAnchors", "GetPressure", "PressureState", "GetShellBending", "GetShellDamping", "GetCreases", "PressureVented",
          "GetBodyContactMaterials")
# the others that allocate for the C ABI
OTHERS = ("GetTearing", "LinkEnergy", "LinkBreakState", "LinkBreakMeasure", "AnchorState", "CreaseState", "CreaseMeasure",
          "WeaveEnergy", "Measure", "CalcKineticEnergy", "CalcPotentialEnergy", "GetRestShape", "DumpCpuState",
          "SyncParticleStateToCpu", "ColliderSignedDistance", "SdfColliderSignedDistance", "DownloadContactPairs",
          "RunCoupledSubsteps", "ExternelBodyForceToHost", "FinalizeExternalContactForces", "AddAppliedExternalSpatialForces")
# the setters: null for an empty optional table, the count, the bytes, the size checks
SETTERS = ("SetWeave", "SetShellBending", "SetCreaseState", "SetRestShape", "SetTornFaces", "SetBrokenLinks", "SetBodyMotions",
           "SetPins", "SetGridBodies", "SetForceFields", "SetBending", "SetDamping", "SetLinks", "SetLinkLimits", "SetAnchors",
           "SetPressure", "SetShellDamping", "SetCreases", "SetBodyContactMaterials", "SetSdfColliders")
METHODS = EVALUATORS + TABLES + OTHERS + SETTERS


def _cxx():
    cc = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cc is None:
        pytest.skip("no host C++ compiler")
    return cc


def test_every_member_of_the_facade_instantiates(tmp_path):
    src = tmp_path / "all.cc"
    src.write_text('#include "gpu_mpm.hpp"\n#include "mpm_driver.hpp"\n'
                   "namespace drake { namespace multibody { namespace gmpm {\n"
                   "template struct GpuMpmState<float>;\ntemplate class GpuMpmSolver<float>;\n"
                   "template void InitalizeExternalContactForces<float>(GpuMpmState<float>*, const std::vector<Vec3<float>>&);\n"
                   "template void FinalizeExternalContactForces<float>(GpuMpmState<float>*, const float&);\n"
                   "template void AddAppliedExternalSpatialForces<float>(const GpuMpmState<float>&, const std::vector<std::array<float, 9>>&,\n"
                   "                                                     std::vector<Vec3<float>>*, std::vector<Vec3<float>>*);\n"
                   "}}}\n")
    subprocess.check_call([_cxx(), "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", *INCLUDES, str(src)])


@pytest.fixture(scope="module")
def sizes_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("facade") / "facade_sizes")
    subprocess.check_call([_cxx(), *FLAGS, "-Wall", "-Wextra", "-Werror", *INCLUDES, "-I", TESTS,
                           os.path.join(TESTS, "facade_sizes.cc"), os.path.join(TESTS, "facade_stub.cc"), "-o", exe])
    return exe


def test_facade_sizes_in_front_of_the_stub(sizes_program):
    out = subprocess.run([sizes_program], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.split("\n")[:-1] == ["ok " + m for m in METHODS]
    assert len(set(METHODS)) == len(METHODS)


def test_every_listed_method_is_a_member_of_the_facade():
    text = open(os.path.join(ROOT, "include", "gpu_mpm.hpp")).read()
    import re
    for m in METHODS:
        assert re.search(r"\b" + m + r"\(", text), m


def test_every_public_method_has_a_block_in_the_replay():
    """the GPU replay (tests/test_facade_gpu.py) names every public method: a method added to the header without a call
    in the replay fails here, without a GPU"""
    from tests import facade_scene
    assert facade_scene.public_methods(ROOT) == set(facade_scene.METHOD_BLOCKS) | set(facade_scene.NOT_REPLAYED)
    replay = open(os.path.join(ROOT, "drake_amd", "host", "facade_replay.cc")).read()
    import re
    for m in facade_scene.METHOD_BLOCKS:
        assert re.search(r"\b" + m + r"\(", replay), m


def test_binding_layouts_match_the_header(tmp_path):
    import ctypes as C

    from tests import facade_scene
    layouts = facade_scene.layouts()
    assert set(layouts) == set(facade_scene.STRUCTS)
    src = '#include <cstddef>\n#include <cstdio>\n#include "mpm_hip.h"\nint main() {\n'
    fields = {}
    for name, t in layouts.items():
        fields[name] = [f[0] for f in t._fields_] if isinstance(t, type) and issubclass(t, C.Structure) else list(t.names)
        src += f'  std::printf("{name} sizeof %zu\\n", sizeof({name}));\n'
        for f in fields[name]:
            src += f'  std::printf("{name} {f} %zu %zu\\n", offsetof({name}, {f}), sizeof((({name}*)0)->{f}));\n'
    src += "  return 0;\n}\n"
    c, exe = tmp_path / "layouts.cc", tmp_path / "layouts"
    c.write_text(src)
    subprocess.check_call([_cxx(), "-std=c++17", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)])
    seen = {name: set() for name in layouts}
    covered = {name: 0 for name in layouts}
    sizes = {}
    for ln in subprocess.check_output([str(exe)]).decode().splitlines():
        name, f, *nums = ln.split()
        t = layouts[name]
        ctype = isinstance(t, type) and issubclass(t, C.Structure)
        if f == "sizeof":
            sizes[name] = int(nums[0])
            assert (C.sizeof(t) if ctype else t.itemsize) == int(nums[0]), name
            continue
        off, size = (getattr(t, f).offset, getattr(t, f).size) if ctype else (t.fields[f][1], t.fields[f][0].itemsize)
        assert (off, size) == (int(nums[0]), int(nums[1])), (name, f)
        seen[name].add(f)
        covered[name] += size
    for name in layouts:
        assert seen[name] == set(fields[name]), name
        # the binding names every field of the header's struct: together they fill it (none of these structs is padded)
        assert covered[name] == sizes[name], name
