"""The C++ facade (include/gpu_mpm.hpp) against the ctypes binding on one scene, to the bit.

Both marshal into the same C ABI, so in deterministic mode the same script of calls gives the same bits through either:
the tolerance is zero and nothing is measured.  The binding's side is what the other GPU tests hold against float64, so
equality carries those references over to the facade.  drake_amd/host/facade_replay.cc replays the script through the
facade; tests/facade_scene.py builds the scene (feature_paths' at its perturbed state, with a weave, tearing with both
couplings, link limits, creases, shell damping and a rest shape added), writes it as raw bytes of the binding's own
tables, and runs the twin."""
import os
import subprocess

import numpy as np
import pytest

from tests import facade_scene as fs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "drake_amd", "host", "facade_replay")


def _replay(mode, scene, tmp_path):
    """the program once, in `mode`, on the scene's file -> [(name, bytes)]"""
    if not os.path.exists(EXE):
        subprocess.check_call(["make", "-C", os.path.dirname(EXE), "-s"])
    scene_file, result_file = str(tmp_path / "scene.blocks"), str(tmp_path / (mode + ".blocks"))
    fs.write_blocks(scene_file, list(scene.items()))
    out = subprocess.run([EXE, mode, scene_file, result_file], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "facade_replay %s ok" % mode in out.stdout
    return [(name, raw) for name, _, _, raw in fs.read_blocks(result_file)]


def _same(replayed, twin):
    """block by block: the list of names, then every block's bytes"""
    twin = [(name, fs._bytes(a)) for name, a in twin]
    assert [n for n, _ in replayed] == [n for n, _ in twin]
    different = [n for (n, a), (_, b) in zip(replayed, twin) if a != b]
    assert not different, different


@pytest.fixture(scope="module")
def scene():
    return fs.build_scene()


@pytest.mark.gpu
def test_replay_through_the_facade_equals_the_binding_to_the_bit(scene, tmp_path):
    replayed = _replay("replay", scene, tmp_path)
    twin = fs.twin(scene)
    _same(replayed, twin)
    blocks = dict(replayed)
    names = {n.split("@")[0] for n in blocks}
    # every public method of GpuMpmState and GpuMpmSolver is behind a block of the list
    assert fs.public_methods(ROOT) == set(fs.METHOD_BLOCKS) | set(fs.NOT_REPLAYED)
    missing = sorted(m for m, b in fs.METHOD_BLOCKS.items() if m not in fs.STATICS and b not in names)
    assert not missing, missing
    # every getter returns the uploaded table to the bit
    for getter, table in (("GetPins", "pins"), ("GetGridBodies", "grid_bodies"), ("GetForceFields", "force_fields"),
                          ("GetBending", "bending"), ("GetDamping", "damping"), ("GetWeave", "weave"), ("GetTearing", "tearing"),
                          ("GetTearCoupling", "tear_coupling"), ("GetRestShape", "rest_shape"), ("GetLinks", "links"),
                          ("GetLinkLimits", "link_limits"), ("GetAnchors", "anchors"), ("GetPressure", "pressure"),
                          ("GetShellBending", "shell"), ("GetShellDamping", "shell_damping"), ("GetCreases", "creases"),
                          ("GetBodyContactMaterials", "contact_materials")):
        assert blocks[getter + "@set"] == fs._bytes(scene[table]), getter
    # ... and what the clearing forms leave: empty tables or zeros, every guard +inf
    for getter in ("GetPins", "GetGridBodies", "GetForceFields", "GetLinks", "GetLinkLimits", "GetAnchors", "GetBodyContactMaterials"):
        assert blocks[getter + "@clear"] == b"", getter
    for getter in ("GetBending", "GetDamping", "GetWeave", "GetTearing", "GetTearCoupling", "GetPressure", "GetShellBending",
                   "GetShellDamping", "GetCreases", "GetRestShape.is_set"):
        assert blocks[getter + "@clear"] and not any(blocks[getter + "@clear"]), getter
    for guard in ("Bending", "Damping", "Weave", "Links", "Anchors", "Shell"):
        assert np.frombuffer(blocks[guard + "MaxStableDt@clear"], np.float32)[0] == np.inf, guard
    # the scene does what it was placed to do: faces of sheet 1 tear and a seam link breaks within the run, hinges yield,
    # the floor is reached; the scissors cut hinges and vent the icosphere
    u32 = lambda name: np.frombuffer(blocks[name], np.uint32)     # noqa: E731
    assert list(u32("TearState.counts@0")) == [0, 0, 0, 0]
    assert u32("TearState.counts@phases")[1] >= fs.N_TORN and not any(u32("TearState.counts@phases")[[0, 2, 3]])
    assert u32("LinkBreakState.count@phases")[0] >= 1
    assert u32("CreaseState.counts@phases")[1] > 0
    assert u32("ShellCutHinges.counts@phases")[1] > 0
    assert np.frombuffer(blocks["GenerateContactPairs"], np.uint64)[0] > 0
    assert list(np.frombuffer(blocks["PressureVented@phases"], np.uint8)) == [0, 0, 0, 0]
    assert list(np.frombuffer(blocks["PressureVented@torn"], np.uint8)) == [0, 0, 1, 0]
    assert u32("ShellCutHinges.counts@torn")[2] > 0
    assert u32("LinkBreakState.count@broken")[0] == 1
    assert not any(u32("CreaseState.counts@ironed")) and blocks["CreaseState@creased"] == blocks["CreaseState@broken"]
    assert np.frombuffer(blocks["AddFixedConstraint"], np.uint64)[0] == 1
    assert len(blocks["GetPins@1"]) == len(blocks["GetPins@set"]) + 20


@pytest.mark.gpu
def test_host_only_statics_equal_the_binding_to_the_bit(tmp_path):
    sc = fs.statics_inputs()
    _same(_replay("statics", sc, tmp_path), fs.statics_twin(sc))


@pytest.mark.gpu
def test_refusals_reach_the_caller_as_runtime_errors_with_the_engines_words(scene, tmp_path):
    replayed = _replay("refusals", scene, tmp_path)
    _same(replayed, fs.refusals_twin(scene))
    for name, raw in replayed:
        if name.startswith("refused."):
            assert raw.startswith(b"mpm_hip: ") and len(raw) > len(b"mpm_hip: "), name
    assert sum(name.startswith("refused.") for name, _ in replayed) == 3


@pytest.mark.gpu
def test_wrong_sizes_throw_and_leave_the_engine_usable(scene, tmp_path):
    replayed = _replay("sizes", scene, tmp_path)
    _same(replayed, fs.sizes_twin(scene))
    assert np.frombuffer(dict(replayed)["wrong_sizes"], np.uint32)[0] == fs.WRONG_SIZE_CALLS
