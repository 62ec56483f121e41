"""Host-side pieces of bench.py that need no GPU: byte accounting and the committed PMC summary."""
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_algorithmic_bytes_follow_survey_8d():
    b = _bench()
    np_, nf, nv, nc = 999952, 663552, 336400, 64 * 972
    ab = b.algorithmic_bytes(np_, nf, nv, nc)
    # B = 188 Np + 200 Nf + 36 Nv + 68 Nc
    assert ab["total"] == 188 * np_ + 200 * nf + 36 * nv + 68 * nc
    assert ab["fem"] + ab["vforce"] == 200 * nf + 36 * nv
    names = b.kernel_names(False, False)
    assert set(names) == {"fem", "vforce", "p2g", "grid", "g2p"}
    # the instantiations a run launches, as rocprofv3 prints them
    assert names["fem"] == "mpm::k_fem<0>" and b.kernel_names(True, False)["fem"] == "mpm::k_fem<1>"
    assert names["p2g"].startswith("mpm::k_p2g<1, ") and b.kernel_names(False, True)["grid"] == "mpm::k_grid<2>"


def test_committed_pmc_summary_feeds_the_roofline_traffic():
    b = _bench()
    with open(os.path.join(ROOT, "profiles", "pmc_traffic.json")) as f:
        t = json.load(f)
    assert t["config"] == "cloth_1m" and os.path.exists(os.path.join(ROOT, t["source"]))
    names = b.kernel_names(False, False)
    for k in names.values():
        if k == "mpm::k_vforce":
            # the single-GPU command the passes profile does not launch it: k_p2g gathers the vertex forces of
            # its work items itself (mpm_run_substeps), and its traffic below includes that work
            assert k not in t["kernels"] and b.measured_traffic(k, "cloth_1m") is None
            continue
        rec = t["kernels"][k]     # (the profiles are collected with the code that ships: the names match exactly)
        assert rec["hbm_bytes_per_launch"] > 0 and rec["launches"] > 0
        assert abs(rec["hbm_bytes_per_launch"] - (rec["read_bytes"] + rec["write_bytes"])) < 1.0
        assert b.measured_traffic(k, "cloth_1m") == rec["hbm_bytes_per_launch"]
    assert b.measured_traffic(names["p2g"], "some_other_config") is None
    # the dominant kernel must not move (much) more than its algorithmic bytes (SURVEY 8d's P2G row: the vertices' x, v, f
    # are in its 116 B per particle)
    ab = b.algorithmic_bytes(999952, 663552, 336400, 64 * 972)
    assert t["kernels"][names["p2g"]]["hbm_bytes_per_launch"] < 1.2 * ab["p2g"]
    # ... and the committed SQ counters of the same command feed roofline.valu_issue_ms
    with open(os.path.join(ROOT, "profiles", "sq_counters.json")) as f:
        q = json.load(f)
    assert q["config"] == "cloth_1m" and q["head"] == t["head"]
    assert b.measured_sq(names["p2g"], "cloth_1m")["SQ_INSTS_VALU"] > 1e6


def test_gpus_flag_launches_that_many_ranks():
    """`python bench.py --gpus N` (how the driver calls it) must become N rank processes with the
    torch.distributed environment set; rank 0 alone prints to stdout."""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "3", "--launcher-selftest"],
                         capture_output=True, text=True, timeout=120, env=env)
    assert out.returncode == 0, out.stderr
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    got = json.loads(lines[0])
    assert got["WORLD_SIZE"] == "3" and got["RANK"] == "0" and got["LOCAL_RANK"] == "0" and got["n_gpus"] == 3
    assert got["MASTER_ADDR"] == "127.0.0.1" and int(got["MASTER_PORT"]) > 0
    # a failing rank fails the launch
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--no-such-flag"],
                         capture_output=True, text=True, timeout=120, env=env)
    assert bad.returncode != 0


class _FakeEngine:
    """download() of a tiny engine whose slots are a shuffle of the particle ids"""

    def __init__(self, n_particles, n_faces):
        import numpy as np
        from drake_amd import ARR
        self.pids = np.random.default_rng(7).permutation(n_particles).astype(np.int32)
        ids = self.pids.astype(np.float32)[:, None]
        self.arrays = {ARR.PIDS: self.pids, ARR.POSITIONS: ids * np.float32([1, 2, 3]),
                       ARR.VELOCITIES: -ids * np.float32([1, 1, 1]),
                       ARR.DEFORMATION_GRADIENTS: np.arange(n_faces * 9, dtype=np.float32).reshape(n_faces, 9)}

    def download(self, which):
        return self.arrays[which].copy()


def test_dump_outputs_writes_particles_in_id_order(tmp_path):
    import numpy as np
    b = _bench()
    g = _FakeEngine(100, 40)
    info = b.dump_outputs(g, str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["deformation_gradients.npy", "positions.npy", "velocities.npy"]
    pos, vel, F = (np.load(tmp_path / f"{n}.npy") for n in ("positions", "velocities", "deformation_gradients"))
    assert pos.dtype == vel.dtype == F.dtype == np.float32
    ids = np.arange(100, dtype=np.float32)[:, None]
    np.testing.assert_array_equal(pos, ids * np.float32([1, 2, 3]))
    np.testing.assert_array_equal(vel, -ids * np.float32([1, 1, 1]))
    np.testing.assert_array_equal(F, np.arange(360, dtype=np.float32).reshape(40, 9))
    assert info["sample_seed"] is None and info["arrays"]["positions"]["shape"] == [100, 3]


def test_dump_outputs_samples_the_same_rows_under_the_limit(tmp_path):
    import numpy as np
    b = _bench()
    g = _FakeEngine(1000, 500)
    limit = 8000   # of 12000 + 12000 + 18000 bytes
    first, second = tmp_path / "a", tmp_path / "b"
    b.dump_outputs(g, str(first), limit=limit)
    b.dump_outputs(_FakeEngine(1000, 500), str(second), limit=limit)
    total = 0
    for n in ("positions", "velocities", "deformation_gradients"):
        x, y = np.load(first / f"{n}.npy"), np.load(second / f"{n}.npy")
        np.testing.assert_array_equal(x, y)
        total += x.nbytes
    assert 0 < total <= limit
    pos = np.load(first / "positions.npy")
    assert np.all(np.diff(pos[:, 0]) > 0)   # a subset of the ids, ascending
    np.testing.assert_array_equal(pos[:, 1], 2 * pos[:, 0])
