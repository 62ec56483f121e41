"""Runs one small deterministic scene through every host path that enqueues a whole substep (tests/substep_paths.py: the
batched, profiled, phase-by-phase, begin / end, halo and coupled paths; no fan mesh, so k_vforce is not launched) and
prints, per path, a hash of positions, velocities, affine and F with the substep, re-sort and re-sort-check counts.

For checking that a change of the host's launch code leaves every path as it was: run once per library (MPM_HIP_LIBRARY
selects a variant built by scripts/build_history.sh) and compare the lines; under `rocprofv3 --kernel-trace -- python
scripts/substep_paths.py --skip coupled` the ordered list of (kernel, grid, workgroup) must be the same too
(scripts/substep_paths.py --trace-list <kernel_trace.csv> prints it; the coupled path is left out there: its contact solve
enqueues Newton iterations in speculative batches until the host sees the mailbox say "done", so the number of idle
launches at the end of a solve depends on the host's timing).  Results: profiles/substep_paths_ab.txt.

--features: the scene of tests/feature_paths.py instead -- every cloth feature on -- through the fused entry points, the
sums family, the seven calls and run_coupled_substeps; the hash covers the accumulators, the feature states and every
force accessor as well (feature_paths.state)."""
import csv
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def trace_list(path):
    """kernel_trace.csv of rocprofv3 -> one line per dispatch, in start order: name, grid, workgroup"""
    with open(path, newline="") as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))   # (one stream: start order = launch order)
    for r in rows:
        dims = lambda what: "x".join(v for k, v in r.items() if k.startswith(what))
        print(r["Kernel_Name"], dims("Grid_Size"), dims("Workgroup_Size"))


def main(skip=()):
    from tests import substep_paths as sp
    lib = os.path.basename(os.environ.get("MPM_HIP_LIBRARY", "default"))
    for name in sp.PATHS:
        if name in skip:
            continue
        state, st = sp.run(name, fan=False)
        h = hashlib.sha256()
        for k in ("pos", "vel", "C", "F"):
            h.update(state[k].tobytes())
        print(lib, f"{name:28s}", h.hexdigest()[:16], "substeps", st["substeps"], "rebuilds", st["rebuilds"], "resort_checks",
              st["resort_checks"], "err", st["error_flags"], flush=True)


def features():
    from tests import feature_paths as fp
    from tests import substep_paths as sp
    lib = os.path.basename(os.environ.get("MPM_HIP_LIBRARY", "default"))

    def line(name, g):
        st, stats = fp.state(g), g.stats()
        print(lib, f"{name:28s}", fp.state_hash(st), "substeps", stats["substeps"], "rebuilds", stats["rebuilds"], "resort_checks",
              stats["resort_checks"], "err", stats["error_flags"], flush=True)
        g.destroy()

    for name, (runner, env) in fp.FUSED.items():
        g = fp.engine(env=env)
        runner(g, -1)
        line(name, g)
    g = fp.engine()
    sp._begin_end(g)
    line("substep_begin_end", g)
    g = fp.engine()
    fp.seven_calls(g, fp.floor(), fp.N)
    line("seven_calls", g)
    g = fp.engine()
    fp.coupled(g, fp.floor())
    line("coupled", g)


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "--features":
        features()
    elif len(sys.argv) == 3 and sys.argv[1] == "--trace-list":
        trace_list(sys.argv[2])
    elif len(sys.argv) >= 2 and sys.argv[1] == "--skip":
        main(sys.argv[2:])
    else:
        main()
