#!/usr/bin/env python3
"""A/B of the contact solve with and without per-body contact materials, interleaved on one box:

  python scripts/bench_contact_materials.py --parent <libmpm_hip.so of the parent commit> [--rounds 5] [--out FILE]

Every round runs, each in a process of its own (the library is bound once per process; MPM_HIP_LIBRARY selects it):
  parent    the parent commit's library
  none      this commit's library, no table set (the path that must cost what the parent's costs)
  uniform   this commit's library with a 1-entry table equal to the call's scalars (the per-contact planes in use)
and in each of them
  * scripts/bench_contact.py --survey-config3 --device-pairs (config 3: 1M particles on a floor, k = 1e6, d = 1e-5, mu = 1,
    dt = 2e-4): solve time per Newton iteration, solve time per substep;
  * the coupled path of bench.py's contact leg (the same scene through mpm_run_coupled_substeps, restated here so that
    the table is set explicitly): iteration_ms (the four kernels of an iteration, HIP events), ms_per_substep and
    ms_beyond_iterations = ms_per_substep - iterations x iteration_ms, over the impact and on the settled stack.
Prints the raw figures of every run and the median and range per variant."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child_leg(table, steps=20, warmup=5):
    """the coupled path of bench.py's contact leg (same scene, parameters, windows and figures: mpm_run_coupled_substeps
    over the impact and over the settled stack, then the four kernels of an iteration by HIP events), with the table set
    explicitly on the engine"""
    import time
    sys.path.insert(0, ROOT)
    import numpy as np
    from drake_amd import Collider, GpuMpm, scenes
    bits, layers, res = scenes.CONFIGS["cloth_1m"]
    floor_z, k, d, mu, dt = 0.25, 1e6, 1e-5, 1.0, 2e-4
    floor = (Collider * 1)(Collider(0, body=0, p_WB=(0.5, 0.5, floor_z)))
    g = GpuMpm(bits, device=0)
    sheets = scenes.cloth_stack(layers, res, bits, z0=floor_z - 0.004)
    for pos, vel, idx in sheets:
        vel[:, 2] -= 0.5
    scenes.populate(g, sheets)
    g.reallocate_external_bodies(1)
    if table:
        g.set_body_contact_materials([(mu, k, d)])

    def window(first, count):
        if first:
            g.run_coupled_substeps(first, dt, floor, mu, k, d)
        g.gpu_sync()
        t0 = time.perf_counter()
        rs = g.run_coupled_substeps(count - first, dt, floor, mu, k, d)
        g.gpu_sync()
        return (time.perf_counter() - t0) / steps * 1e3, float(np.mean([r["iterations"] for r in rs]))

    ms, its = window(warmup, warmup + steps)
    ms_s, its_s = window(100, 100 + steps)
    g.rebuild_mapping(False)
    g.calc_fem_state_and_force(dt)
    g.particle_to_grid(dt)
    g.update_grid(-1)
    g.generate_contact_pairs(floor)
    g.update_contact(dt, mu, k, d)
    kms = g.profile_contact_iteration(20)
    g.grid_to_particle(dt)
    assert g.stats()["error_flags"] == 0
    g.destroy()
    it_ms = sum(kms.values())
    print(json.dumps(dict(iteration_ms=it_ms, kernel_ms=kms, ms_per_substep=ms, newton_iterations=its,
                          ms_beyond_iterations=ms - its * it_ms, settled_ms_per_substep=ms_s,
                          settled_ms_beyond_iterations=ms_s - its_s * it_ms)))


def last_json(text):
    for ln in reversed(text.strip().splitlines()):
        if ln.startswith("{"):
            return json.loads(ln)
    raise RuntimeError("no JSON line in:\n" + text[-2000:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="the parent commit's libmpm_hip.so (required: without it there is no A)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out")
    ap.add_argument("--child-leg", choices=["plain", "table"])
    args = ap.parse_args()
    if args.child_leg:
        return child_leg(args.child_leg == "table")
    if not args.parent or not os.path.exists(args.parent):
        ap.error("--parent: the parent commit's library is needed")
    variants = [("parent", args.parent, False), ("none", None, False), ("uniform", None, True)]
    rows = {v[0]: [] for v in variants}
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    for rnd in range(args.rounds):
        for name, lib, table in variants:
            env = dict(os.environ)
            env.pop("MPM_HIP_LIBRARY", None)
            if lib:
                env["MPM_HIP_LIBRARY"] = os.path.abspath(lib)
            cmd = [sys.executable, os.path.join(ROOT, "scripts", "bench_contact.py"), "--survey-config3", "--device-pairs"]
            # (the parent's library has no table to set: its script is this one without the option)
            a = last_json(subprocess.run(cmd + (["--uniform-table"] if table else []), env=env, capture_output=True, text=True,
                                         check=True, timeout=600).stdout)
            b = last_json(subprocess.run([sys.executable, os.path.abspath(__file__), "--child-leg", "table" if table else "plain"],
                                         env=env, capture_output=True, text=True, check=True, timeout=600).stdout)
            row = dict(solve_us_per_iteration=a["solve_us_per_iteration"], solve_ms_per_substep=a["ms_per_substep"]["solve"],
                       bench_contact_iterations=a["newton_iterations_mean"], **b)
            rows[name].append(row)
            say(f"round {rnd} {name:8s} " + json.dumps(row))
    say("")
    keys = ("solve_us_per_iteration", "solve_ms_per_substep", "iteration_ms", "ms_per_substep", "ms_beyond_iterations",
            "settled_ms_per_substep", "settled_ms_beyond_iterations")
    say(f"{'figure':30s} " + " ".join(f"{n + ' median [min, max]':>36s}" for n, _, _ in variants))
    for k in keys:
        cells = []
        for n, _, _ in variants:
            v = [r[k] for r in rows[n]]
            cells.append(f"{statistics.median(v):12.4f} [{min(v):9.4f}, {max(v):9.4f}]")
        say(f"{k:30s} " + " ".join(f"{c:>36s}" for c in cells))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
