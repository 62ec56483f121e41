#!/usr/bin/env python3
"""Cost of fixed constraints (mpm_set_pins): the bench.py workload (BASELINE.json configs[1], ~1M particles) timed per
substep with 0, 1k and 100k pinned vertices, on a static and on a moving (translating and rotating) body.

  python scripts/bench_pins.py [--steps 40] [--warmup 10] [--config cloth_1m] [--pins 0,1000,100000]

Prints one JSON record.  Under `rocprofv3 --kernel-trace --stats -- python scripts/bench_pins.py ...` the kernel table
gives k_pin's own duration; `ms_per_substep` here is wall time per substep of mpm_run_substeps, synchronised at the end.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def rot(a):
    a = np.asarray(a, np.float64)
    th = float(np.linalg.norm(a))
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    if th < 1e-12:
        return np.eye(3)
    return np.eye(3) + np.sin(th) / th * K + (1.0 - np.cos(th)) / (th * th) * (K @ K)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--config", default="cloth_1m")
    ap.add_argument("--dt", type=float, default=1e-3)
    ap.add_argument("--pins", default="0,1000,100000", help="comma-separated pin counts")
    args = ap.parse_args()
    from drake_amd import BodyMotion, GpuMpm, MpmError, Pin, scenes
    bits, layers, res = scenes.CONFIGS[args.config]
    rows = []
    for n_pins in [int(s) for s in args.pins.split(",")]:
        for moving in ((False,) if n_pins == 0 else (False, True)):
            g = GpuMpm(bits)
            scenes.populate(g, scenes.cloth_stack(layers, res, bits))
            g.reallocate_external_bodies(1)
            x, _ = g.dump_cpu_state()
            nv = x.shape[0]
            if n_pins:
                # the first n vertices of the numbering: whole rows of the first sheets, clamped as a block (a rod along one
                # edge, a gripper).  (Every k-th vertex of the whole stack held still while the rest falls is a stiff and
                # unstable constraint pattern at this resolution, on the host model too.)
                verts = np.arange(min(n_pins, nv))
                p = x[verts].mean(axis=0).astype(np.float64)
                q = x[verts].astype(np.float64) - p
                arr = (Pin * len(verts))(*[Pin(int(v), 0, q[k]) for k, v in enumerate(verts)])
                g.set_pins(arr)
                v, w = ((0.02, 0.0, 0.0), (0.0, 0.0, 0.2)) if moving else ((0, 0, 0), (0, 0, 0))
                g.set_body_motions([BodyMotion(0, p, rot((0, 0, 0)).ravel(), v, w)])
            row = dict(pins=int(n_pins and min(n_pins, nv)), moving=moving)
            try:
                g.run_substeps(args.warmup, args.dt, -1)
                g.gpu_sync()
                t0 = time.perf_counter()
                g.run_substeps(args.steps, args.dt, -1)
                g.gpu_sync()
                row["ms_per_substep"] = round((time.perf_counter() - t0) * 1e3 / args.steps, 4)
            except MpmError as e:   # (an engine error, e.g. MPM_ERR_DOMAIN: reported, the next row gets a new engine)
                row["error"] = str(e)
            st = g.stats()
            row.update(rebuilds=int(st["rebuilds"]), error_flags=int(st["error_flags"]))
            rows.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
            g.destroy()
    base = next((r.get("ms_per_substep") for r in rows if r["pins"] == 0), None)
    for r in rows:
        if base is not None and "ms_per_substep" in r:
            r["delta_us_per_substep"] = round((r["ms_per_substep"] - base) * 1e3, 2)
    print(json.dumps(dict(workload=f"{args.config}: mpm_run_substeps with pinned vertices", dt=args.dt, steps=args.steps,
                          rows=rows)))


if __name__ == "__main__":
    main()
