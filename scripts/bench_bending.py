#!/usr/bin/env python3
"""Cost of bending stiffness (mpm_set_bending): the bench.py workload (cloth_1m, 16 sheets) on three engines -- plain,
`neutral` (every cloth with the smallest positive normal float as stiffness: k_vforce and k_bend run, the table is read,
the trajectory is the plain engine's) and `stiff` (k such that dt is a quarter of mpm_bending_max_stable_dt).  Per round
every engine runs once, in turn, in one process: mpm_profile_substeps' VFORCE phase (k_vforce + k_bend on an engine with
bending, empty on the plain one, whose vertex forces are summed inside k_p2g; event time), its P2G phase, and the whole
substep (wall time of mpm_run_substeps, synchronised at the end).  Medians over the rounds; the raw rounds are printed
too.

  python scripts/bench_bending.py [--steps 40] [--warmup 10] [--rounds 5] [--config cloth_1m]

Prints one JSON record.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

TINY = float(np.finfo(np.float32).tiny)


def engine(bits, sheets, kind, dt):
    from drake_amd import GpuMpm
    g = GpuMpm(bits)
    for pos, vel, idx in sheets:
        g.add_qr_cloth(pos, vel, idx)
    g.finalize()
    n = g.cloth_count()
    if kind == "neutral":
        g.set_bending([TINY] * n)
    elif kind == "stiff":
        g.set_bending([1.0] * n)
        k = (0.25 * g.bending_max_stable_dt() / dt) ** 2     # (the limit scales with 1 / sqrt(k))
        g.set_bending([k] * n)
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--config", default="cloth_1m")
    ap.add_argument("--dt", type=float, default=1e-3)
    args = ap.parse_args()
    from drake_amd import scenes
    bits, layers, res = scenes.CONFIGS[args.config]
    sheets = scenes.cloth_stack(layers, res, bits)
    kinds = ("plain", "neutral", "stiff")
    engines = {k: engine(bits, sheets, k, args.dt) for k in kinds}
    for g in engines.values():
        g.run_substeps(args.warmup, args.dt, -1)
        g.gpu_sync()
    samples = {k: dict(phases=[], substep_us=[]) for k in kinds}
    for _ in range(args.rounds):
        for k in kinds:
            g = engines[k]
            ph, _ = g.profile_substeps(args.steps, args.dt, -1)
            samples[k]["phases"].append(ph)
            g.gpu_sync()
            t0 = time.perf_counter()
            g.run_substeps(args.steps, args.dt, -1)
            g.gpu_sync()
            samples[k]["substep_us"].append((time.perf_counter() - t0) * 1e6 / args.steps)
    rows = []
    for k in kinds:
        s, g = samples[k], engines[k]
        st = g.stats()
        rows.append(dict(engine=k, stiffness=float(g.get_bending()[0]), max_stable_dt=g.bending_max_stable_dt(),
                         vforce_us=round(float(np.median([d["vforce"] for d in s["phases"]])) * 1e3, 2),
                         phases_us={p: round(float(np.median([d[p] for d in s["phases"]])) * 1e3, 2) for p in s["phases"][0]},
                         substep_us=round(float(np.median(s["substep_us"])), 2),
                         vforce_us_rounds=[round(d["vforce"] * 1e3, 2) for d in s["phases"]],
                         substep_us_rounds=[round(float(x), 2) for x in s["substep_us"]], error_flags=int(st["error_flags"])))
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    base = rows[0]
    for r in rows[1:]:
        r["substep_ratio"] = round(r["substep_us"] / base["substep_us"], 4)
    for g in engines.values():
        g.destroy()
    print(json.dumps(dict(workload=f"{args.config}: bending stiffness, VFORCE phase and substep", dt=args.dt,
                          steps=args.steps, rounds=args.rounds, rows=rows)))


if __name__ == "__main__":
    main()
