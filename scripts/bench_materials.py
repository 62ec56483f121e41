#!/usr/bin/env python3
"""Cost of per-cloth materials (mpm_add_qr_cloth_with_material): the bench.py workload (cloth_1m, 16 sheets) with the
sheets given 1, 2 and 4 distinct materials, against the plain engine.  Per round every engine runs once, in turn, in one
process: mpm_profile_substeps' FEM phase (k_fem or k_fem_mat; event time) and the whole substep (wall time of
mpm_run_substeps, synchronised at the end).  Medians over the rounds.

  python scripts/bench_materials.py [--steps 40] [--warmup 10] [--rounds 5] [--config cloth_1m]

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


def materials(k):
    """k distinct materials around the engine's defaults (E, K, gamma, rho and c_F vary; nu stays in range)"""
    from drake_amd import ClothMaterial
    return [ClothMaterial(4e5 * (1 + 0.25 * j), 0.3 - 0.02 * j, 2000.0 * (1 + 0.5 * j), 0.0, 1e5 * (1 + 0.5 * j), 0.0)
            for j in range(k)]


def engine(bits, sheets, n_materials):
    from drake_amd import GpuMpm
    g = GpuMpm(bits)
    mats = materials(n_materials) if n_materials else None
    for s, (pos, vel, idx) in enumerate(sheets):
        g.add_qr_cloth(pos, vel, idx, material=mats[s % len(mats)] if mats else None)
    g.finalize()
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
    variants = [0, 1, 2, 4]   # 0: plain engine (k_fem)
    engines = {k: engine(bits, sheets, k) for k in variants}
    for g in engines.values():
        g.run_substeps(args.warmup, args.dt, -1)
        g.gpu_sync()
    samples = {k: dict(fem_us=[], phases=[], substep_us=[]) for k in variants}
    for _ in range(args.rounds):
        for k in variants:
            g = engines[k]
            ph, _ = g.profile_substeps(args.steps, args.dt, -1)
            samples[k]["fem_us"].append(ph["fem"] * 1e3)
            samples[k]["phases"].append(ph)
            g.gpu_sync()
            t0 = time.perf_counter()
            g.run_substeps(args.steps, args.dt, -1)
            g.gpu_sync()
            samples[k]["substep_us"].append((time.perf_counter() - t0) * 1e6 / args.steps)
    rows = []
    for k in variants:
        s = samples[k]
        st = engines[k].stats()
        rows.append(dict(materials=k or "plain", fem_us=round(float(np.median(s["fem_us"])), 2),
                         phases_us={p: round(float(np.median([d[p] for d in s["phases"]])) * 1e3, 2) for p in s["phases"][0]},
                         substep_us=round(float(np.median(s["substep_us"])), 2), error_flags=int(st["error_flags"])))
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    base = rows[0]
    for r in rows[1:]:
        r["fem_ratio"] = round(r["fem_us"] / base["fem_us"], 4)
        r["substep_ratio"] = round(r["substep_us"] / base["substep_us"], 4)
    for g in engines.values():
        g.destroy()
    print(json.dumps(dict(workload=f"{args.config}: per-cloth materials, FEM phase and substep", dt=args.dt,
                          steps=args.steps, rounds=args.rounds, rows=rows)))


if __name__ == "__main__":
    main()
