#!/usr/bin/env python3
"""Cost of external force fields (mpm_set_force_fields): the bench.py workload (cloth_1m, 16 sheets) with no table, one
ACCEL field, a DRAG with an affine wind, a quadratic NORMAL_DRAG in a region, and 8 mixed fields.  Per round every
engine runs once, in turn, in one process: mpm_profile_substeps' P2G phase (k_p2g with or without FIELDS; event time)
and the whole substep (wall time of mpm_run_substeps, synchronised at the end).  Medians over the rounds; the raw
rounds are printed too.

A field changes where the cloth goes, and with it the work of every later substep (sheets that drift sideways or fold
fill their cells and blocks differently).  --neutral keeps every table's shape (kinds, flags, regions, a non-zero G)
and sets the coefficients that act to zero (gamma = 0; ACCEL with u0 = 0 and G = 0): the
kernel does the same work per particle, the trajectory is the plain engine's, and the difference is the evaluation's
cost alone.

  python scripts/bench_force_fields.py [--steps 40] [--warmup 10] [--rounds 5] [--config cloth_1m] [--neutral]

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


def neutral(fields):
    """the same tables adding nothing: drags with gamma = 0, ACCEL fields with u = 0"""
    from drake_amd import FF_ACCEL
    for f in fields:
        f.gamma = 0.0
        if f.kind == FF_ACCEL:
            f.u0[:] = [0.0, 0.0, 0.0]
            f.G[:] = [0.0] * 9
    return fields


def tables():
    from drake_amd import FF_ACCEL, FF_DRAG, FF_NORMAL_DRAG, ForceField
    c = (0.5, 0.5, 0.6)
    shear = [0.0, 2.0, -0.5, 0.8, 0.0, 0.3, -1.2, 0.6, 0.0]
    accel = ForceField(FF_ACCEL, u0=(0.5, -0.3, 0.0))
    drag = ForceField(FF_DRAG, gamma=2.0, u0=(0.3, 0.1, 0.0), G=shear, x0=c)
    normal = ForceField(FF_NORMAL_DRAG, gamma=5.0, u0=(0.0, 0.0, 0.5), quadratic=True, region=((0.3, 0.3, 0.0), (0.6, 0.7, 1.0)))
    eight = [accel, drag, normal, ForceField(FF_NORMAL_DRAG, gamma=3.0, u0=(0.1, 0.0, 0.2)),
             ForceField(FF_ACCEL, G=[-4.0, 0, 0, 0, -4.0, 0, 0, 0, 0], x0=c), ForceField(FF_DRAG, gamma=1.0, region=((0.0, 0.0, 0.0), (0.5, 1.0, 1.0))),
             ForceField(FF_ACCEL, u0=(0.0, 0.2, 0.0), region=((0.4, 0.0, 0.0), (1.0, 1.0, 1.0))),
             ForceField(FF_NORMAL_DRAG, gamma=2.0, G=shear, x0=c, quadratic=True)]
    return {"none": [], "accel": [accel], "drag_wind": [drag], "normal_quadratic_region": [normal], "eight": eight}


def engine(bits, sheets, fields):
    from drake_amd import GpuMpm
    g = GpuMpm(bits)
    for pos, vel, idx in sheets:
        g.add_qr_cloth(pos, vel, idx)
    g.finalize()
    if fields:
        g.set_force_fields(fields)
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--config", default="cloth_1m")
    ap.add_argument("--dt", type=float, default=1e-3)
    ap.add_argument("--neutral", action="store_true", help="tables of the same shape that add nothing (see above)")
    args = ap.parse_args()
    from drake_amd import scenes
    bits, layers, res = scenes.CONFIGS[args.config]
    sheets = scenes.cloth_stack(layers, res, bits)
    variants = tables()
    if args.neutral:
        variants = {k: neutral(f) for k, f in variants.items()}
    engines = {k: engine(bits, sheets, f) for k, f in variants.items()}
    for g in engines.values():
        g.run_substeps(args.warmup, args.dt, -1)
        g.gpu_sync()
    samples = {k: dict(p2g_us=[], phases=[], substep_us=[]) for k in variants}
    for _ in range(args.rounds):
        for k in variants:
            g = engines[k]
            ph, _ = g.profile_substeps(args.steps, args.dt, -1)
            samples[k]["p2g_us"].append(ph["p2g"] * 1e3)
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
        rows.append(dict(table=k, fields=len(variants[k]), p2g_us=round(float(np.median(s["p2g_us"])), 2),
                         phases_us={p: round(float(np.median([d[p] for d in s["phases"]])) * 1e3, 2) for p in s["phases"][0]},
                         substep_us=round(float(np.median(s["substep_us"])), 2),
                         p2g_us_rounds=[round(float(x), 2) for x in s["p2g_us"]],
                         substep_us_rounds=[round(float(x), 2) for x in s["substep_us"]], error_flags=int(st["error_flags"])))
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    base = rows[0]
    for r in rows[1:]:
        r["p2g_ratio"] = round(r["p2g_us"] / base["p2g_us"], 4)
        r["substep_ratio"] = round(r["substep_us"] / base["substep_us"], 4)
    for g in engines.values():
        g.destroy()
    print(json.dumps(dict(workload=f"{args.config}: force fields, P2G phase and substep", dt=args.dt,
                          steps=args.steps, rounds=args.rounds, neutral=bool(args.neutral), rows=rows)))


if __name__ == "__main__":
    main()
