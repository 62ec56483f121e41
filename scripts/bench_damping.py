#!/usr/bin/env python3
"""Cost of stiffness-proportional damping (mpm_set_damping): the bench.py workload (cloth_1m, 16 sheets) on four engines
in one process -- `plain` (the feature off: the kernels every engine ran before it existed), `membrane` (beta_membrane
such that dt is a quarter of mpm_damping_max_stable_dt: k_damp behind k_fem), `bend` (bending stiffness at a quarter of
its limit, no damping: k_vforce + k_bend) and `bend_damped` (the same with both coefficients at a quarter of the damping
limit: k_damp and k_bend_damp too).  Per round every engine runs once, in turn: mpm_profile_substeps' FEM and VFORCE
phases (event times) and the whole substep (wall time of mpm_run_substeps, synchronised at the end).  Medians over the
rounds; the raw rounds are printed too.  k_damp's time is FEM(membrane) - FEM(plain), k_bend_damp's is
VFORCE(bend_damped) - VFORCE(bend); their algorithmic bytes (counted below from the kernels' loads and stores) over
those times are set against HBM's 8 TB/s.

  python scripts/bench_damping.py [--steps 40] [--warmup 10] [--rounds 5] [--config cloth_1m]

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

HBM_PEAK_GBS = 8000.0
# k_damp per face: the static records fq[2], fq[3] (32), PSet::pid (4), the cloth byte (1); six 16-byte gathers of corner
# positions and velocities (96; 48 if the in-plane columns k_fem stored were read instead of the positions); three 12-byte
# records read and written (72).  The per-cloth coefficient record stays in cache.
DAMP_BYTES_PER_FACE = 32 + 4 + 1 + 96 + 72   # (the cloth index is an int; one byte of it is needed)
# k_bend_damp per row: row id and slot (8), own velocity (16), per entry the record (8), the column's slot (4) and its
# velocity (16); the force read and written (24)
BEND_DAMP_BYTES = lambda rows, entries: rows * (8 + 16 + 24) + entries * (8 + 4 + 16)   # noqa: E731


def engine(bits, sheets, kind, dt):
    from drake_amd import GpuMpm
    g = GpuMpm(bits)
    for pos, vel, idx in sheets:
        g.add_qr_cloth(pos, vel, idx)
    g.finalize()
    n = g.cloth_count()
    if kind in ("bend", "bend_damped"):
        g.set_bending([1.0] * n)
        k = (0.25 * g.bending_max_stable_dt() / dt) ** 2     # (the limit scales with 1 / sqrt(k))
        g.set_bending([k] * n)
    on = dict(membrane=(1.0, 0.0), bend_damped=(1.0, 1.0)).get(kind)
    if on:
        g.set_damping([on] * n)
        c = 0.25 * g.damping_max_stable_dt() / dt            # (the limit scales with 1 / beta)
        g.set_damping([(on[0] * c, on[1] * c)] * n)
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--config", default="cloth_1m")
    ap.add_argument("--dt", type=float, default=1e-3)
    args = ap.parse_args()
    from drake_amd import bending_matrix, scenes
    bits, layers, res = scenes.CONFIGS[args.config]
    sheets = scenes.cloth_stack(layers, res, bits)
    kinds = ("plain", "membrane", "bend", "bend_damped")
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
    rows = {}
    for k in kinds:
        s, g = samples[k], engines[k]
        rows[k] = dict(engine=k, damping=[float(x) for x in g.get_damping()[0]], bending=float(g.get_bending()[0]),
                       max_stable_dt=g.damping_max_stable_dt(),
                       phases_us={p: round(float(np.median([d[p] for d in s["phases"]])) * 1e3, 2) for p in s["phases"][0]},
                       substep_us=round(float(np.median(s["substep_us"])), 2),
                       fem_us_rounds=[round(d["fem"] * 1e3, 2) for d in s["phases"]],
                       vforce_us_rounds=[round(d["vforce"] * 1e3, 2) for d in s["phases"]],
                       substep_us_rounds=[round(float(x), 2) for x in s["substep_us"]], error_flags=int(g.stats()["error_flags"]))
        print(json.dumps(rows[k]), file=sys.stderr, flush=True)
    nf, nv = engines["plain"].n_faces, engines["plain"].n_verts
    off, _, _ = bending_matrix(sheets[0][0], sheets[0][2])
    entries = (int(off[-1]) - len(sheets[0][0])) * len(sheets)          # off-diagonal entries of the whole table
    k_damp_us = rows["membrane"]["phases_us"]["fem"] - rows["plain"]["phases_us"]["fem"]
    k_bend_damp_us = rows["bend_damped"]["phases_us"]["vforce"] - rows["bend"]["phases_us"]["vforce"]
    cost = dict(faces=nf, vertices=nv,
                k_damp=dict(us=round(k_damp_us, 2), bytes=nf * DAMP_BYTES_PER_FACE, bytes_per_face=DAMP_BYTES_PER_FACE,
                            hbm_fraction=round(nf * DAMP_BYTES_PER_FACE / (k_damp_us * 1e-6) / (HBM_PEAK_GBS * 1e9), 4)
                            if k_damp_us > 0 else None,
                            k_fem_us=rows["plain"]["phases_us"]["fem"],
                            k_damp_us_under_bending=round(rows["bend_damped"]["phases_us"]["fem"] - rows["bend"]["phases_us"]["fem"], 2)),
                k_bend_damp=dict(us=round(k_bend_damp_us, 2), bytes=BEND_DAMP_BYTES(nv, entries), table_entries=entries,
                                 hbm_fraction=round(BEND_DAMP_BYTES(nv, entries) / (k_bend_damp_us * 1e-6) / (HBM_PEAK_GBS * 1e9), 4)
                                 if k_bend_damp_us > 0 else None))
    for k in kinds[1:]:
        rows[k]["substep_ratio"] = round(rows[k]["substep_us"] / rows["plain"]["substep_us"], 4)
    for g in engines.values():
        g.destroy()
    print(json.dumps(dict(workload=f"{args.config}: stiffness-proportional damping, FEM and VFORCE phases and substep", dt=args.dt,
                          steps=args.steps, rounds=args.rounds, rows=[rows[k] for k in kinds], cost=cost)))


if __name__ == "__main__":
    main()
