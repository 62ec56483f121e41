#!/usr/bin/env python3
"""Cost of anchors (mpm_set_anchors): the bench.py workload (cloth_1m, 16 sheets) on three engines -- plain, `edge` (one
anchor per vertex of one edge of every sheet) and `dense` (one anchor per vertex: the worst case, comparable to one link
per vertex in scripts/bench_links.py).  Every anchor is a spring at its rest length to a point of a still body 2 cells
above its vertex, k such that dt is a quarter of mpm_anchors_max_stable_dt, c = 0: k_vforce, k_anchor_pose and k_anchor
run, every record is read and evaluated and every reaction is added, while the trajectory stays close to the plain
engine's.  Per round every engine runs once, in turn, in one process: mpm_profile_substeps' VFORCE phase (event time;
empty on the plain engine, whose vertex forces are summed inside k_p2g), and the whole substep (wall time of
mpm_run_substeps, synchronised at the end).  Medians over the rounds; the raw rounds are printed too.

  python scripts/bench_anchors.py [--steps 40] [--warmup 10] [--rounds 5] [--config cloth_1m] [--engines plain,edge,dense]

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


def anchor_table(sheets, kind, res):
    from drake_amd import ANCHOR_DTYPE
    first = np.cumsum([0] + [len(pos) for pos, _, _ in sheets])
    verts = []
    for s, (pos, _, _) in enumerate(sheets):
        n = len(pos)
        verts.append(first[s] + (np.arange(n) if kind == "dense" else np.arange(min(res, n))))
    verts = np.concatenate(verts)
    x = np.concatenate([np.asarray(pos, np.float32).reshape(-1, 3) for pos, _, _ in sheets])
    t = np.zeros(len(verts), ANCHOR_DTYPE)
    rest = np.float32(2.0 / 128)
    t["vertex"], t["body"], t["stiffness"], t["rest_length"] = verts, 0, 1.0, rest
    t["p_BQ"] = x[verts] + np.array([0, 0, rest], np.float32)       # (the body's frame is the world's: p_WB = 0, R_WB = I)
    return t


def engine(bits, sheets, kind, dt, res):
    from drake_amd import BodyMotion, GpuMpm
    g = GpuMpm(bits)
    for pos, vel, idx in sheets:
        g.add_qr_cloth(pos, vel, idx)
    g.finalize()
    if kind != "plain":
        g.reallocate_external_bodies(1)
        g.set_body_motions([BodyMotion(0)])
        t = anchor_table(sheets, kind, res)
        g.set_anchors(t)
        t["stiffness"] *= np.float32((0.25 * g.anchors_max_stable_dt() / dt) ** 2)   # (the limit scales with 1 / sqrt(k))
        g.set_anchors(t)
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--config", default="cloth_1m")
    ap.add_argument("--dt", type=float, default=1e-3)
    ap.add_argument("--engines", default="plain,edge,dense", help="which of the three engines run (a kernel trace of one)")
    args = ap.parse_args()
    from drake_amd import scenes
    bits, layers, res = scenes.CONFIGS[args.config]
    sheets = scenes.cloth_stack(layers, res, bits)
    kinds = tuple(args.engines.split(","))
    engines = {k: engine(bits, sheets, k, args.dt, res) for k in kinds}
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
        t = g.get_anchors()
        rows.append(dict(engine=k, anchors=int(len(t)), stiffness=float(t["stiffness"][0]) if len(t) else 0.0,
                         max_stable_dt=g.anchors_max_stable_dt(),
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
    print(json.dumps(dict(workload=f"{args.config}: anchors to a rigid body, VFORCE phase and substep", dt=args.dt,
                          steps=args.steps, rounds=args.rounds, rows=rows)))


if __name__ == "__main__":
    main()
