#!/usr/bin/env python3
"""Cost of the enclosed-volume pressure (mpm_set_pressure) on two scenes:

  sheets   the bench.py workload (cloth_1m, 16 open sheets): `plain` against `constant` (every sheet under a constant
           pressure of 1 Pa: k_vforce and k_pressure run over every vertex, the trajectory stays close to the plain one)
  spheres  128 icospheres of four subdivisions (2562 vertices, 5120 faces each: 327,936 vertices, close to cloth_1m's
           336,400) of radius 0.05 on a lattice at domain_bits 7, without gravity: `plain` against `constant` (1 Pa) against `gas` (an
           isothermal gas at 1.001 x p_ambient = 1000 Pa in every sphere: k_pressure_volume and k_pressure_gauge run too)

Per round every engine of a scene runs once, in turn, in one process: mpm_profile_substeps' VFORCE phase (k_vforce and
the pressure kernels on an engine with pressure, empty on the plain one, whose vertex forces are summed inside k_p2g;
event time), and the whole substep (wall time of mpm_run_substeps, synchronised at the end).  Medians over the rounds;
the raw rounds are printed too.

  python scripts/bench_pressure.py [--steps 40] [--warmup 10] [--rounds 5] [--scenes sheets,spheres] [--engines ...]

Prints one JSON record.
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def icosphere(centre, radius, subdivisions):
    t = (1 + math.sqrt(5)) / 2
    V = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    F = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    V = [np.array(v, np.float64) / np.linalg.norm(v) for v in V]
    for _ in range(subdivisions):
        mid, out = {}, []
        for a, b, c in F:
            m = []
            for p, q in ((a, b), (b, c), (c, a)):
                key = (min(p, q), max(p, q))
                if key not in mid:
                    w = V[p] + V[q]
                    V.append(w / np.linalg.norm(w))
                    mid[key] = len(V) - 1
                m.append(mid[key])
            out += [(a, m[0], m[2]), (b, m[1], m[0]), (c, m[2], m[1]), (m[0], m[1], m[2])]
        F = out
    X, T = np.array(V) * radius, np.array(F, np.int32)
    if (X[T[:, 0]] * np.cross(X[T[:, 1]], X[T[:, 2]])).sum() < 0:
        T = T[:, [0, 2, 1]].copy()
    return (X + centre).astype(np.float32), T


def spheres():
    X0, T = icosphere((0.0, 0.0, 0.0), 0.05, 4)
    out = []
    for i in range(8):
        for j in range(4):
            for k in range(4):
                X = (X0 + np.array([0.115 + 0.11 * i, 0.335 + 0.11 * j, 0.335 + 0.11 * k], np.float32)).astype(np.float32)
                out.append((X, np.zeros_like(X), T))
    return out


def volume(X, T):
    x = X.astype(np.float64)
    return float((x[T[:, 0]] * np.cross(x[T[:, 1]], x[T[:, 2]])).sum()) / 6.0


def engine(bits, cloths, kind, gravity):
    from drake_amd import GpuMpm, PRESSURE_DTYPE, PRESSURE_CONSTANT, PRESSURE_GAS
    mat = GpuMpm.default_material()
    if not gravity:
        mat.gravity = 0.0          # (the spheres float: 400 substeps of free fall would land them on the floor)
    g = GpuMpm(bits, mat)
    for pos, vel, idx in cloths:
        g.add_qr_cloth(pos, vel, idx)
    g.finalize()
    if kind != "plain":
        t = np.zeros(len(cloths), PRESSURE_DTYPE)
        if kind == "constant":
            t["mode"], t["p"] = PRESSURE_CONSTANT, 1.0
        else:
            t["mode"], t["p_ambient"], t["p_max"] = PRESSURE_GAS, 1000.0, 2000.0
            t["pv"] = [1001.0 * volume(np.asarray(pos, np.float32).reshape(-1, 3), np.asarray(idx).reshape(-1, 3)) for pos, _, idx in cloths]
        g.set_pressure(t)
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--dt", type=float, default=1e-3)
    ap.add_argument("--scenes", default="sheets,spheres")
    ap.add_argument("--engines", default="plain,constant,gas", help="which engines run (a kernel trace of one); sheets have no gas")
    args = ap.parse_args()
    from drake_amd import scenes
    records = []
    for scene in args.scenes.split(","):
        if scene == "sheets":
            bits, layers, res = scenes.CONFIGS["cloth_1m"]
            cloths = scenes.cloth_stack(layers, res, bits)
        else:
            bits, cloths = 7, spheres()
        kinds = tuple(k for k in args.engines.split(",") if not (scene == "sheets" and k == "gas"))
        engines = {k: engine(bits, cloths, k, scene == "sheets") for k in kinds}
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
            ps = g.pressure_state()
            rows.append(dict(scene=scene, engine=k, cloths=len(cloths), vertices=int(g.n_verts), faces=int(g.n_faces),
                             vforce_us=round(float(np.median([d["vforce"] for d in s["phases"]])) * 1e3, 2),
                             phases_us={p: round(float(np.median([d[p] for d in s["phases"]])) * 1e3, 2) for p in s["phases"][0]},
                             substep_us=round(float(np.median(s["substep_us"])), 2),
                             vforce_us_rounds=[round(d["vforce"] * 1e3, 2) for d in s["phases"]],
                             substep_us_rounds=[round(float(x), 2) for x in s["substep_us"]],
                             gauge_first_cloth=float(ps["gauge"][0]), capped=int(ps["capped"].sum()), error_flags=int(st["error_flags"])))
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
        for r in rows[1:]:
            r["substep_ratio"] = round(r["substep_us"] / rows[0]["substep_us"], 4)
        for g in engines.values():
            g.destroy()
        records += rows
    print(json.dumps(dict(workload="enclosed-volume pressure: VFORCE phase and substep", dt=args.dt, steps=args.steps,
                          rounds=args.rounds, rows=records)))


if __name__ == "__main__":
    main()
