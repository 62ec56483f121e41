#!/usr/bin/env python3
"""Cost of the weave (mpm_set_weave): the bench.py workload (cloth_1m, 16 sheets) on four engines in one process --
`plain` (the feature off: the kernels every engine ran before it existed), `weave` (every cloth woven, E_warp = 10 E_weft,
moduli such that dt is a quarter of mpm_weave_max_stable_dt: k_weave behind k_fem), `damp` (membrane damping at a quarter
of its limit: k_damp behind k_fem, the yardstick) and `weave_damp` (both: k_fem, k_weave, k_damp).  Per round every engine
runs once, in turn (alternated rounds, so that drift of the box hits all engines alike): mpm_profile_substeps' FEM phase
(event times) and the whole substep (wall time of mpm_run_substeps, synchronised at the end).  Medians over the rounds;
the raw rounds are printed too.  k_weave's time is FEM(weave) - FEM(plain), k_damp's FEM(damp) - FEM(plain), from the
same run; their algorithmic bytes (counted below from the kernels' loads and stores) over those times are set against
HBM's 8 TB/s.

  python scripts/bench_weave.py [--steps 40] [--warmup 10] [--rounds 5] [--config cloth_1m]

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
# k_weave per face: the static records fq[2], fq[3] (32), PSet::pid (4), the cloth index (4), the axis (8); three 16-byte
# gathers of corner positions (48); three 12-byte records read and written (72).  The per-cloth coefficients stay in cache.
WEAVE_BYTES_PER_FACE = 32 + 4 + 4 + 8 + 48 + 72
# k_damp per face (scripts/bench_damping.py): six gathers, no axis
DAMP_BYTES_PER_FACE = 32 + 4 + 1 + 96 + 72


def engine(bits, sheets, kind, dt):
    from drake_amd import GpuMpm
    g = GpuMpm(bits)
    for pos, vel, idx in sheets:
        g.add_qr_cloth(pos, vel, idx)
    g.finalize()
    n = g.cloth_count()
    if kind in ("weave", "weave_damp"):
        unit = np.array([(10.0, 1.0, 0.2, 0.05, 1.0, 0.3, 0.0)] * n, np.float32)
        g.set_weave(unit)
        unit[:, [0, 1, 3]] *= np.float32((0.25 * g.weave_max_stable_dt() / dt) ** 2)     # (the limit scales with 1 / sqrt(k))
        g.set_weave(unit)
    if kind in ("damp", "weave_damp"):
        g.set_damping([(1.0, 0.0)] * n)
        g.set_damping([(0.25 * g.damping_max_stable_dt() / dt, 0.0)] * n)              # (the limit scales with 1 / beta)
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
    kinds = ("plain", "weave", "damp", "weave_damp")
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
        w = g.get_weave()[0]
        rows[k] = dict(engine=k, weave=[float(w[f]) for f in ("E_warp", "E_weft", "nu", "G")],
                       damping=[float(x) for x in g.get_damping()[0]], weave_max_stable_dt=g.weave_max_stable_dt(),
                       phases_us={p: round(float(np.median([d[p] for d in s["phases"]])) * 1e3, 2) for p in s["phases"][0]},
                       substep_us=round(float(np.median(s["substep_us"])), 2),
                       fem_us_rounds=[round(d["fem"] * 1e3, 2) for d in s["phases"]],
                       substep_us_rounds=[round(float(x), 2) for x in s["substep_us"]], error_flags=int(g.stats()["error_flags"]))
        print(json.dumps(rows[k]), file=sys.stderr, flush=True)
    nf = engines["plain"].n_faces
    fem = {k: rows[k]["phases_us"]["fem"] for k in kinds}
    spread = max(max(rows[k]["fem_us_rounds"]) - min(rows[k]["fem_us_rounds"]) for k in kinds)

    def kernel(us, per_face):
        return dict(us=round(us, 2), bytes=nf * per_face, bytes_per_face=per_face,
                    hbm_fraction=round(nf * per_face / (us * 1e-6) / (HBM_PEAK_GBS * 1e9), 4) if us > 0 else None)

    cost = dict(faces=nf, k_fem_us=fem["plain"], fem_spread_of_the_rounds_us=round(spread, 2),
                k_weave=kernel(fem["weave"] - fem["plain"], WEAVE_BYTES_PER_FACE),
                k_damp=kernel(fem["damp"] - fem["plain"], DAMP_BYTES_PER_FACE),
                k_weave_plus_k_damp_us=round(fem["weave_damp"] - fem["plain"], 2))
    for k in kinds[1:]:
        rows[k]["substep_ratio"] = round(rows[k]["substep_us"] / rows["plain"]["substep_us"], 4)
    for g in engines.values():
        g.destroy()
    print(json.dumps(dict(workload=f"{args.config}: weave, FEM phase and substep", dt=args.dt, steps=args.steps, rounds=args.rounds,
                          rows=[rows[k] for k in kinds], cost=cost)))


if __name__ == "__main__":
    main()
