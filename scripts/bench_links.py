#!/usr/bin/env python3
"""Cost of links between cloth vertices (mpm_set_links): the bench.py workload (cloth_1m, 16 sheets) on three engines --
plain, `seams` (a few thousand links between neighbouring sheets: the first 256 vertices of every sheet joined to the
same vertices of the next) and `dense` (one link per vertex: every vertex of an even sheet joined to the same vertex of
the sheet above); `dense_limits` is `dense` with a break_length of 1 m on every link (mpm_set_link_limits: k_link_break
runs in front of k_link, reads every link's ends and breaks nothing).  The links are springs at their rest length (L = the distance at the start), k such that dt is a
quarter of mpm_links_max_stable_dt, c = 0: k_vforce and k_link run and every record is read and evaluated, while the
trajectory stays close to the plain engine's.  Per round every engine runs once, in turn, in one process:
mpm_profile_substeps' VFORCE phase (k_vforce + k_link on an engine with links, empty on the plain one, whose vertex
forces are summed inside k_p2g; event time), its P2G phase, and the whole substep (wall time of mpm_run_substeps,
synchronised at the end).  Medians over the rounds; the raw rounds are printed too.

  python scripts/bench_links.py [--steps 40] [--warmup 10] [--rounds 5] [--config cloth_1m]
                                [--engines plain,seams,dense,dense_limits]

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


def link_table(sheets, kind):
    from drake_amd import links
    first = np.cumsum([0] + [len(pos) for pos, _, _ in sheets])
    a, b = [], []
    if kind == "seams":
        for s in range(len(sheets) - 1):
            n = min(256, len(sheets[s][0]), len(sheets[s + 1][0]))
            a.append(first[s] + np.arange(n))
            b.append(first[s + 1] + np.arange(n))
    elif kind in ("dense", "dense_limits"):
        for s in range(0, len(sheets) - 1, 2):
            n = min(len(sheets[s][0]), len(sheets[s + 1][0]))
            a.append(first[s] + np.arange(n))
            b.append(first[s + 1] + np.arange(n))
    a, b = np.concatenate(a), np.concatenate(b)
    x = np.concatenate([np.asarray(pos, np.float32).reshape(-1, 3) for pos, _, _ in sheets]).astype(np.float64)
    rest = np.linalg.norm(x[b] - x[a], axis=1)
    return links(a, b, 1.0, rest, 0.0, 0)


def engine(bits, sheets, kind, dt):
    from drake_amd import GpuMpm
    g = GpuMpm(bits)
    for pos, vel, idx in sheets:
        g.add_qr_cloth(pos, vel, idx)
    g.finalize()
    if kind != "plain":
        t = link_table(sheets, kind)
        g.set_links(t)
        t["stiffness"] *= np.float32((0.25 * g.links_max_stable_dt() / dt) ** 2)   # (the limit scales with 1 / sqrt(k))
        g.set_links(t)
        if kind == "dense_limits":
            g.set_link_limits(np.full(len(t), 1.0, np.float32))
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--config", default="cloth_1m")
    ap.add_argument("--dt", type=float, default=1e-3)
    ap.add_argument("--engines", default="plain,seams,dense", help="which of the three engines run (a kernel trace of one)")
    args = ap.parse_args()
    from drake_amd import scenes
    bits, layers, res = scenes.CONFIGS[args.config]
    sheets = scenes.cloth_stack(layers, res, bits)
    kinds = tuple(args.engines.split(","))
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
        t = g.get_links()
        rows.append(dict(engine=k, links=int(len(t)), stiffness=float(t["stiffness"][0]) if len(t) else 0.0,
                         max_stable_dt=g.links_max_stable_dt(),
                         limits=int((g.get_link_limits() > 0).sum()), broken=g.link_break_state()[1],
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
    print(json.dumps(dict(workload=f"{args.config}: links between cloth vertices, VFORCE phase and substep", dt=args.dt,
                          steps=args.steps, rounds=args.rounds, rows=rows)))


if __name__ == "__main__":
    main()
