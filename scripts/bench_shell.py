#!/usr/bin/env python3
"""Cost of shell bending (mpm_set_shell_bending) on the bench.py workload (cloth_1m, 16 open sheets): `plain` against
`flat` (mpm_set_bending on every sheet: k_vforce and k_bend) against `shell` (mpm_set_shell_bending on every sheet:
k_vforce, k_hinge over every hinge, k_hinge_gather over every vertex) against `creased` (the shell engine with
mpm_set_creases at a yield angle of 1 rad on every sheet: k_crease runs in front of k_hinge, reads every hinge's corners,
and no hinge yields) against `damped` (the shell engine with mpm_set_shell_damping, beta = dt / 2 on every sheet: k_hinge<1>
runs in k_hinge<0>'s place and also reads every hinge's four corner velocities).  The stiffness is the one at which dt is a quarter of the feature's own guard, so both models act
and the trajectory stays stable.

Per round every engine runs once, in turn, in one process: mpm_profile_substeps' VFORCE phase (k_vforce and the
feature's kernels; empty on the plain engine, whose vertex forces are summed inside k_p2g; event time), and the whole
substep (wall time of mpm_run_substeps, synchronised at the end).  Medians over the rounds; the raw rounds are printed too.

  python scripts/bench_shell.py [--steps 40] [--warmup 10] [--rounds 5] [--engines plain,flat,shell,creased,damped]

Prints one JSON record.  Under `rocprofv3 --kernel-trace --stats -- python scripts/bench_shell.py --engines shell
--rounds 2` the kernel summary gives k_hinge's and k_hinge_gather's own durations, with `--engines creased` k_crease's.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def engine(bits, cloths, kind, dt):
    from drake_amd import GpuMpm
    g = GpuMpm(bits, GpuMpm.default_material())
    for pos, vel, idx in cloths:
        g.add_qr_cloth(pos, vel, idx)
    g.finalize()
    if kind != "plain":
        set_k = (lambda k: g.set_bending([k] * len(cloths))) if kind == "flat" else (lambda k: g.set_shell_bending([k] * len(cloths)))
        limit = g.bending_max_stable_dt if kind == "flat" else g.shell_max_stable_dt
        set_k(1.0)
        set_k(float(np.float32((0.25 * limit() / dt) ** 2)))
        assert dt <= 0.26 * limit()
    if kind == "creased":
        from drake_amd import CREASE_DTYPE
        t = np.zeros(len(cloths), CREASE_DTYPE)
        t["yield_angle"] = 1.0
        g.set_creases(t)
    if kind == "damped":
        g.set_shell_damping([0.5 * dt] * len(cloths))
        assert dt <= g.shell_max_stable_dt()
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--dt", type=float, default=1e-3)
    ap.add_argument("--engines", default="plain,flat,shell")
    args = ap.parse_args()
    from drake_amd import scenes
    bits, layers, res = scenes.CONFIGS["cloth_1m"]
    cloths = scenes.cloth_stack(layers, res, bits)
    kinds = tuple(args.engines.split(","))
    engines = {k: engine(bits, cloths, k, args.dt) for k in kinds}
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
        rows.append(dict(engine=k, cloths=len(cloths), vertices=int(g.n_verts), faces=int(g.n_faces), hinges=len(g.shell_hinges()[1]),
                         vforce_us=round(float(np.median([d["vforce"] for d in s["phases"]])) * 1e3, 2),
                         phases_us={p: round(float(np.median([d[p] for d in s["phases"]])) * 1e3, 2) for p in s["phases"][0]},
                         substep_us=round(float(np.median(s["substep_us"])), 2),
                         vforce_us_rounds=[round(d["vforce"] * 1e3, 2) for d in s["phases"]],
                         substep_us_rounds=[round(float(x), 2) for x in s["substep_us"]],
                         shell_energy=float(g.shell_state()[0].sum()), error_flags=int(st["error_flags"])))
        if k == "creased":
            rows[-1]["creased_hinges"] = int(g.crease_state()[1].sum())
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    for r in rows[1:]:
        r["substep_ratio"] = round(r["substep_us"] / rows[0]["substep_us"], 4)
    for g in engines.values():
        g.destroy()
    print(json.dumps(dict(workload="shell bending: VFORCE phase and substep on cloth_1m", dt=args.dt, steps=args.steps,
                          rounds=args.rounds, rows=rows)))


if __name__ == "__main__":
    main()
