#!/usr/bin/env python3
"""Cost of the tear coupling (mpm_set_tear_coupling) in the kernels it touches, on the bench.py workload (cloth_1m, 16 open
sheets) with shell bending and creases (yield angle 1 rad: k_crease reads every hinge, none yields) on every sheet, and a gas
icosphere of 20,480 faces below the stack (k_pressure_volume over 20 chunks, k_pressure_gauge).

  --mask M   call mpm_set_tear_coupling(M) first (omit: the call is never made -- what a library without it can run)
  --limit L  a tear limit on every cloth (needs a mask that permits it); 100 never tears: the tear tables exist, the flags
             are read by k_crease, k_hinge and k_pressure_volume, and no face is torn
  --root D   import drake_amd from another checkout of the project (its own library), for an A/B against this one

Prints one JSON record: wall time per substep of mpm_run_substeps, and the state's checksum.  Under
`rocprofv3 --kernel-trace --stats -- python scripts/bench_tear_coupling.py ...` the kernel summary gives the durations of
k_crease, k_hinge, k_hinge_gather, k_pressure_volume, k_pressure_gauge and k_pressure.
"""
import argparse
import json
import os
import sys
import time
import zlib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=80)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--dt", type=float, default=1e-3)
    ap.add_argument("--mask", type=int, default=None)
    ap.add_argument("--limit", type=float, default=0.0)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import numpy as np
    from drake_amd import ARR, CREASE_DTYPE, PRESSURE_DTYPE, PRESSURE_GAS, GpuMpm, scenes
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tests import pressure as pr

    bits, layers, res = scenes.CONFIGS["cloth_1m"]
    cloths = list(scenes.cloth_stack(layers, res, bits))
    Xi, Ti = pr.icosphere((0.5, 0.5, 0.3), 0.08, subdivisions=5)
    cloths.append((Xi, np.zeros_like(Xi), Ti.reshape(-1)))
    n = len(cloths)
    g = GpuMpm(bits, GpuMpm.default_material())
    for pos, vel, idx in cloths:
        g.add_qr_cloth(pos, vel, idx)
    g.finalize()
    if args.mask is not None:
        g.set_tear_coupling(args.mask)
    on = np.array([1.0] * layers + [0.0])
    g.set_shell_bending(on)
    g.set_shell_bending(np.float32((0.25 * g.shell_max_stable_dt() / args.dt) ** 2) * on)
    assert args.dt <= 0.26 * g.shell_max_stable_dt()
    t = np.zeros(n, CREASE_DTYPE)
    t["yield_angle"][:layers] = 1.0
    g.set_creases(t)
    p = np.zeros(n, PRESSURE_DTYPE)
    p[n - 1] = (PRESSURE_GAS, 0.0, np.float32(1.5 * 100.0 * pr.volume64(Xi, Ti)), 100.0, 1000.0)
    g.set_pressure(p)
    if args.limit:
        g.set_tearing([args.limit] * n)
    g.run_substeps(args.warmup, args.dt, -1)
    g.gpu_sync()
    t0 = time.perf_counter()
    g.run_substeps(args.steps, args.dt, -1)
    g.gpu_sync()
    us = (time.perf_counter() - t0) * 1e6 / args.steps
    st = g.stats()
    crc = 0
    for arr in (ARR.POSITIONS, ARR.VELOCITIES):
        crc = zlib.crc32(np.ascontiguousarray(g.download(arr)).tobytes(), crc)
    rec = dict(mask=args.mask, limit=args.limit, substep_us=round(us, 2), hinges=len(g.shell_hinges()[1]), faces=int(g.n_faces),
               vertices=int(g.n_verts), gauge=float(g.pressure_state()["gauge"][n - 1]), creased=int(g.crease_state()[1].sum()),
               torn=int(g.tear_state()[1].sum()), error_flags=st["error_flags"], rebuilds=st["rebuilds"], state_crc32=crc,
               library=os.path.abspath(args.root))
    print(json.dumps(rec))
    g.destroy()


if __name__ == "__main__":
    main()
