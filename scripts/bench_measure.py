#!/usr/bin/env python3
"""Time per mpm_measure call on the bench.py workload (cloth_1m, 16 sheets), with HIP events on the engine's stream: 20
calls after 3 warm-up calls, bending off and on, next to the substep time of the same run (200 substeps of
mpm_run_substeps after 20: wall clock as bench.py takes it, and HIP events around them).

  python scripts/bench_measure.py > profiles/measure_1m.txt"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from drake_amd import GpuMpm, scenes  # noqa: E402

torch.cuda.set_device(0)
bits, layers, res = scenes.CONFIGS["cloth_1m"]
dt = 1e-3
g = GpuMpm(bits)
scenes.populate(g, scenes.cloth_stack(layers, res, bits, seed=1234))
stream = torch.cuda.Stream()
g.set_stream(stream.cuda_stream)
g.run_substeps(20, dt, -1)
g.gpu_sync()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
t0 = time.perf_counter()
e0.record(stream)
g.run_substeps(200, dt, -1)
e1.record(stream)
g.gpu_sync()
wall = (time.perf_counter() - t0) / 200 * 1e6
torch.cuda.synchronize()
sub_ev = e0.elapsed_time(e1) / 200 * 1e3
lines = [f"cloth_1m: {g.n_particles} particles, {g.cloth_count()} cloths, dt = {dt}",
         f"substep (mpm_run_substeps, 200 after 20): {wall:.1f} us wall clock, {sub_ev:.1f} us between HIP events"]
for label, bend in (("bending off", False), ("bending on (k = 1e-5 every cloth)", True)):
    if bend:
        g.set_bending([1e-5] * g.cloth_count())
    for _ in range(3):
        g.measure()
    ev, host = [], []
    for _ in range(20):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        th = time.perf_counter()
        a.record(stream)
        rows, total = g.measure()
        b.record(stream)
        host.append((time.perf_counter() - th) * 1e6)
        torch.cuda.synchronize()
        ev.append(a.elapsed_time(b) * 1e3)
    ev, host = np.array(ev), np.array(host)
    lines.append(f"mpm_measure, {label}: {ev.mean():.1f} us between HIP events (min {ev.min():.1f}, max {ev.max():.1f}), "
                 f"{host.mean():.1f} us on the host per call; 20 calls after 3 = {ev.mean() / sub_ev:.2f} substeps")
    lines.append(f"    total: mass {float(total['mass']):.6g} kinetic {float(total['kinetic']):.6g} faces {int(total['faces'])} "
                 f"vertices {int(total['vertices'])} bending {float(total['bending']):.6g}")
assert g.stats()["error_flags"] == 0
print("\n".join(lines))
g.destroy()
