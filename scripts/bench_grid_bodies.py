#!/usr/bin/env python3
"""Cost of rigid bodies in the grid update (mpm_set_grid_bodies, mpm_bc = MPM_BC_BODIES): the bench.py workload
(BASELINE.json configs[1], ~1M particles) lowered onto the height of mpm_bc = 2's plane and run on
  plane        the mpm_bc = 2 plane (k_grid<1>, the reference's scene)
  plane_body   the same plane as a half-space body
  box          a box whose top face is that plane
  cylinder     a cylinder lying under the cloth, spinning about its axis
  mesh         a mesh body (a slab of 12 triangles, its lattice built by mpm_sdf_shape_from_mesh)
  bodies16     sixteen boxes tiled under the cloth
in alternated rounds, one engine per table.

  python scripts/bench_grid_bodies.py [--steps 40] [--warmup 10] [--rounds 5] [--config cloth_1m] [--tables plane,box]

Prints one JSON record: per table the median wall time per substep of mpm_run_substeps and the median event time of the
grid phase (mpm_profile_substeps).  Under `rocprofv3 --kernel-trace --stats -- python scripts/bench_grid_bodies.py
--tables <one table>` the kernel table gives the grid kernel's own duration for that table (k_grid<1> or the
k_grid_bodies instance).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

PLANE_Z = 0.11
TABLES = ("plane", "plane_body", "box", "cylinder", "mesh", "bodies16")


def slab_mesh(half):
    """a box of 12 triangles with half extents `half`, body frame"""
    h = np.asarray(half, np.float32)
    v = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float32) * h
    t = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4],
                  [1, 5, 7], [1, 7, 3]], np.int32)
    return v, t


def table_of(name, g):
    from drake_amd import Collider, GridBody
    slip = dict(mode=2, friction=-1.0)
    if name == "plane_body":
        return [GridBody(Collider(0, p_WB=(0, 0, PLANE_Z)), **slip)]
    if name == "box":
        return [GridBody(Collider(2, p_WB=(0.5, 0.5, PLANE_Z - 0.05), dims=(0.3, 0.3, 0.05)), **slip)]
    if name == "cylinder":   # axis along y: R_WB maps z_B to y_W
        R = np.array([[1, 0, 0], [0, 0, 1], [0, -1, 0]], np.float32)
        return [GridBody(Collider(4, p_WB=(0.5, 0.5, PLANE_Z - 0.07), R_WB=R, dims=(0.08, 0.3, 0), w=(0, 2.0, 0)), **slip)]
    if name == "mesh":
        v, t = slab_mesh((0.3, 0.3, 0.05))
        sid = g.sdf_shape_from_mesh(v, t, 0.0125, 2)
        return [GridBody(Collider(0, p_WB=(0.5, 0.5, PLANE_Z - 0.05)), sdf_shape=sid, **slip)]
    if name == "bodies16":
        return [GridBody(Collider(2, p_WB=(0.275 + 0.15 * i, 0.275 + 0.15 * j, PLANE_Z - 0.05), dims=(0.07, 0.07, 0.05)), **slip)
                for i in range(4) for j in range(4)]
    raise ValueError(name)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--config", default="cloth_1m")
    ap.add_argument("--dt", type=float, default=1e-3)
    ap.add_argument("--tables", default=",".join(TABLES))
    args = ap.parse_args()
    from drake_amd import BC_BODIES, GpuMpm, PHASES, scenes
    bits, layers, res = scenes.CONFIGS[args.config]
    dx = 1.0 / (1 << bits)
    names = [t for t in args.tables.split(",") if t]
    engines = {}
    for name in names:
        g = GpuMpm(bits)
        # the stack's lowest sheet a cell above the plane: its stencils load the plane's nodes from the first substep on
        scenes.populate(g, scenes.cloth_stack(layers, res, bits, z0=PLANE_Z + dx))
        g.reallocate_external_bodies(16)
        bc = 2
        if name != "plane":
            g.set_grid_bodies(table_of(name, g))
            bc = BC_BODIES
        g.run_substeps(args.warmup, args.dt, bc)
        g.gpu_sync()
        engines[name] = (g, bc)
    wall = {n: [] for n in names}
    grid = {n: [] for n in names}
    for _ in range(args.rounds):
        for name in names:
            g, bc = engines[name]
            t0 = time.perf_counter()
            g.run_substeps(args.steps, args.dt, bc)
            g.gpu_sync()
            wall[name].append((time.perf_counter() - t0) * 1e6 / args.steps)
            ph, _ = g.profile_substeps(args.steps, args.dt, bc)
            grid[name].append(ph["grid"] * 1e3)
    rows = []
    for name in names:
        g, _ = engines[name]
        st = g.stats()
        _, f = g.external_body_force_to_host()
        rows.append(dict(table=name, us_per_substep=round(statistics.median(wall[name]), 2),
                         grid_phase_us=round(statistics.median(grid[name]), 2), rebuilds=int(st["rebuilds"]),
                         error_flags=int(st["error_flags"]), f_z_body0=float(f[0, 2])))
        g.destroy()
    assert "grid" in PHASES
    print(json.dumps(dict(workload=f"{args.config} on the plane z = {PLANE_Z}: mpm_run_substeps per table", dt=args.dt,
                          steps=args.steps, rounds=args.rounds, rows=rows)))


if __name__ == "__main__":
    main()
