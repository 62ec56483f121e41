#!/usr/bin/env python3
"""BASELINE.json configs[2]: the 1M-particle cloth stack dropped on a rigid floor (MPM + contact solve).

Not a bench.py line (bench.py measures configs[1]); prints a JSON record with the time split of a
contact substep so the contact kernels can be profiled at scale:

  python scripts/bench_contact.py [--steps 30] [--config cloth_1m] [--mu 0.5]

Contact pairs are produced the way the reference's DeformableDriver does it (positions to the host,
signed distance per particle, pairs back to the device, deformable_driver.h:120-194); that host
round trip is timed separately from the solve.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402


def box_mesh(half):
    """12 triangles: the box with half extents `half`, centred on the body origin"""
    v = np.array([[sx * half[0], sy * half[1], sz * half[2]] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float32)
    f = np.array([(0, 1, 3), (0, 3, 2), (4, 6, 7), (4, 7, 5), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4),
                  (1, 5, 7), (1, 7, 3)], np.int32)
    return v, f


def slab_mesh(half_xy=0.5, depth=0.125):
    """a slab under the whole domain whose top face is the body frame's z = 0"""
    v, f = box_mesh((half_xy, half_xy, depth / 2))
    v[:, 2] -= depth / 2
    return v, f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", default="cloth_1m")
    ap.add_argument("--mu", type=float, default=0.5)
    ap.add_argument("--floor", type=float, default=0.5)
    ap.add_argument("--dt", type=float, default=1e-3)
    ap.add_argument("--stiffness", type=float, default=1e5)
    ap.add_argument("--damping", type=float, default=1e-3)
    ap.add_argument("--survey-config3", action="store_true",
                    help="SURVEY.md 8(d) config 3: floor z<0.25, k=1e6, d=1e-5, mu=1, dt=2e-4")
    ap.add_argument("--device-pairs", action="store_true",
                    help="contact pairs from mpm_generate_contact_pairs instead of the host round trip")
    ap.add_argument("--colliders", default="floor",
                    choices=["floor", "capsules16", "cylinders16", "ellipsoids16", "boxes16", "mesh", "mesh1", "mesh_floor"],
                    help="with --device-pairs: the floor, or 16 bodies of one kind on a 4 x 4 grid across the floor plane "
                         "(rotated, cutting the cloth; no floor).  Mesh colliders (mpm_set_sdf_colliders): mesh = the 16 "
                         "boxes of boxes16 as 12-triangle meshes, mesh1 = one of them (on the cloth) alone, mesh_floor = a slab mesh "
                         "whose top face is the floor plane")
    ap.add_argument("--uniform-table", action="store_true",
                    help="mpm_set_body_contact_materials with one entry equal to the call's scalars: the same solve through "
                         "the per-contact parameter planes")
    args = ap.parse_args()
    if args.survey_config3:
        args.floor, args.stiffness, args.damping, args.mu, args.dt = 0.25, 1e6, 1e-5, 1.0, 2e-4
    from drake_amd import Collider, GpuMpm, SdfCollider, scenes
    bits, layers, res = scenes.CONFIGS[args.config]
    dt, stiffness, damping = args.dt, args.stiffness, args.damping
    floor = [Collider(0, body=0, p_WB=(0.5, 0.5, args.floor))]
    mesh = []          # (shape builder, per-collider poses) of the mesh choices
    if args.colliders != "floor":
        assert args.device_pairs, "--colliders needs --device-pairs"
        c, s_ = np.cos(1.2), np.sin(1.2)
        R = ((1, 0, 0), (0, c, -s_), (0, s_, c))   # tilted about x: a slanted cut through the sheets
        grid = [(0.2 + 0.2 * (j % 4), 0.2 + 0.2 * (j // 4), args.floor) for j in range(16)]
        box_half = (0.06, 0.03, 0.02)
        if args.colliders in ("mesh", "mesh1"):
            floor = []
            mesh = [(box_mesh(box_half), 0.005, dict(p_WB=p, R_WB=R)) for p in (grid if args.colliders == "mesh" else grid[5:6])]
        elif args.colliders == "mesh_floor":
            floor = []
            mesh = [(slab_mesh(), 1.0 / 128, dict(p_WB=(0.5, 0.5, args.floor)))]
        else:
            kind, dims = {"capsules16": (3, (0.02, 0.05, 0)), "cylinders16": (4, (0.02, 0.05, 0)),
                          "ellipsoids16": (5, (0.06, 0.03, 0.02)), "boxes16": (2, box_half)}[args.colliders]
            floor = [Collider(kind, body=0, p_WB=p, R_WB=R, dims=dims) for p in grid]
    g = GpuMpm(bits)
    # the stack starts with its lowest sheets already touching the floor and moves down at 0.5 m/s
    sheets = scenes.cloth_stack(layers, res, bits, z0=args.floor - 0.004)
    for pos, vel, idx in sheets:
        vel[:, 2] -= 0.5
    scenes.populate(g, sheets)
    g.reallocate_external_bodies(1)
    if args.uniform_table:
        g.set_body_contact_materials([(args.mu, stiffness, damping)])
    build_ms = 0.0
    if mesh:
        shapes = {}
        for (v, f), cell, pose in mesh:     # (one lattice per distinct mesh; a build is a synchronisation point)
            key = (v.tobytes(), cell)
            if key not in shapes:
                t = time.perf_counter()
                shapes[key] = g.sdf_shape_from_mesh(v, f, cell)
                build_ms += 1e3 * (time.perf_counter() - t)
        g.set_sdf_colliders([SdfCollider(shapes[(v.tobytes(), cell)], body=0, **pose) for (v, f), cell, pose in mesh])
    T = dict(transfer=0.0, pairs_host=0.0, copy_pairs=0.0, solve=0.0, step=0.0)
    iters, ncontacts = [], []
    for s in range(args.warmup + args.steps):
        timed = s >= args.warmup
        t0 = time.perf_counter()
        g.rebuild_mapping(False)
        g.calc_fem_state_and_force(dt)
        g.particle_to_grid(dt)
        g.update_grid(-1)
        g.gpu_sync()
        t1 = time.perf_counter()
        if args.device_pairs:
            t2 = t3 = time.perf_counter()
            n = g.generate_contact_pairs(floor)
            t4 = time.perf_counter()
        else:
            pos = g.sync_particle_state_to_cpu()
            t2 = time.perf_counter()
            z = pos[:, 2]
            idx = np.nonzero(z < args.floor)[0].astype(np.uint32)
            n = idx.size
            dist = (z[idx] - args.floor).astype(np.float32)
            normal = np.tile(np.array([0, 0, -1], np.float32), (n, 1))
            cpos = pos[idx]
            zeros = np.zeros((n, 3), np.float32)
            body = np.zeros(n, np.uint32)
            t3 = time.perf_counter()
            g.copy_contact_pairs(idx, body, dist, normal, cpos, zeros, zeros)
            t4 = time.perf_counter()
        r = g.update_contact(dt, args.mu, stiffness, damping)
        g.gpu_sync()
        t5 = time.perf_counter()
        g.grid_to_particle(dt)
        g.gpu_sync()
        t6 = time.perf_counter()
        if timed:
            T["step"] += (t1 - t0) + (t6 - t5)
            T["transfer"] += t2 - t1
            T["pairs_host"] += t3 - t2
            T["copy_pairs"] += t4 - t3
            T["solve"] += t5 - t4
            iters.append(r["iterations"])
            ncontacts.append(n)
    k = args.steps
    out = dict(config=args.config, particles=g.n_particles, steps=k, mu=args.mu, dt=dt, stiffness=stiffness,
               damping=damping, floor=args.floor, pairs="device" if args.device_pairs else "host", colliders=args.colliders,
               uniform_table=bool(args.uniform_table),
               contacts_mean=float(np.mean(ncontacts)), contacts_max=int(np.max(ncontacts)),
               newton_iterations_mean=float(np.mean(iters)), newton_iterations_max=int(np.max(iters)),
               ms_per_substep={a: 1e3 * b / k for a, b in T.items()},
               solve_us_per_iteration=1e6 * T["solve"] / max(1, int(np.sum(iters))), stats=g.stats())
    if mesh:
        out["sdf_build_ms"] = build_ms
    print(json.dumps(out))


if __name__ == "__main__":
    main()
