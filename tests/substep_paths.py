"""The host paths that enqueue a whole substep, each run on one small deterministic scene (tests/test_substep_paths_gpu.py,
scripts/substep_paths.py).  All of them go through the same two functions of the engine's host code
(enqueue_substep_front / enqueue_substep_rest, mpm_engine.hip); they fall into two families by the grid kernel:

  fused    the fused grid update: run_substeps in uneven batches, profile_substeps, the five phase calls (held back and
           launched as one substep, or -- MPM_DEFER_PHASES=0 -- launched call by call)
  sums     the gather of the raw node sums, then the update from sums: substep_begin / substep_end, and
           substep_begin_halo / (substep_mid_halo /) substep_end_halo with no zone
  coupled  run_coupled_substeps over a floor the lower sheet reaches after ~35 substeps: contact-free chunks behind a
           watch kernel first, then substeps with pair generation and contact solve

The scene: GpuMpm(6), two sheets of 32 x 32 vertices moving sideways at 2 m/s -- a cell every 16 substeps of 5e-4 s, so
re-sorts and owed substeps occur within the 48 substeps --, optionally a fan of 12 faces around one vertex, which makes
the vertex forces a kernel of their own (k_vforce)."""
import os

import numpy as np

DT = 5e-4
N = 48
BATCHES = (1, 7, 3, 16, 2, 19)   # uneven, N in all
assert sum(BATCHES) == N


def fan_sheet(n_rim, radius, centre, z, seed):
    """A disc of n_rim triangles around a hub vertex (tests/test_parity_gpu.py)."""
    from tests.test_parity_gpu import _fan_sheet
    return _fan_sheet(n_rim, radius, centre, z, seed)


def sheets(fan=True):
    from drake_amd import scenes
    out = list(scenes.cloth_stack(2, 32, 6, z0=0.5, side=0.4, seed=11, vel_amp=0.2))
    if fan:
        dx = 1.0 / 64
        out.append(fan_sheet(12, 0.9 * dx, (0.5, 0.5), 0.5 + 4 * dx, 5))
    for pos, vel, idx in out:
        vel[:, 0] += 2.0
    return out


def engine(fan=True, pins=False, bending=False, defer_phases=True):
    """-> a finalised deterministic engine.  pins: two vertices of the first sheet on a moving body; bending: stiffness on
    every cloth.  defer_phases = False: the engine is created under MPM_DEFER_PHASES=0."""
    from drake_amd import BodyMotion, GpuMpm, Pin, scenes
    old = os.environ.get("MPM_DEFER_PHASES")
    if not defer_phases:
        os.environ["MPM_DEFER_PHASES"] = "0"
    try:
        g = GpuMpm(6)
    finally:
        if not defer_phases:
            if old is None:
                del os.environ["MPM_DEFER_PHASES"]
            else:
                os.environ["MPM_DEFER_PHASES"] = old
    g.set_deterministic(True)
    sh = sheets(fan)
    scenes.populate(g, sh)
    if pins:
        # (the body moves with the sheet: the pinned vertices keep their place in it)
        p0, p1 = sh[0][0][0], sh[0][0][31]
        g.reallocate_external_bodies(1)
        g.set_body_motions([BodyMotion(0, p_WB=(0, 0, 0), v=(2.0, 0, 0))])
        g.set_pins([Pin(0, 0, p0), Pin(31, 0, p1)])
    if bending:
        # (the limit goes with 1 / sqrt(k): DT at half of it)
        g.set_bending([1e-5] * len(sh))
        g.set_bending([1e-5 * (g.bending_max_stable_dt() / (2.0 * DT)) ** 2] * len(sh))
    return g


def _phase_calls(g, bc=-1):
    for _ in range(N):
        g.rebuild_mapping(False)
        g.calc_fem_state_and_force(DT)
        g.particle_to_grid(DT)
        g.update_grid(bc)
        g.grid_to_particle(DT)


def _run_substeps(g, bc=-1):
    for k in BATCHES:
        g.run_substeps(k, DT, bc)


def _profile_substeps(g, bc=-1):
    for k in BATCHES:
        g.profile_substeps(k, DT, bc)


def _begin_end(g, bc=-1):
    for _ in range(N):
        g.substep_begin(DT)
        g.substep_end(DT, bc)


def _begin_end_halo(g):
    from drake_amd import GpuMpm
    zones = GpuMpm.halo_zone_args([], [])
    bufs = GpuMpm.halo_buffer_args([])
    for _ in range(N):
        g.substep_begin_halo(DT, zones, 0)
        g.substep_end_halo(DT, -1, bufs, 0)


def _begin_mid_end_halo(g):
    from drake_amd import GpuMpm
    zones = GpuMpm.halo_zone_args([], [])
    bufs = GpuMpm.halo_buffer_args([])
    for _ in range(N):
        g.substep_begin_halo(DT, zones, 0)
        g.substep_mid_halo(DT, -1)
        g.substep_end_halo(DT, -1, bufs, 0)


def _coupled(g):
    from drake_amd import Collider
    g.reallocate_external_bodies(1)
    floor = [Collider(0, body=0, p_WB=(0.5, 0.5, 0.4985))]
    for k in BATCHES:
        g.run_coupled_substeps(k, DT, floor, 0.5, 1e5, 1e-3)


# name -> (family, runner, engine keyword arguments)
PATHS = {
    "run_substeps": ("fused", _run_substeps, {}),
    "profile_substeps": ("fused", _profile_substeps, {}),
    "phase_calls": ("fused", _phase_calls, {}),
    "phase_calls_undeferred": ("fused", _phase_calls, {"defer_phases": False}),
    "substep_begin_end": ("sums", _begin_end, {}),
    "substep_begin_end_halo": ("sums", _begin_end_halo, {}),
    "substep_begin_mid_end_halo": ("sums", _begin_mid_end_halo, {}),
    "coupled": ("coupled", _coupled, {}),
}


def run(name, **scene):
    """Runs path `name` on a fresh engine -> (the four state arrays as uint32 words, stats)."""
    from drake_amd import ARR as A
    _, runner, kw = PATHS[name]
    g = engine(**scene, **kw)
    runner(g)
    g.gpu_sync()
    state = {k: np.ascontiguousarray(g.download(arr)).view(np.uint32).copy()
             for k, arr in (("pos", A.POSITIONS), ("vel", A.VELOCITIES), ("C", A.AFFINE), ("F", A.DEFORMATION_GRADIENTS))}
    st = g.stats()
    g.destroy()
    return state, st
