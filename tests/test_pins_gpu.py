"""Fixed constraints (pins, include/mpm_hip.h: mpm_set_pins, mpm_set_body_motions, mpm_pins_inside_collider) on the
device: against the CPU oracle with the pins emulated on the host (tests/pin_reference.py), the substep paths against
each other to the bit, a coupled run, the reaction, tile crossings, the selection, clearing and the refusals."""
import numpy as np
import pytest

from tests.helpers import build_pair, close, natural_scales
from tests.pin_layouts import clock_after, pin_bounds
from tests.pin_reference import PinEmulator, face_recentring, rodrigues
from tests import harness as hs

pytestmark = pytest.mark.gpu
DT = 1e-3
MOTION = ((0.5, 0.5, 0.5), rodrigues([0.1, 0.2, 0.3]), (0.05, -0.02, 0.01), (0.3, -0.2, 0.5))
# a pinned vertex against the float64 target: the kernel evaluates the target in double and rounds once.  The bound per pin
# and component is tests/pin_layouts.py's: half a float32 ulp of the value plus the double term counted there.
ERR_INVALID, ERR_DOMAIN = -1, -6


def _motion(body, m):
    from drake_amd import BodyMotion
    p, R, v, w = m
    return BodyMotion(body, p, np.asarray(R).ravel(), v, w)


def _pins_for(g, every=20, body=0, motion=MOTION, verts=None):
    """every `every`-th vertex (5 %) pinned where it is now, in the frame of `motion`'s starting pose"""
    from drake_amd import Pin
    x, _ = g.dump_cpu_state()
    if verts is None:
        verts = np.arange(0, x.shape[0], every)
    p = np.asarray(motion[0], np.float64)
    R = np.asarray(motion[1], np.float64).reshape(3, 3)
    q = (x[verts].astype(np.float64) - p) @ R   # R^T (x - p), row by row
    pins = [(int(v), body, q[k]) for k, v in enumerate(verts)]
    return pins, [Pin(v, b, qq) for v, b, qq in pins]


def _state(g):
    A = hs.ARR()
    tau, f = g.external_body_force_to_host()
    return dict(pos=g.download(A.POSITIONS), vel=g.download(A.VELOCITIES), C=g.download(A.AFFINE), tau=tau, f=f)


def _same(a, b, what=""):
    for k in ("pos", "vel", "C", "tau", "f"):
        assert np.array_equal(a[k], b[k]), (what, k)


def _engine(sheets, env=None, bodies=1):
    from drake_amd import GpuMpm, scenes
    with hs.environ(dict(env or {}, MPM_DETERMINISTIC="1")):
        g = GpuMpm(6)
    scenes.populate(g, [(p.copy(), v.copy(), i.copy()) for p, v, i in sheets])
    g.reallocate_external_bodies(bodies)
    return g


def test_pins_against_the_oracle():
    """20 phase-by-phase substeps, 5 % of the vertices pinned to a translating and rotating body: the state against the
    oracle with the pins emulated on the host; the pinned vertices against the float64 target."""
    A = hs.ARR()
    o, g = build_pair(domain_bits=6, layers=2, res=16, vel_amp=0.2)
    sc = natural_scales(o, DT)
    g.reallocate_external_bodies(1)
    pins, arr = _pins_for(g)
    g.set_pins(arr)
    g.set_body_motions([_motion(0, MOTION)])
    em = PinEmulator(pins, {0: MOTION})
    nf, dens = o.n_faces, float(o.p.density)
    for _ in range(20):
        o.substep(DT, -1)
        em.apply(o, DT, nf, dens)
        hs.phases(g, DT)
    g.gpu_sync()
    assert g.stats()["error_flags"] == 0
    pid = g.download(A.PIDS)

    def orig(a):
        out = np.empty_like(a)
        out[pid] = a
        return out

    so = o.state_in_original_order()
    # (trajectory bounds of tests/test_parity_gpu.py::test_trajectory_with_sorts_and_rebuilds)
    close(orig(g.download(A.POSITIONS)), so["pos"], scale=1.0, rtol=1e-5, what="pins traj pos")
    close(orig(g.download(A.VELOCITIES)), so["vel"], scale=sc["vel"], rtol=3e-4, what="pins traj vel")
    verts = np.array([p[0] for p in pins])
    x, _ = g.dump_cpu_state()
    xt, vt, Ct, bx, bv = pin_bounds(MOTION, np.array([p[2] for p in pins]), clock_after([DT] * 20))
    assert np.all(np.abs(x[verts] - xt) <= bx), (np.abs(x[verts] - xt) / bx).max()
    vel = orig(g.download(A.VELOCITIES))[nf + verts]
    assert np.all(np.abs(vel - vt) <= bv), (np.abs(vel - vt) / bv).max()
    Cg = orig(g.download(A.AFFINE))[nf + verts].reshape(-1, 3, 3)
    assert np.abs(Cg - np.float32(Ct)[None]).max() == 0.0


def _moving_sheets(seed=5, vx=9.0):
    from drake_amd import scenes
    sheets = scenes.cloth_stack(2, 16, 6, z0=0.5, side=0.25, seed=seed, vel_amp=0.1, center=(0.35, 0.5))
    for pos, vel, idx in sheets:
        vel[:, 0] += vx   # 9 m/s * 1e-3 s * 64 cells = 0.58 cells per substep: re-sorts inside a batch
    return sheets


def test_paths_agree_to_the_bit():
    """deterministic mode: phase calls, mpm_substep, one mpm_run_substeps batch through re-sorts and owed substeps, and
    mpm_run_coupled_substeps with a collider nobody touches give the same state and impulses to the bit"""
    from drake_amd import Collider
    sheets = _moving_sheets()
    n = 14
    motion = ((0.4, 0.5, 0.5), rodrigues([0.0, 0.1, 0.0]), (9.0, 0.0, 0.0), (0.0, 0.0, 0.4))
    engines = [_engine(sheets, bodies=2) for _ in range(4)]
    for g in engines:
        g.set_pins(_pins_for(g, motion=motion)[1])
        g.set_body_motions([_motion(0, motion)])
    a, b, c, d = engines
    for _ in range(n):
        hs.phases(a, DT)
        b.substep(DT, -1)
    c.run_substeps(n, DT, -1)
    far = [Collider(1, body=1, p_WB=(0.9, 0.1, 0.1), dims=(0.02, 0, 0))]
    d.run_coupled_substeps(n, DT, far, 0.5, 1e5, 1e-4)
    for g in engines:
        g.gpu_sync()
        assert g.stats()["error_flags"] == 0
    assert c.stats()["rebuilds"] >= 3
    sa = _state(a)
    assert np.abs(sa["f"][0]).max() > 0
    for g, what in ((b, "substep"), (c, "run_substeps"), (d, "coupled")):
        _same(sa, _state(g), what)


def test_coupled_pinned_cloth_falls_onto_a_sphere():
    """a sheet pinned at two corners to body 0 sags onto a sphere on body 1 (mpm_run_coupled_substeps): bit for bit the
    seven calls per substep plus pins; both bodies' impulses are nonzero and equal between the two runs"""
    from drake_amd import Collider, Pin, scenes
    dt, mu, k, dmp = 2e-4, 0.5, 1e5, 1e-5
    sheets = scenes.cloth_stack(1, 24, 6, z0=0.55, side=0.3, seed=3, vel_amp=0.0)
    sheets[0][1][:, 2] -= 0.5
    pos = sheets[0][0]
    c0 = int(np.argmin(pos[:, 0] + pos[:, 1]))
    c1 = int(np.argmax(pos[:, 0] + pos[:, 1]))
    sphere = [Collider(1, body=1, p_WB=(0.5, 0.5, 0.55 - 0.06 - 0.006), dims=(0.06, 0, 0))]
    motion = ((0.5, 0.5, 0.55), np.eye(3), (0, 0, 0), (0, 0, 0))
    runs = []
    for coupled in (False, True):
        g = _engine(sheets, bodies=2)
        x, _ = g.dump_cpu_state()
        g.set_pins([Pin(v, 0, x[v].astype(np.float64) - motion[0]) for v in (c0, c1)])
        g.set_body_motions([_motion(0, motion)])
        n = 150
        if coupled:
            g.run_coupled_substeps(n, dt, sphere, mu, k, dmp)
        else:
            for _ in range(n):
                g.rebuild_mapping(False)
                g.calc_fem_state_and_force(dt)
                g.particle_to_grid(dt)
                g.update_grid(-1)
                g.generate_contact_pairs(sphere, want_count=False)
                g.update_contact(dt, mu, k, dmp)
                g.grid_to_particle(dt)
        g.gpu_sync()
        assert g.stats()["error_flags"] == 0
        runs.append(_state(g))
    _same(runs[0], runs[1], "coupled")
    f = runs[0]["f"]
    assert np.abs(f[0]).max() > 0 and np.abs(f[1]).max() > 0, f


def test_reaction_momentum_identity_on_the_device():
    """P = sum of the grid momentum after ParticleToGrid; per substep P_{k+1} - P_k = M g dt - l_k + d_{k+1} (l_k the
    pins' force impulse of substep k from mpm_external_body_force_to_host, d the face re-centring term of
    tests/test_pins.py).  Tolerance 1e-5 of M |g| dt: float32 sums over the grid and the particles (the float32 oracle
    meets 1e-6)."""
    A = hs.ARR()
    o, g = build_pair(domain_bits=6, layers=2, res=16, vel_amp=0.2, deterministic=True)
    g.reallocate_external_bodies(1)
    pins, arr = _pins_for(g)
    g.set_pins(arr)
    g.set_body_motions([_motion(0, MOTION)])
    nf, dens = o.n_faces, float(o.p.density)
    gvec = np.zeros(3)
    gvec[o.p.gravity_axis] = o.p.gravity
    idx = g.download(A.INDICES).reshape(-1)
    P_prev = l_prev = f_acc = None
    checked = 0
    for s in range(8):
        g.rebuild_mapping(False)
        pid = g.download(A.PIDS)
        vel, vol = np.empty((pid.size, 3)), np.empty(pid.size)
        vel[pid] = g.download(A.VELOCITIES)
        vol[pid] = g.download(A.VOLUMES)
        d = face_recentring(vel, vol, idx, nf, dens)
        g.calc_fem_state_and_force(DT)
        g.particle_to_grid(DT)
        P = g.download(A.GRID_MOMENTUM).astype(np.float64).sum(axis=0)
        M = float(g.download(A.GRID_MASSES).astype(np.float64).sum())
        scale = M * abs(float(o.p.gravity)) * DT
        if P_prev is not None:
            r = P - P_prev - (M * gvec * DT - l_prev + d)
            assert np.abs(r).max() <= 1e-5 * scale, (s, r, scale)
            assert np.abs(l_prev).max() > 0.05 * scale
            checked += 1
        g.update_grid(-1)
        g.grid_to_particle(DT)
        _, f = g.external_body_force_to_host()
        f = f[0].astype(np.float64)
        l_prev = f if f_acc is None else f - f_acc
        f_acc, P_prev = f, P
    assert checked == 7


def test_pins_crossing_tiles_resort_and_match_host_emulation():
    """the pin body moves more than two blocks (8 cells) within one mpm_run_substeps call: no error, the re-sort counter
    rises, and the positions are those of the same motion run as phase calls plus host emulation"""
    from drake_amd import scenes
    sheets = scenes.cloth_stack(1, 16, 6, z0=0.5, side=0.2, seed=8, vel_amp=0.0, center=(0.3, 0.5))
    sheets[0][1][:, 0] += 12.0
    motion = ((0.3, 0.5, 0.5), np.eye(3), (12.0, 0.0, 0.0), (0.0, 0.0, 0.0))
    n = 20   # 12 m/s * 20 ms = 0.24 = 15 cells at 64^3
    a, b = _engine(sheets), _engine(sheets)
    for g in (a, b):
        g.set_pins(_pins_for(g, every=3, motion=motion)[1])
        g.set_body_motions([_motion(0, motion)])
    r0 = a.stats()["rebuilds"]
    a.run_substeps(n, DT, -1)
    a.gpu_sync()
    for _ in range(n):
        hs.phases(b, DT)
    b.gpu_sync()
    sa, sb = a.stats(), b.stats()
    assert sa["error_flags"] == 0 and sb["error_flags"] == 0
    assert sa["rebuilds"] >= r0 + 2, (r0, sa["rebuilds"])
    xa, xb = a.dump_cpu_state()[0], b.dump_cpu_state()[0]
    assert xa[:, 0].mean() - sheets[0][0][:, 0].mean() > 8.0 / 64
    close(xa, xb, scale=1.0, rtol=1e-6, what="tile crossing pos")
    verts, _, q = a.get_pins()   # (the p_BQ the engine holds: float32 of what _pins_for formed)
    assert np.array_equal(verts, np.arange(0, xa.shape[0], 3))
    xt, _, _, bx, _ = pin_bounds(motion, q, clock_after([DT] * n))
    assert np.all(np.abs(xa[verts] - xt) <= bx), (np.abs(xa[verts] - xt) / bx).max()


@pytest.mark.parametrize("kind", ["box", "sphere"])
def test_selection_matches_host_phi(kind):
    from drake_amd import Collider
    o, g = build_pair(domain_bits=6, layers=2, res=16)
    x, _ = g.dump_cpu_state()
    p_WB = np.array([0.45, 0.5, 0.5], np.float32)
    R = rodrigues([0.0, 0.0, 0.3]).astype(np.float32)
    if kind == "box":
        shape = Collider(2, body=0, p_WB=p_WB, R_WB=R.ravel(), dims=(0.08, 0.05, 0.2))
    else:
        shape = Collider(1, body=0, p_WB=p_WB, dims=(0.07, 0, 0))
    phi, _ = g.collider_signed_distance(shape, x)
    want = np.nonzero(phi <= 0)[0]
    assert 0 < want.size < x.shape[0]
    n = g.pins_inside_collider(shape, 3, p_WB, R)
    assert n == want.size
    v, b, q = g.get_pins()
    assert np.array_equal(np.sort(v), want) and np.all(b == 3)
    q_ref = (x[v].astype(np.float64) - p_WB.astype(np.float64)) @ R.astype(np.float64)
    assert np.abs(q - q_ref).max() <= 4 * 2.0 ** -24
    # a second selection adds nothing new: refused, the set unchanged
    from drake_amd import MpmError
    with pytest.raises(MpmError) as e:
        g.pins_inside_collider(shape, 3, p_WB, R)
    assert e.value.code == ERR_INVALID
    assert np.array_equal(g.get_pins()[0], v)


def test_cleared_pins_equal_an_engine_that_never_had_pins():
    A = hs.ARR()
    sheets = _moving_sheets(seed=6, vx=0.5)
    a, b = _engine(sheets), _engine(sheets)
    a.set_pins(_pins_for(a)[1])
    a.set_body_motions([_motion(0, MOTION)])
    a.run_substeps(3, DT, -1)
    a.gpu_sync()
    st = {k: a.download(getattr(A, k)) for k in ("POSITIONS", "VELOCITIES", "AFFINE", "DEFORMATION_GRADIENTS")}
    a.set_pins([])
    # the same uploaded state on both (API slot order; deformation gradients in face order)
    for g in (a, b):
        g.upload_particle_state(st["POSITIONS"], st["VELOCITIES"], st["AFFINE"], None, st["DEFORMATION_GRADIENTS"])
    for g in (a, b):
        g.run_substeps(6, DT, -1)
        g.gpu_sync()
    for k in ("POSITIONS", "VELOCITIES", "AFFINE"):
        assert np.array_equal(a.download(getattr(A, k)), b.download(getattr(A, k))), k


def test_refusals_leave_the_state_unchanged():
    from drake_amd import BodyMotion, GpuMpm, MpmError, Pin, scenes

    def refused(fn):
        with pytest.raises(MpmError) as e:
            fn()
        assert e.value.code == ERR_INVALID

    # before mpm_finalize
    h = GpuMpm(6)
    sheets = scenes.cloth_stack(1, 12, 6, z0=0.5, side=0.2, seed=1, vel_amp=0.1)
    h.add_qr_cloth(*sheets[0])
    refused(lambda: h.set_pins([Pin(0, 0, (0, 0, 0))]))
    refused(lambda: h.set_body_motions([_motion(0, MOTION)]))
    h.finalize()
    x0 = h.dump_cpu_state()[0]
    nv = x0.shape[0]
    refused(lambda: h.set_pins([Pin(nv, 0, (0, 0, 0))]))
    refused(lambda: h.set_pins([Pin(1, 0, (0, 0, 0)), Pin(1, 0, (0, 0, 0))]))
    refused(lambda: h.set_pins([Pin(1, 0, (np.nan, 0, 0))]))
    refused(lambda: h.set_body_motions([BodyMotion(0, (np.inf, 0, 0))]))
    refused(lambda: h.set_body_motions([BodyMotion(0, (0, 0, 0), None, (0, np.nan, 0))]))
    refused(lambda: h.set_body_motions([BodyMotion(0, (0, 0, 0), np.diag([1.0, 1.0, -1.0]))]))
    refused(lambda: h.set_body_motions([BodyMotion(0, (0, 0, 0), 1.01 * np.eye(3))]))
    assert h.get_pins()[0].size == 0
    # a pin whose body has no motion: every substep entry point refuses, nothing runs
    h.set_pins([Pin(1, 5, (0, 0, 0))])
    h.set_body_motions([_motion(0, MOTION)])
    refused(lambda: h.substep(DT, -1))
    refused(lambda: h.run_substeps(3, DT, -1))
    refused(lambda: h.run_coupled_substeps(2, DT, [], 0.5, 1e5, 1e-4))
    for call in (lambda: h.rebuild_mapping(False), lambda: h.calc_fem_state_and_force(DT), lambda: h.particle_to_grid(DT),
                 lambda: h.update_grid(-1)):
        call()
    refused(lambda: h.grid_to_particle(DT))
    h.gpu_sync()
    assert np.array_equal(h.dump_cpu_state()[0], x0)   # (no GridToParticle has run)
    assert h.get_pins()[0].tolist() == [1]
    # a partitioned engine, in either order
    nb = 64 // 4
    refused(lambda: h.dist_init(0, 1, [0, nb], 2, 2, 2))
    h.set_pins([])
    h.dist_init(0, 1, [0, nb], 2, 2, 2)
    refused(lambda: h.set_pins([Pin(1, 0, (0, 0, 0))]))
    refused(lambda: h.set_body_motions([_motion(0, MOTION)]))
    h.destroy()
