"""Rigid bodies of the grid update (mpm_set_grid_bodies, mpm_bc = MPM_BC_BODIES) on the GPU, against the float64
reference of tests/grid_bodies.py.

What is compared and to what (the rules are conditions, not measurements):
  * a node is left out when float and double may disagree about membership or the normal (grid_bodies.undecided); at most
    1 % of the massive nodes inside some body may be left out per scene and every kind and mode keeps >= 100 nodes;
  * membership and the deciding body of every compared node: exact (a node the reference gives to no body equals the
    mpm_bc = -1 result to the bit; a node it gives to a body carries that body's update within the bound below);
  * v and v*: per node, |engine - reference| <= NOISE_FLOOR x Y (|v_in| + |v_c(x)|), where the yardstick Y of the scene is
    the largest per-node distance between the reference's formulas evaluated in float32 numpy and in float64 on the same
    inputs, relative to |v_in| + |v_c(x)|;
  * per body, force and torque impulse: |engine - reference| <= NOISE_FLOOR x (the same float32-against-float64 distance of
    the reference's sums) + half a float32 ulp of the value (mpm_external_body_force_to_host returns floats) + one
    fixed-point quantum per node, all relative to the sum of |l| (torque: of |r| |l|) over the body's compared nodes.

Measured on an MI355X (128^3 grid, a block of cloth 0.3 x 0.3 x 0.2 around each body; yardstick Y, then the engine's largest
per-node error / Y, bound NOISE_FLOOR = 4):
  scene        FIXED              SLIP_APPROACHING    SLIP               compared nodes of those inside
  half_space   2.86e-08  1.00     1.84e-07  0.87      1.84e-07  0.87     20,800 of 20,800
  sphere       2.44e-08  1.00     1.93e-07  1.16      1.93e-07  1.16      1,904 of  1,904
  box          2.45e-08  1.00     1.43e-07  0.88      1.43e-07  0.88      6,439 of  6,439
  capsule      2.44e-08  1.00     5.61e-07  0.88      5.61e-07  0.88      2,446 of  2,456
  cylinder     2.44e-08  1.00     1.63e-07  1.21      1.74e-07  1.13      3,214 of  3,216
  ellipsoid    2.44e-08  1.00     2.16e-07  0.68      2.16e-07  0.68      2,382 of  2,384
  mesh         2.45e-08  1.00     4.35e-07  0.93      4.35e-07  0.93      2,870 of  2,874
  overlap (five bodies, mixed modes)                  2.34e-07  1.08     18,042 of 18,062
(FIXED writes v_c(x): its noise is that of w x r alone, and the engine's float evaluation of it is the float32 numpy one.)
The impulse sums: yardsticks 1.1e-09 - 1.4e-08, the engine's error 1e-09 - 5.5e-08 of the sum of |l|, most of it the float32
the interface returns.
"""
import numpy as np
import pytest

from tests import grid_bodies as gb
from tests.helpers import NOISE_FLOOR

pytestmark = pytest.mark.gpu
DT = 1e-3
_RUNS = {}


def _engine(sheets, bits=gb.BITS, deterministic=False, n_acc=gb.N_ACC, material=None):
    from drake_amd import GpuMpm
    mat = None
    if material:
        mat = GpuMpm.default_material()
        for k, v in material.items():
            setattr(mat, k, v)
    g = GpuMpm(bits, mat)
    if deterministic:
        g.set_deterministic(True)
    for pos, vel, idx in sheets:
        g.add_qr_cloth(pos.copy(), vel.copy(), idx.copy())
    g.finalize()
    if n_acc:
        g.reallocate_external_bodies(n_acc)
    return g


def _front(g, dt=DT):
    g.rebuild_mapping(False)
    g.calc_fem_state_and_force(dt)
    g.particle_to_grid(dt)


def _table(g, bodies):
    """Body list -> GridBody list; a mesh body's lattice is built by the engine and its values downloaded: the header's
    definition of that surface is the interpolant ON THOSE VALUES"""
    out = []
    for b in bodies:
        sid = None
        if b.kind == gb.MESH:
            verts, tris = b.mesh
            sid = g.sdf_shape_from_mesh(verts, tris, b.cell, b.pad)
            n, lo, cell = g.sdf_shape_info(sid)
            b.lattice = (g.sdf_shape_download(sid), np.asarray(n, np.int64), lo, np.float32(cell))
        out.append(b.capi(sid))
    return out


def _run(name):
    """one engine per scene: ParticleToGrid once, then the grid update once per table (it gathers the same tile sums again)"""
    if name in _RUNS:
        return _RUNS[name]
    from drake_amd import ARR as A, BC_BODIES
    sheets, tables = gb.SCENES[name]()
    g = _engine(sheets)
    _front(g)
    d = dict(m=g.download(A.GRID_MASSES), mv=g.download(A.GRID_MOMENTUM), tables={})
    g.update_grid(-1)
    d["v_free"], d["vs_free"] = g.download(A.GRID_MOMENTUM), g.download(A.GRID_V_STAR)
    for key, bodies in tables.items():
        g.set_grid_bodies(_table(g, bodies))
        g.reallocate_external_bodies(gb.N_ACC)     # (zeroes the accumulators)
        g.update_grid(BC_BODIES)
        tau, f = g.external_body_force_to_host()
        t = dict(bodies=bodies, v=g.download(A.GRID_MOMENTUM), vs=g.download(A.GRID_V_STAR), tau=tau, f=f)
        r64 = gb.reference(d["m"], d["mv"], gb.BITS, bodies, gb.N_ACC)
        r32 = gb.reference(d["m"], d["mv"], gb.BITS, bodies, gb.N_ACC, T=gb.F32, decider=r64["decider"])
        t["r64"], t["r32"] = r64, r32
        t["und"] = gb.undecided(bodies, r64["x"], r64["decider"])
        d["tables"][key] = t
    d["mass_total"] = float(g.download(A.MASSES).astype(np.float64).sum())
    g.gpu_sync()
    assert g.stats()["error_flags"] == 0
    g.destroy()
    _RUNS[name] = d
    return d


def _norm(a):
    return np.sqrt((np.asarray(a, np.float64) ** 2).sum(-1))


CASES = [(KIND, mode) for KIND in gb.KIND_NAMES for mode in (gb.FIXED, gb.SLIP_APPROACHING, gb.SLIP)] + [("overlap", "overlap")]


@pytest.mark.parametrize("name,key", CASES)
def test_nodes_against_the_float64_reference(name, key):
    d = _run(name)
    t = d["tables"][key]
    r64, r32, und, bodies = t["r64"], t["r32"], t["und"], t["bodies"]
    on, dec = r64["on"], r64["decider"]
    share, counts = gb.check_scene_conditions(bodies, r64["x"], dec, und)
    assert share <= gb.MAX_UNDECIDED_SHARE, share
    assert all(c >= gb.MIN_COMPARED for c in counts.values()), counts
    # nodes without mass: zero velocity, as always
    off = np.ones(len(d["m"]), bool)
    off[on] = False
    assert not t["v"][off].any() and not t["vs"][off].any()
    cmp_ = ~und
    # nodes no body contains: the mpm_bc = -1 result to the bit
    free = cmp_ & (dec < 0)
    assert free.any()
    assert np.array_equal(t["v"][on][free], d["v_free"][on][free]) and np.array_equal(t["vs"][on][free], d["vs_free"][on][free])
    # nodes of a body: per node within NOISE_FLOOR x the measured float noise of the formulas
    inb = cmp_ & (dec >= 0)
    scale = _norm(r64["v_in"]) + _norm(r64["vc"])
    noise = _norm(r32["v"].astype(np.float64) - r64["v"])[inb] / scale[inb]
    Y = float(noise.max())
    assert Y > 0
    worst = 0.0
    for what in ("v", "vs"):
        err = _norm(t[what][on].astype(np.float64) - r64["v"])[inb] / scale[inb]
        worst = max(worst, float(err.max()))
    print("grid bodies %-10s %-8s compared %6d of %6d inside, yardstick %.3e, engine / yardstick %.3f"
          % (name, key, int(inb.sum()), int((dec >= 0).sum()), Y, worst / Y))
    assert worst <= NOISE_FLOOR * Y, (name, key, worst, Y)
    # membership, exactly: a compared node whose reference update is not (nearly) the identity did move
    moved64 = _norm(r64["v"] - r64["v_in"]) > 1e-4 * scale
    moved = (t["v"][on] != d["v_free"][on]).any(-1)
    assert np.array_equal(moved[inb & moved64], np.ones(int((inb & moved64).sum()), bool))
    # v and v* are the same vector
    assert np.array_equal(t["v"][on], t["vs"][on])


def _sums(mass, v_out, v_in, x, p, sel):
    """force and torque impulse of the nodes `sel` on a body with origin p, float64: (f (3,), tau (3,), sum |l|, sum |r||l|)"""
    l = -mass[sel, None] * (np.asarray(v_out, np.float64)[sel] - np.asarray(v_in, np.float64)[sel])
    r = x[sel] - np.asarray(p, np.float64)
    return l.sum(0), np.cross(r, l).sum(0), float(_norm(l).sum()), float((_norm(r) * _norm(l)).sum())


def _engine_decider(bodies, x, v_in, v_eng, v_free):
    """which body the ENGINE let decide at the (undecided) nodes x: the one whose float64 update of v_in is nearest to what
    the engine wrote; -1 where the mpm_bc = -1 value is nearest.  Only used to take these nodes out of the engine's sums."""
    best = np.full(len(x), -1)
    err = _norm(v_eng.astype(np.float64) - v_free.astype(np.float64))
    for k, b in enumerate(bodies):
        _, n = gb.body_sdf(b, x)
        e = _norm(v_eng.astype(np.float64) - gb.apply_mode(b, v_in, gb.rigid_velocity(b, x), n))
        e = np.where(np.isfinite(e), e, np.inf)
        best = np.where(e < err, k, best)
        err = np.minimum(e, err)
    return best


@pytest.mark.parametrize("name,key", CASES)
def test_reaction_against_the_float64_sums(name, key):
    """Per accumulator, over the compared nodes.  The undecided nodes' own contributions are taken out of the engine's
    sums first: the engine forms l = -m (v_out - v_in) in double from the floats it writes, so the downloaded grid gives
    them back exactly (up to the fixed-point quantum, one per node and component), and which body it let decide there
    shows in what it wrote (_engine_decider)."""
    d = _run(name)
    t = d["tables"][key]
    r64, r32, bodies, und = t["r64"], t["r32"], t["bodies"], t["und"]
    on, x = r64["on"], r64["x"]
    mass = d["m"][on].astype(np.float64)
    v_eng, v_free = t["v"][on], d["v_free"][on]
    quantum = 2.0 ** np.ceil(np.log2(d["mass_total"])) * 2.0 ** -47
    ulp = 2.0 ** -24
    ui = np.nonzero(und)[0]
    eng_dec = np.full(len(on), -2)
    eng_dec[ui] = _engine_decider(bodies, x[ui], r64["v_in"][ui], v_eng[ui], v_free[ui])
    for acc in range(gb.N_ACC):
        mine = [k for k, b in enumerate(bodies) if b.body == acc]
        if not mine:
            assert not t["tau"][acc].any() and not t["f"][acc].any()
            continue
        p = bodies[mine[0]].p
        assert all(np.array_equal(bodies[k].p, p) for k in mine)
        sel = np.isin(r64["decider"], mine) & ~und
        f64, tau64, absl, absrl = _sums(mass, r64["v"], r64["v_in"], x, p, sel)
        f32, tau32, _, _ = _sums(mass, r32["v"], r32["v_in"], x, p, sel)
        assert absl > 0
        fu, tauu, _, _ = _sums(mass, v_eng, v_free, x, p, np.isin(eng_dec, mine))
        n_nodes = int(sel.sum()) + int(und.sum())
        rmax = float(_norm(x[sel] - p.astype(np.float64)).max())
        for what, want, want32, corr, unit, q in (("f", f64, f32, fu, absl, quantum), ("tau", tau64, tau32, tauu, absrl, quantum * rmax)):
            Y = float(np.abs(want32 - want).max()) / unit
            got = t[what][acc].astype(np.float64)
            err = float(np.abs(got - corr - want).max()) / unit
            bound = NOISE_FLOOR * Y + (ulp * float(np.abs(got).max()) + n_nodes * q) / unit
            print("grid bodies %-10s %-8s body %d %-3s yardstick %.3e, engine error %.3e, bound %.3e"
                  % (name, key, acc, what, Y, err, bound))
            assert err <= bound, (name, key, acc, what, err, bound)
    assert t["f"].shape == (gb.N_ACC, 3)


@pytest.mark.parametrize("name", ["sphere", "box", "cylinder", "mesh"])
def test_momentum_identity_over_one_grid_update(name):
    """sum m (v_out - v_walls) = - sum over bodies of l, in float64 from the downloaded grid.  Bound from its parts: every
    contributing node component is rounded once to the fixed-point quantum of the momentum scale (M 2^-47 with M the
    total mass rounded up to a power of two; half a quantum each, taken whole), the products m (v_out - v_in) are formed
    in double from floats (2^-52 relative each) and the sum is returned as float32 (half an ulp)."""
    d = _run(name)
    t = d["tables"][gb.SLIP]
    on = t["r64"]["on"]
    m = d["m"][on].astype(np.float64)
    dv = t["v"][on].astype(np.float64) - d["v_free"][on].astype(np.float64)
    contrib = (dv != 0).any(-1)
    dp = (m[:, None] * dv).sum(0)
    quantum = 2.0 ** np.ceil(np.log2(d["mass_total"])) * 2.0 ** -47
    absl = float((m * _norm(dv)).sum())
    bound = contrib.sum() * quantum + absl * 2.0 ** -52 * 4 + np.abs(t["f"][0]).max() * 2.0 ** -24
    err = np.abs(dp + t["f"][0].astype(np.float64)).max()
    print("momentum identity %-8s nodes %d, |dp| %.3e, error %.3e, bound %.3e" % (name, int(contrib.sum()), _norm(dp), err, bound))
    assert contrib.sum() >= gb.MIN_COMPARED and err <= bound, (err, bound)


# ---- equivalences with the presets, to the bit --------------------------------------------------------------------------------
def _preset_bodies(bc, friction=-1.0):
    """the scenes of mpm_bc = 1, 2, 3 (mpm_grid_collider_preset) as bodies"""
    if bc == 2:
        return [gb.Body(gb.HALF_SPACE, p=(0, 0, 0.11), mode=gb.SLIP, friction=friction)]
    if bc == 1:
        return [gb.Body(gb.SPHERE, p=(0.38, y, 0.75), dims=(0.04, 0, 0), mode=gb.FIXED, friction=friction) for y in (0.38, 0.62)]
    return [gb.Body(gb.SPHERE, p=(x, y, 0.5), dims=(0.02, 0, 0), mode=gb.FIXED, friction=friction)
            for y in (0.3, 0.7) for x in (0.3, 0.7)]


@pytest.mark.parametrize("bc", [2, 1, 3])
def test_bodies_reproduce_the_presets_to_the_bit(bc):
    """A half-space body (R_WB = identity, p_WB on the plane) is mpm_bc = 2's plane, sphere bodies are the spheres of
    mpm_bc = 1 and 3: with w = 0 the body-frame evaluation multiplies by exact ones and zeros, and the same formulas
    follow -- the grid, and after GridToParticle the particles, to the bit."""
    from drake_amd import ARR as A, BC_BODIES, scenes
    z0, side = {2: 0.105, 1: 0.74, 3: 0.49}[bc], {2: 0.3, 1: 0.4, 3: 0.5}[bc]
    sheets = scenes.cloth_stack(6, 40, 6, z0=z0, side=side, seed=5, vel_amp=0.3)
    for _, vel, _ in sheets:
        vel[:, 2] -= 0.4
    a, b = _engine(sheets, 6, True, 0), _engine(sheets, 6, True, 0)
    b.set_grid_bodies(_table(b, _preset_bodies(bc)))
    for g, code in ((a, bc), (b, BC_BODIES)):
        _front(g)
        g.update_grid(code)
    va, vb = a.download(A.GRID_MOMENTUM), b.download(A.GRID_MOMENTUM)
    a2 = _engine(sheets, 6, True, 0)
    _front(a2)
    a2.update_grid(-1)
    acted = (va != a2.download(A.GRID_MOMENTUM)).any(-1).sum()
    assert acted >= 20, acted                  # (the preset's collider does act on this scene)
    assert np.array_equal(va.view(np.uint32), vb.view(np.uint32))
    assert np.array_equal(a.download(A.GRID_V_STAR).view(np.uint32), b.download(A.GRID_V_STAR).view(np.uint32))
    for g in (a, b):
        g.grid_to_particle(DT)
    for g, code in ((a, bc), (b, BC_BODIES)):
        g.run_substeps(5, DT, code)
    for arr in (A.POSITIONS, A.VELOCITIES, A.AFFINE, A.DEFORMATION_GRADIENTS):
        assert np.array_equal(a.download(arr).view(np.uint32), b.download(arr).view(np.uint32)), arr
    for g in (a, b, a2):
        g.destroy()


# ---- reaction and paths, deterministic mode -----------------------------------------------------------------------------------
def _falling(bits=6, speed=5.0, seed=17):
    """a cloth block falling fast through three bodies: re-sorts within ten substeps"""
    sheets = gb.slab(bits, center=(0.5, 0.5, 0.5), side=0.3, thickness=0.1, seed=seed, v0=(0.3, 0.0, -speed), vel_amp=0.2)
    bodies = [
        gb.Body(gb.BOX, body=0, p=(0.5, 0.5, 0.45), R=gb.rot((1, 2, 0.5), 0.7), dims=(0.11, 0.07, 0.05), v=(0, 0.1, 0), w=(0, 0, 2.0),
                mode=gb.SLIP, friction=0.3),
        gb.Body(gb.CYLINDER, body=1, p=(0.42, 0.5, 0.5), R=gb.rot((1, 0.3, 0.2), 1.1), dims=(0.07, 0.05, 0), w=(0.5, 0.5, -1),
                mode=gb.FIXED),
        gb.Body(gb.ELLIPSOID, body=2, p=(0.58, 0.55, 0.5), R=gb.rot((0.5, -1, 0.7), 0.8), dims=(0.10, 0.06, 0.045), v=(0, 0, 0.2),
                mode=gb.SLIP_APPROACHING, friction=0.5),
    ]
    return sheets, bodies


def _state(g):
    from drake_amd import ARR as A
    tau, f = g.external_body_force_to_host()
    return dict(pos=g.download(A.POSITIONS), vel=g.download(A.VELOCITIES), C=g.download(A.AFFINE),
                F=g.download(A.DEFORMATION_GRADIENTS), tau=tau, f=f)


def _same(a, b):
    for k in a:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


def _phase_substeps(g, n, dt, bc):
    for _ in range(n):
        _front(g, dt)
        g.update_grid(bc)
        g.grid_to_particle(dt)


def test_batch_equals_phase_calls_state_and_impulses_through_a_resort():
    """Deterministic mode: a 10-substep mpm_run_substeps batch against ten phase-by-phase substeps -- particle state and the
    bodies' impulses to the bit, a re-sort inside the batch included (a substep that gates itself out adds nothing, its
    replay adds once); and two engines fed the same state report identical bits."""
    from drake_amd import BC_BODIES
    sheets, bodies = _falling()
    a, b, c = (_engine(sheets, 6, True, 3) for _ in range(3))
    for g in (a, b, c):
        g.set_grid_bodies(_table(g, bodies))
    _phase_substeps(a, 10, DT, BC_BODIES)
    b.run_substeps(10, DT, BC_BODIES)
    c.run_substeps(10, DT, BC_BODIES)
    for g in (a, b, c):
        g.gpu_sync()
    sa, sb, sc = _state(a), _state(b), _state(c)
    assert (np.abs(sa["f"]).sum(axis=1) > 0).all() and (np.abs(sa["tau"]).sum(axis=1) > 0).all()   # every body received something
    assert b.stats()["rebuilds"] > 1, b.stats()        # (a re-sort inside the batch)
    _same(sa, sb)
    _same(sb, sc)
    for g in (a, b, c):
        assert g.stats()["error_flags"] == 0
        g.destroy()


def test_coupled_substeps_with_bodies_equal_the_seven_calls():
    """mpm_run_coupled_substeps with MPM_BC_BODIES and a contact collider that makes pairs, against the seven calls per
    substep: the state, and the grid bodies' and the contact solve's impulses in the same accumulators, to the bit."""
    from drake_amd import BC_BODIES, Collider
    sheets, bodies = _falling(speed=0.6)
    dt, mu, k, dmp = 2e-4, 1.0, 1e6, 1e-5
    floor = [Collider(0, body=3, p_WB=(0.5, 0.5, 0.47))]
    a, b = _engine(sheets, 6, True, 4), _engine(sheets, 6, True, 4)
    ra = []
    for g in (a, b):
        g.set_grid_bodies(_table(g, bodies))
    for _ in range(8):
        _front(a, dt)
        a.update_grid(BC_BODIES)
        a.generate_contact_pairs(floor, want_count=False)
        ra.append(a.update_contact(dt, mu, k, dmp))
        a.grid_to_particle(dt)
    rb = b.run_coupled_substeps(3, dt, floor, mu, k, dmp, mpm_bc=BC_BODIES) + \
        b.run_coupled_substeps(5, dt, floor, mu, k, dmp, mpm_bc=BC_BODIES)
    for g in (a, b):
        g.gpu_sync()
    assert [r["contacts"] for r in ra] == [r["contacts"] for r in rb] and ra[0]["contacts"] > 0
    assert [r["iterations"] for r in ra] == [r["iterations"] for r in rb]
    sa, sb = _state(a), _state(b)
    assert np.abs(sa["f"][3]).sum() > 0 and np.abs(sa["f"][0]).sum() > 0     # the contact body and a grid body
    _same(sa, sb)
    for g in (a, b):
        assert g.stats()["error_flags"] == 0
        g.destroy()


def test_a_table_changed_between_batches_leaves_owed_substeps_their_table():
    """Two batches with a different table each, nothing synchronised in between: substeps of the first batch that gated
    themselves out are run with the first table before the second takes effect (the version rule).  Against phase calls."""
    from drake_amd import BC_BODIES
    sheets, bodies = _falling()
    second = [gb.Body(gb.SPHERE, body=1, p=(0.5, 0.5, 0.42), R=gb.rot((0.3, 1, 0.2), 0.9), dims=(0.09, 0, 0), v=(0, 0, 0.5),
                      w=(0, 3, 0), mode=gb.SLIP, friction=0.2)]
    a, b = _engine(sheets, 6, True, 3), _engine(sheets, 6, True, 3)
    a.set_grid_bodies(_table(a, bodies))
    _phase_substeps(a, 8, DT, BC_BODIES)
    a.set_grid_bodies(_table(a, second))
    _phase_substeps(a, 8, DT, BC_BODIES)
    b.set_grid_bodies(_table(b, bodies))
    b.run_substeps(8, DT, BC_BODIES)
    b.set_grid_bodies(_table(b, second))
    b.run_substeps(8, DT, BC_BODIES)
    for g in (a, b):
        g.gpu_sync()
    assert b.stats()["rebuilds"] > 1
    _same(_state(a), _state(b))
    got = b.get_grid_bodies()
    assert len(got) == 1 and got[0].shape.kind == gb.SPHERE and got[0].shape.body == 1
    # an empty table behaves as mpm_bc = -1
    a.set_grid_bodies([])
    b.set_grid_bodies([])
    a.run_substeps(3, DT, BC_BODIES)
    b.run_substeps(3, DT, -1)
    for g in (a, b):
        g.gpu_sync()
    _same(_state(a), _state(b))
    for g in (a, b):
        g.destroy()


# ---- behaviour ---------------------------------------------------------------------------------------------------------------
def test_a_cloth_lands_on_a_box_as_on_the_plane():
    """A cloth released above a fixed, axis-aligned box whose top face it lands wholly upon sinks no deeper below that face
    than the same cloth sinks below the mpm_bc = 2-style plane of mpm_set_grid_colliders at the face's height (same mode
    and friction), plus a quarter of a cell."""
    from drake_amd import ARR as A, BC_BODIES, BC_TABLE, GridCollider, scenes
    bits, top = 6, 0.4
    dx = 1.0 / (1 << bits)
    sheets = scenes.cloth_stack(2, 30, bits, z0=top + 2.5 * dx, side=0.2, seed=3, vel_amp=0.02)
    a, b = _engine(sheets, bits, False, 1), _engine(sheets, bits, False, 1)
    a.set_grid_colliders([GridCollider(1, gb.SLIP, p=(0, 0, top), n=(0, 0, 1), friction=0.5)])
    box = gb.Body(gb.BOX, body=0, p=(0.5, 0.5, top - 0.1), dims=(0.2, 0.2, 0.1), mode=gb.SLIP, friction=0.5)
    b.set_grid_bodies(_table(b, [box]))
    n = 400
    a.run_substeps(n, DT, BC_TABLE)
    b.run_substeps(n, DT, BC_BODIES)
    za, zb = a.download(A.POSITIONS)[:, 2], b.download(A.POSITIONS)[:, 2]
    xb = b.download(A.POSITIONS)
    assert np.abs(xb[:, :2] - 0.5).max() < 0.2 - 2 * dx      # it landed wholly upon the face
    assert za.min() < top + 2 * dx                           # ... and did reach the collider's layer of nodes
    sink_a, sink_b = max(top - float(za.min()), 0.0), max(top - float(zb.min()), 0.0)
    print("sink below the face: plane %.5f, box %.5f (cell %.5f)" % (sink_a, sink_b, dx))
    assert sink_b <= sink_a + 0.25 * dx
    _, f = b.external_body_force_to_host()
    assert f[0, 2] < 0                                       # the cloth pushes the box down
    for g in (a, b):
        assert g.stats()["error_flags"] == 0
        g.destroy()


def test_a_fixed_spinning_cylinder_gives_its_nodes_w_cross_r():
    """FIXED writes v_c(x), whatever the node's own velocity was: every decided node of a cylinder spinning about its
    axis carries w x r -- the float32 value of the reference's formula within the rounding of its five operations per
    component (a cross product's two products and difference, the sum with v = 0; fused or not: 4 ulp of |w| |r|)."""
    from drake_amd import ARR as A, BC_BODIES
    sheets, _ = gb.kind_scene(gb.CYLINDER)
    R = gb.rot((1, 0.3, 0.2), 1.1)
    axis = R[:, 2].astype(np.float64)
    cyl = gb.Body(gb.CYLINDER, p=(0.5, 0.5, 0.5), R=R, dims=(0.07, 0.05, 0), w=tuple(np.float32(6.0) * R[:, 2]), mode=gb.FIXED)
    g = _engine(sheets)
    _front(g)
    g.set_grid_bodies(_table(g, [cyl]))
    g.update_grid(BC_BODIES)
    vs = g.download(A.GRID_V_STAR)
    m, mv = g.download(A.GRID_MASSES), g.download(A.GRID_MOMENTUM)
    r64 = gb.reference(m, mv * 0, gb.BITS, [cyl], 1)
    und = gb.undecided([cyl], r64["x"], r64["decider"])
    sel = (r64["decider"] == 0) & ~und
    assert sel.sum() >= gb.MIN_COMPARED
    r = r64["x"][sel] - 0.5
    want = np.cross(cyl.w.astype(np.float64), r)
    got = vs[r64["on"]][sel].astype(np.float64)
    bound = 4 * 2.0 ** -24 * np.linalg.norm(cyl.w.astype(np.float64)) * _norm(r)
    assert (np.abs(got - want).max(-1) <= bound).all()
    assert np.abs((got * axis).sum(-1)).max() <= bound.max()     # no velocity along the axis
    g.destroy()


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_table_in_force():
    from drake_amd import BC_BODIES, MpmError, scenes
    sheets = scenes.cloth_stack(2, 16, 6, z0=0.5, side=0.3)
    g = _engine(sheets, 6, False, 1)
    good = [gb.Body(gb.SPHERE, p=(0.5, 0.5, 0.5), dims=(0.05, 0, 0), mode=gb.SLIP, friction=0.4)]
    g.set_grid_bodies(_table(g, good))

    def refused(bodies, shape_ids=None):
        table = [b.capi((shape_ids or {}).get(k)) for k, b in enumerate(bodies)]
        with pytest.raises(MpmError) as e:
            g.set_grid_bodies(table)
        assert e.value.code == -1, e.value
        got = g.get_grid_bodies()
        assert len(got) == 1 and got[0].shape.kind == gb.SPHERE and got[0].mode == gb.SLIP and abs(got[0].friction - 0.4) < 1e-7

    ok = dict(p=(0.5, 0.5, 0.5), dims=(0.05, 0.05, 0.05))
    refused([gb.Body(gb.SPHERE, **ok)] * 17)
    refused([gb.Body(7, **ok)])                                   # a kind outside 0-5
    refused([gb.Body(-1, **ok)])
    refused([gb.Body(gb.CYLINDER, p=(0.5, 0.5, 0.5), dims=(0.05, 0.0, 0))])
    refused([gb.Body(gb.CYLINDER, p=(0.5, 0.5, 0.5), dims=(np.inf, 0.1, 0))])
    refused([gb.Body(gb.ELLIPSOID, p=(0.5, 0.5, 0.5), dims=(0.05, 0.05, -0.01))])
    refused([gb.Body(gb.ELLIPSOID, p=(0.5, 0.5, 0.5), dims=(0.05, np.nan, 0.01))])
    m = gb.Body(gb.MESH, **ok)
    refused([m], {0: 12345})                                      # an unknown shape id
    refused([gb.Body(gb.SPHERE, mode=3, **ok)])
    refused([gb.Body(gb.SPHERE, mode=-1, **ok)])
    refused([gb.Body(gb.SPHERE, friction=np.nan, **ok)])
    refused([gb.Body(gb.SPHERE, friction=np.inf, **ok)])
    refused([gb.Body(gb.SPHERE, p=(np.nan, 0, 0), dims=(0.05, 0, 0))])
    refused([gb.Body(gb.SPHERE, v=(0, np.inf, 0), **ok)])
    refused([gb.Body(gb.SPHERE, w=(0, 0, np.nan), **ok)])
    refused([gb.Body(gb.SPHERE, R=2 * np.eye(3), **ok)])
    refused([gb.Body(gb.SPHERE, R=np.diag([1, 1, -1]), **ok)])    # a reflection
    refused([gb.Body(gb.SPHERE, R=gb.rot((1, 2, 3), 0.3) + np.float32(3e-4), **ok)])
    bad = np.eye(3)
    bad[0, 0] = np.nan
    refused([gb.Body(gb.SPHERE, R=bad, **ok)])
    # the table in force still runs; a negative friction selects the material's; an unknown mpm_bc is still refused
    g.run_substeps(2, DT, BC_BODIES)
    g.set_grid_bodies(_table(g, [gb.Body(gb.SPHERE, p=(0.5, 0.5, 0.5), dims=(0.05, 0, 0), mode=gb.SLIP, friction=-1.0)]))
    g.run_substeps(2, DT, BC_BODIES)
    with pytest.raises(MpmError):
        g.run_substeps(1, DT, 6)
    g.gpu_sync()
    assert g.stats()["error_flags"] == 0
    # partitioned engines, both ways
    nb = 64 // 4
    with pytest.raises(MpmError) as e:
        g.dist_init(0, 1, [0, nb], 2, 2, 2)
    assert e.value.code == -1
    g.set_grid_bodies([])
    g.dist_init(0, 1, [0, nb], 2, 2, 2)
    with pytest.raises(MpmError) as e:
        g.set_grid_bodies(_table(g, good))
    assert e.value.code == -1 and g.get_grid_bodies() == []
    g.destroy()


def test_profile_substeps_takes_the_bodies():
    from drake_amd import BC_BODIES
    sheets, bodies = _falling(speed=0.5)
    a, b = _engine(sheets, 6, True, 3), _engine(sheets, 6, True, 3)
    for g in (a, b):
        g.set_grid_bodies(_table(g, bodies))
    a.profile_substeps(4, DT, BC_BODIES)
    _phase_substeps(b, 4, DT, BC_BODIES)
    for g in (a, b):
        g.gpu_sync()
    _same(_state(a), _state(b))
    for g in (a, b):
        g.destroy()
