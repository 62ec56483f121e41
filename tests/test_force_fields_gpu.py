"""External force fields (mpm_set_force_fields) on the engine.

1. ParticleToGrid node by node against the float64 restatement of tests/force_fields.py on the layouts dense, kinds,
   materials and magnitudes of tests/transfer_layouts.py, every field table, default and deterministic mode: grid mass
   and momentum within the extended bound K (L_n + 16 + R) u A_n + N_n q, touched flags bit-exact, total momentum
   against the particle sums plus sum m a dt.  The inputs are the engine's own after the FEM call, the directors
   F[:,2] included.  (The layout `materials` is a multi-material engine: fields with per-cloth materials.)
2. The fused instance k_p2g<1, 1, 1> (mpm_substep) is bit-equal to the phase calls on a twin engine.
3. No table, no change: an engine that set and cleared a table is bit-identical to one that never had one; a table
   that adds zero agrees with both.
4. Terminal speed under DRAG against the float64 recurrence, 5. hover under ACCEL = -g, 6. scheduling through re-sorts,
7. the coupled path, 8. combinations (pins, grid bodies) and refusals."""
import numpy as np
import pytest

from tests import force_fields as ff
from tests import harness as hs
from tests import transfer_layouts as tl

pytestmark = pytest.mark.gpu

LAYOUTS = ("dense", "kinds", "materials", "magnitudes")
MODES = ("default", "deterministic")
DT = tl.DT
G32 = float(np.float32(-9.8))
U = 2.0 ** -24
_RUNS = {}


def _c(fields):
    from drake_amd import ForceField
    return [ForceField(kind=f["kind"], gamma=float(f["gamma"]), u0=f["u0"], G=f["G"], x0=f["x0"],
                       region=(f["lo"], f["hi"]) if f["flags"] & ff.FF_REGION else None, flags=f["flags"]) for f in fields]


def _layout_engine(name, table, mode):
    from tests import test_transfer_layouts_gpu as ttl
    lay = tl.layout(name)
    g = ttl._engine(lay, mode)
    fields = ff.table(table, *ff.bbox(lay["pos"]))
    g.set_force_fields(_c(fields))
    return lay, fields, g


def _run(name, table, mode):
    """the phase calls with the table set, a download after the FEM call and after each later phase (slot order)"""
    key = (name, table, mode)
    if key in _RUNS:
        return _RUNS[key]
    A = hs.ARR()
    lay, fields, g = _layout_engine(name, table, mode)
    g.rebuild_mapping(False)
    g.calc_fem_state_and_force(DT)
    d = dict(lay=lay, fields=fields)
    for k, a in (("pids", A.PIDS), ("x", A.POSITIONS), ("v", A.VELOCITIES), ("C", A.AFFINE), ("m", A.MASSES),
                 ("taus", A.TAUS), ("f", A.FORCES), ("F", A.DEFORMATION_GRADIENTS)):
        d[k] = g.download(a)
    g.particle_to_grid(DT)
    d["gm"], d["gmv"], d["flags"] = g.download(A.GRID_MASSES), g.download(A.GRID_MOMENTUM), g.download(A.GRID_TOUCHED_FLAGS)
    g.update_grid(-1)
    g.grid_to_particle(DT)
    d["x1"], d["v1"], d["C1"] = g.download(A.POSITIONS), g.download(A.VELOCITIES), g.download(A.AFFINE)
    d["stats"] = g.stats()
    g.destroy()
    _RUNS[key] = d
    return d


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("table", ff.TABLES)
@pytest.mark.parametrize("name", LAYOUTS)
def test_p2g_with_fields_node_by_node(name, table, mode):
    from tests import helpers
    from tests import test_transfer_layouts_gpu as ttl
    helpers.tag_default_engine(mode == "default")
    d = _run(name, table, mode)
    lay, fields = d["lay"], d["fields"]
    nf, bits = lay["nf"], lay["bits"]
    assert d["stats"]["error_flags"] == 0, d["stats"]
    assert np.array_equal(np.sort(d["pids"]), np.arange(nf + lay["nv"]))
    x, v, C, m, taus, f = ttl._p2g_inputs(d)
    face = d["pids"] < nf
    # the director of a face particle: column 2 of its deformation gradient (original face order), as k_fem left it
    Fc = d["F"].reshape(nf, 3, 3)[:, :, 2]
    dirs = np.zeros((len(face), 3), np.float32)
    dirs[face] = Fc[d["pids"][face]]
    r, a64, T = ff.p2g64_fields(fields, x, v, C, m, taus, f, dirs, face, bits, lay["gravity_axis"])
    assert (T > 0).any(), "the table reaches no particle of the layout"
    quanta = tl.fixed_quanta(m) if mode != "default" else None
    bm, bmv = ff.p2g_bounds(r, quanta)
    fails = []

    def check(field, err, bound):
        w = tl.margin(err, bound)
        hs.record(f"force fields: {name} {table} [{mode}] {field}", w)
        print(f"force fields: {name} {table} [{mode}] {field}: {w:.4g} of the bound")
        if not w <= 1.0:
            fails.append(f"{field}: {w:.3g} x the bound")

    check("p2g mass", np.abs(d["gm"] - r["m"]), bm)
    check("p2g momentum", np.abs(d["gmv"] - r["mv"]), bmv)
    assert np.array_equal(d["flags"], r["flags"]), "GRID_TOUCHED_FLAGS"
    m64 = np.asarray(m, np.float64)
    ext = m64[:, None] * v + np.asarray(f, np.float64) * tl.DT32 + m64[:, None] * a64 * tl.DT32
    ext[:, lay["gravity_axis"]] += m64 * tl.GRAVITY * tl.DT32
    check("p2g total momentum", np.abs(d["gmv"].astype(np.float64).sum(axis=0) - ext.sum(axis=0)),
          bmv.sum(axis=0) + 1e-12 * np.abs(ext).sum(axis=0))
    # the fields are in the sums: without them the momentum is far outside the bound
    r0, _, _ = ff.p2g64_fields(fields, x, v, C, m, taus, f, dirs, face, bits, lay["gravity_axis"], accel=np.zeros_like(a64))
    assert tl.margin(np.abs(d["gmv"] - r0["mv"]), bmv) > 10
    assert not fails, f"{name} {table} [{mode}]:\n" + "\n".join(fails)


@pytest.mark.parametrize("name", LAYOUTS)
def test_fused_instance_equals_phase_calls(name):
    """deterministic mode: mpm_substep (k_p2g<1, 1, 1>) is bit-equal to the phase calls (k_vforce, k_p2g<0, 1, 1>)"""
    A = hs.ARR()
    d = _run(name, "eight", "deterministic")
    _, _, g = _layout_engine(name, "eight", "deterministic")
    g.substep(DT, -1)
    assert g.stats()["error_flags"] == 0
    assert np.array_equal(g.download(A.PIDS), d["pids"])
    for k, a in (("x1", A.POSITIONS), ("v1", A.VELOCITIES), ("C1", A.AFFINE)):
        got = g.download(a)
        assert np.array_equal(got.view(np.uint32), d[k].view(np.uint32)), (k, float(np.abs(got - d[k]).max()))
    g.destroy()


# ---- scenes of whole sheets ----------------------------------------------------------------------------------------
def _flat_sheet(res=24, side=0.3, z=0.6, center=(0.5, 0.5), vel=(0.0, 0.0, 0.0)):
    from drake_amd import scenes
    pos, idx = scenes.cloth_sheet(res, side, z, center)
    v = np.broadcast_to(np.asarray(vel, np.float32), pos.shape).copy()
    return [(pos, v, idx)]


def test_no_table_no_change():
    """40 deterministic substeps through at least two re-sorts: never set == set and cleared, to the bit, in x, v, C and
    F; an ACCEL field with u0 = 0 and G = 0 (the FIELDS instance adding zero) agrees within RTOL of max|v|"""
    from drake_amd import ForceField
    from tests import helpers
    sheets = _flat_sheet(res=32, side=0.3, z=0.6, center=(0.3, 0.5), vel=(4.0, 0.3, 0.0))
    sheets[0][1][:] += 0.05 * np.random.default_rng(3).normal(size=sheets[0][1].shape).astype(np.float32)
    never, cleared, zero = (hs.engine(sheets) for _ in range(3))
    cleared.set_force_fields(_c(ff.table("eight")))
    assert len(cleared.get_force_fields()) == 8
    cleared.set_force_fields([])
    assert cleared.get_force_fields() == []
    zero.set_force_fields([ForceField()])
    before = never.stats()["rebuilds"]
    for g in (never, cleared, zero):
        for _ in range(4):
            g.run_substeps(10, DT, -1)
        g.gpu_sync()
        assert g.stats()["error_flags"] == 0
    assert never.stats()["rebuilds"] - before >= 2, never.stats()
    a, b, c = hs.state(never), hs.state(cleared), hs.state(zero)
    hs.same_bits(a, b, "set and cleared")
    assert np.array_equal(a["pids"], c["pids"])
    vmax = float(np.abs(a["v"]).max())
    helpers.close(c["v"], a["v"], scale=vmax, what="force fields: zero table v")
    helpers.close(c["x"], a["x"], scale=1.0, what="force fields: zero table x")
    for g in (never, cleared, zero):
        g.destroy()


def _vertex_velocities(g, nf):
    A = hs.ARR()
    return g.download(A.VELOCITIES)[g.download(A.PIDS) >= nf].astype(np.float64)


def test_terminal_speed():
    """a flat horizontal sheet with uniform velocity under gravity and DRAG gamma towards a uniform wind: nothing
    deforms, every vertex follows v_{k+1} = v_k + dt (g e - gamma (v_k - w)).  Tolerance: the larger of RTOL max|v| and
    4 x the error the same engine shows on the same scene with gamma = 0 against v_0 + k g dt."""
    from drake_amd import FF_DRAG, ForceField
    from tests import helpers
    v0, w, gamma, n = np.array([0.5, -0.2, 0.3]), np.array([1.0, 0.5, 0.2]), 8.0, 200
    dt, g32 = float(np.float32(DT)), G32
    e = np.array([0.0, 0.0, 1.0])
    out = {}
    for gam in (0.0, gamma):
        sheets = _flat_sheet(res=24, side=0.25, z=0.75, center=(0.4, 0.45), vel=v0)
        g = hs.engine(sheets)
        nf = len(sheets[0][2]) // 3
        g.set_force_fields([ForceField(FF_DRAG, gamma=gam, u0=w)])
        for _ in range(n // 20):
            g.run_substeps(20, DT, -1)
        g.gpu_sync()
        assert g.stats()["error_flags"] == 0
        out[gam] = _vertex_velocities(g, nf)
        g.destroy()
    yard = float(np.abs(out[0.0] - (v0 + n * g32 * dt * e)[None]).max())
    ref = v0.astype(np.float32).astype(np.float64)
    g64, w64 = float(np.float32(gamma)), w.astype(np.float32).astype(np.float64)
    for _ in range(n):
        ref = ref + dt * (g32 * e - g64 * (ref - w64))
    vmax = float(np.abs(ref).max())
    err = float(np.abs(out[gamma] - ref[None]).max())
    tol = max(helpers.RTOL * vmax, 4.0 * yard)
    print(f"terminal speed: err {err:.3e}, yardstick (gamma = 0) {yard:.3e}, RTOL max|v| {helpers.RTOL * vmax:.3e}")
    hs.record("force fields: terminal speed", err / tol)
    # the drag matters: without it the sheet would be far from the recurrence
    assert float(np.abs(out[0.0] - ref[None]).max()) > 100 * tol
    assert err <= tol, (err, tol, yard)


def test_hover():
    """ACCEL u0 = -g e cancels gravity: a sheet at rest keeps |v| below 50 x 4u x |g| dt over 50 substeps"""
    from drake_amd import ForceField
    sheets = _flat_sheet(res=24, side=0.3, z=0.6)
    g = hs.engine(sheets)
    g.set_force_fields([ForceField(u0=(0.0, 0.0, -G32))])
    g.run_substeps(50, DT, -1)
    g.gpu_sync()
    assert g.stats()["error_flags"] == 0
    v = float(np.abs(g.download(hs.ARR().VELOCITIES)).max())
    bound = 50 * 4 * U * abs(G32) * float(np.float32(DT))
    print(f"hover: max|v| {v:.3e}, bound {bound:.3e}")
    hs.record("force fields: hover", v / bound)
    assert v <= bound, (v, bound)
    # (without the field the sheet falls: 50 substeps of gravity)
    h = hs.engine(sheets)
    h.run_substeps(50, DT, -1)
    assert float(np.abs(h.download(hs.ARR().VELOCITIES)).max()) > 0.4
    for s in (g, h):
        s.destroy()


def test_scheduling_through_resorts():
    """ACCEL of 5 g sideways inside a region the cloth enters and leaves forces several re-sorts: in deterministic mode
    mpm_run_substeps(h, 120) is bit-equal to 120 mpm_substep calls"""
    from drake_amd import ForceField
    sheets = _flat_sheet(res=24, side=0.2, z=0.6, center=(0.3, 0.5), vel=(2.5, 0.0, 0.0))
    field = ForceField(u0=(-5.0 * G32, 0.0, 0.0), region=((0.45, 0.0, 0.0), (0.5, 1.0, 1.0)))
    a, b = hs.engine(sheets), hs.engine(sheets)
    for g in (a, b):
        g.set_force_fields([field])
    before = a.stats()["rebuilds"]
    a.run_substeps(120, DT, -1)
    for _ in range(120):
        b.substep(DT, -1)
    for g in (a, b):
        g.gpu_sync()
        assert g.stats()["error_flags"] == 0, g.stats()
    assert a.stats()["rebuilds"] - before >= 3, a.stats()
    sa, sb = hs.state(a), hs.state(b)
    hs.same_bits(sa, sb, "run_substeps(120) against 120 substeps")
    # the cloth went through the region: it ends faster than it started
    assert float(sa["v"][:, 0].min()) > 2.6, float(sa["v"][:, 0].min())
    for g in (a, b):
        g.destroy()


def test_coupled_path():
    """mpm_run_coupled_substeps on a floor, device pairs, deterministic: material gravity g plus ACCEL u0 = g e against
    material gravity 2 g without a table -- the same contact count per substep, the summed body impulse within
    IMPULSE_RTOL, positions within RTOL.  (The two engines form the same impulse with different roundings, m g dt twice
    against m 2 g dt once, so their states differ in the last bits: the scene is a flat sheet over a flat floor, whose
    particles all cross the floor's surface in the same substep, and not a jittered one, where some particle is always
    within those bits of the surface when a substep starts.)"""
    from drake_amd import Collider, ForceField
    from tests import helpers
    sheets = _flat_sheet(res=24, side=0.3, z=0.492)
    floor = [Collider(0, body=0, p_WB=(0.5, 0.5, 0.49))]
    a = hs.engine(sheets, material=dict(gravity=G32), bodies=1)
    b = hs.engine(sheets, material=dict(gravity=2.0 * G32), bodies=1)
    a.set_force_fields([ForceField(u0=(0.0, 0.0, G32))])
    n = 40
    ra = a.run_coupled_substeps(n, DT, floor, 0.5, 1e5, 1e-4)
    rb = b.run_coupled_substeps(n, DT, floor, 0.5, 1e5, 1e-4)
    for g in (a, b):
        g.gpu_sync()
        assert g.stats()["error_flags"] == 0
    print("coupled path, contacts per substep:", [r["contacts"] for r in ra], [r["contacts"] for r in rb])
    assert [r["contacts"] for r in ra] == [r["contacts"] for r in rb]
    assert max(r["contacts"] for r in ra) > 0, "the sheet never reached the floor"
    (_, fa), (_, fb) = a.external_body_force_to_host(), b.external_body_force_to_host()
    assert float(np.abs(fb).max()) > 0
    helpers.close(fa, fb, scale=float(np.abs(fb).max()), rtol=helpers.IMPULSE_RTOL, what="force fields: coupled body impulse")
    A = hs.ARR()
    assert np.array_equal(a.download(A.PIDS), b.download(A.PIDS))
    helpers.close(a.download(A.POSITIONS), b.download(A.POSITIONS), scale=1.0, what="force fields: coupled positions")
    # (and the field is what makes them agree: engine A without it falls half as fast)
    c = hs.engine(sheets, material=dict(gravity=G32), bodies=1)
    rc = c.run_coupled_substeps(n, DT, floor, 0.5, 1e5, 1e-4)
    assert [r["contacts"] for r in rc] != [r["contacts"] for r in rb]
    for g in (a, b, c):
        g.destroy()


def test_combinations_run():
    """a table together with pins and with grid bodies: 20 substeps, error_flags == 0 (per-cloth materials: the layout
    `materials` of test_p2g_with_fields_node_by_node is a multi-material engine)"""
    from drake_amd import BC_BODIES, BodyMotion, ClothMaterial, Collider, GpuMpm, GridBody, Pin
    fields = _c(ff.table("eight"))
    # pins
    sheets = _flat_sheet(res=20, side=0.3, z=0.6)
    g = hs.engine(sheets, bodies=1)
    x, _ = g.dump_cpu_state()
    g.set_body_motions([BodyMotion(0, (0, 0, 0), np.eye(3).ravel(), (0, 0, 0), (0, 0, 0))])
    g.set_pins([Pin(v, 0, x[v]) for v in (0, 19)])
    g.set_force_fields(fields)
    g.run_substeps(20, DT, -1)
    g.gpu_sync()
    assert g.stats()["error_flags"] == 0
    pinned = g.dump_cpu_state()[0][[0, 19]]
    assert np.abs(pinned - x[[0, 19]]).max() < 1e-5
    g.destroy()
    # grid bodies
    g = hs.engine(sheets, bodies=1)
    g.set_grid_bodies([GridBody(Collider(1, body=0, p_WB=(0.5, 0.5, 0.53), dims=(0.06, 0, 0)), mode=0)])
    g.set_force_fields(fields)
    g.run_substeps(20, DT, BC_BODIES)
    g.gpu_sync()
    assert g.stats()["error_flags"] == 0
    assert np.isfinite(g.download(hs.ARR().VELOCITIES)).all()
    g.destroy()
    # per-cloth materials, the batched path
    mat = GpuMpm.default_material()
    g = GpuMpm(6, mat)
    g.set_deterministic(True)
    for k, z in enumerate((0.6, 0.62)):
        cm = ClothMaterial.of(mat)
        cm.density = (2000.0, 300.0)[k]
        g.add_qr_cloth(*_flat_sheet(res=20, side=0.3, z=z)[0], material=cm)
    g.finalize()
    g.set_force_fields(fields)
    g.run_substeps(20, DT, -1)
    g.gpu_sync()
    assert g.stats()["error_flags"] == 0
    g.destroy()


def test_refusals():
    from drake_amd import FF_DRAG, FF_NORMAL_DRAG, Collider, ForceField, MpmError
    g = hs.engine(_flat_sheet(res=20, side=0.3, z=0.6), bodies=1)

    def refused(call, says=None):
        with pytest.raises(MpmError) as e:
            call()
        assert e.value.code == -1, e.value
        if says:
            assert says in str(e.value), e.value

    good = _c(ff.table("regions"))
    g.set_force_fields(good)
    got = g.get_force_fields()
    assert len(got) == len(good) and all(bytes(p) == bytes(q) for p, q in zip(got, good))
    # n = 9, and a bad entry: the table in force stays
    refused(lambda: g.set_force_fields([ForceField()] * 9))
    refused(lambda: g.set_force_fields([ForceField(kind=5)]))
    refused(lambda: g.set_force_fields([ForceField(FF_DRAG, gamma=-1.0)]))
    assert all(bytes(p) == bytes(q) for p, q in zip(g.get_force_fields(), good))
    # partitioned and halo calls on an engine with a table
    nb = 64 // 4
    refused(lambda: g.dist_init(0, 1, [0, nb], 2, 2, 2), says="force fields")
    refused(lambda: g.substep_mid_halo(DT), says="force fields")
    refused(lambda: g.team_prepare(), says="force fields")
    refused(lambda: g.chain_substeps(1, DT), says="force fields")
    # dt * sum of the linear gammas > 1: every substep entry point that takes a dt
    g.set_force_fields([ForceField(FF_DRAG, gamma=600.0), ForceField(FF_NORMAL_DRAG, gamma=600.0),
                        ForceField(FF_NORMAL_DRAG, gamma=1e6, quadratic=True)])
    before = g.stats()["substeps"]
    floor = [Collider(0, body=0, p_WB=(0.5, 0.5, 0.3))]
    for call in (lambda: g.run_substeps(2, DT, -1), lambda: g.substep(DT, -1), lambda: g.particle_to_grid(DT),
                 lambda: g.profile_substeps(2, DT, -1), lambda: g.run_coupled_substeps(2, DT, floor, 0.5, 1e5, 1e-4),
                 lambda: g.substep_begin(DT)):
        refused(call, says="gamma")
    assert g.stats()["substeps"] == before
    # at half the step the same table runs (quadratic fields are not part of the sum)
    g.set_force_fields([ForceField(FF_DRAG, gamma=600.0), ForceField(FF_NORMAL_DRAG, gamma=600.0)])
    refused(lambda: g.run_substeps(1, DT, -1), says="gamma")
    g.run_substeps(2, 0.5 * DT, -1)
    g.gpu_sync()
    assert g.stats()["error_flags"] == 0
    # a cleared table lifts the refusals
    g.set_force_fields([])
    g.run_substeps(1, DT, -1)
    g.dist_init(0, 1, [0, nb], 2, 2, 2)
    refused(lambda: g.set_force_fields(good), says="partitioned")
    assert g.get_force_fields() == []
    g.destroy()
