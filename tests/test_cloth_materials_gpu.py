"""Per-cloth materials (include/mpm_hip.h: mpm_add_qr_cloth_with_material) on the device: a multi-material engine whose
cloths all share one material against an engine created with it, to the bit, on every substep path; exact scaling of
forces, taus and masses between two sheets whose materials differ by a power of two; three materials against CPU oracles
that each hold one sheet; the contact momentum balance of two sheets of different density; refusals and getters."""

import numpy as np
import pytest

from tests.helpers import close, natural_scales
from tests import harness as hs

pytestmark = pytest.mark.gpu
DT = 1e-3
ERR_INVALID = -1
# different from mpm_default_material in every per-cloth field
M_FIELDS = dict(youngs_modulus=2.5e5, poisson_ratio=0.22, density=1300.0, gamma=40.0, K=2.0e5, c_F=15.0)


def _cm(**kw):
    from drake_amd import ClothMaterial
    return ClothMaterial(*[float(kw[f]) for f, _ in ClothMaterial._fields_])


def _sheets(layers=2, res=16, seed=7, vel_amp=0.2, **kw):
    from drake_amd import scenes
    return scenes.cloth_stack(layers, res, 6, z0=kw.pop("z0", 0.5), side=kw.pop("side", 0.3), seed=seed,
                              vel_amp=vel_amp, **kw)


def _engine(sheets, materials=None, engine_material=None, deterministic=True, fast_math=False, bodies=0):
    """materials: None (plain mpm_add_qr_cloth) or one ClothMaterial (or None: the engine's) per sheet"""
    from drake_amd import GpuMpm
    gm = None
    if engine_material:
        gm = GpuMpm.default_material()
        for k, v in engine_material.items():
            setattr(gm, k, v)
    g = GpuMpm(6, gm)
    g.set_deterministic(deterministic)
    g.set_fast_math(fast_math)
    for k, (pos, vel, idx) in enumerate(sheets):
        if materials is None:
            g.add_qr_cloth(pos, vel, idx)
        elif materials[k] is None:
            # (the new entry point with a NULL material: the engine's own)
            import ctypes as C
            from drake_amd.capi import _f32, _ptr
            p, v = _f32(pos, (-1, 3)), _f32(vel, (-1, 3))
            i = np.ascontiguousarray(idx, dtype=np.int32).reshape(-1)
            g._ck(g.lib.mpm_add_qr_cloth_with_material(g.h, _ptr(p), _ptr(v), p.shape[0], _ptr(i), i.size // 3,
                                                       C.c_void_p()))
        else:
            g.add_qr_cloth(pos, vel, idx, material=materials[k])
    g.finalize()
    if bodies:
        g.reallocate_external_bodies(bodies)
    return g


def _state(g, grid=True):
    A = hs.ARR()
    s = {k: g.download(getattr(A, k)) for k in ("POSITIONS", "VELOCITIES", "AFFINE", "DEFORMATION_GRADIENTS", "FORCES",
                                                 "TAUS", "MASSES", "PIDS")}
    if grid:
        s["GRID_MASSES"] = g.download(A.GRID_MASSES)
        s["GRID_MOMENTUM"] = g.download(A.GRID_MOMENTUM)
    if getattr(g, "_n_bodies", 0):
        s["tau"], s["f"] = g.external_body_force_to_host()
    return s


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.isfinite(a[k]).all() if a[k].dtype.kind == "f" else True, (what, k)
        assert np.array_equal(a[k], b[k]), (what, k, float(np.abs(a[k].astype(np.float64) - b[k]).max()))


# The fixed-point scales of deterministic ParticleToGrid come from the total mass, summed in double: as sum of
# |vol| * density in a single-material engine and as sum of the stored float masses in a multi-material one.  The two
# sums differ in their last bits, so the power of two derived from them could differ -- but only when the total mass lies
# within about 1e-7 (relative) of a power of two.  The scenes of these tests are checked to be far from that boundary.
def _far_from_power_of_two(g):
    m = float(np.sum(g.download(hs.ARR().MASSES).astype(np.float64)))
    r = np.log2(m)
    assert abs(r - np.round(r)) > 1e-4, m


def _run(g, path, n, colliders=None):
    if path == "phases":
        for _ in range(n):
            hs.phases(g, DT)
    elif path == "run_substeps":
        g.run_substeps(n, DT, -1)
    else:
        g.run_coupled_substeps(n, DT, colliders, 0.5, 1e5, 1e-4)
    g.gpu_sync()
    assert g.stats()["error_flags"] == 0


def _contact_colliders():
    from drake_amd import Collider
    # a sphere under the middle of the stack and a floor under it all (bodies 0 and 1)
    return [Collider(1, body=0, p_WB=(0.5, 0.5, 0.5 - 0.05 - 0.004), dims=(0.05, 0, 0)),
            Collider(0, body=1, p_WB=(0.5, 0.5, 0.44))]


@pytest.mark.parametrize("path", ["phases", "run_substeps", "coupled"])
@pytest.mark.parametrize("fast_math", [False, True])
def test_same_material_same_bits(path, fast_math):
    """deterministic mode: cloths added with material M through the new call against an engine created with M, 20
    substeps -- positions, velocities, C, F, vertex forces, taus, masses, grid mass and momentum and body impulses equal
    to the bit.  And cloths added through the new call with the engine's own material (M, and NULL) against a plain
    engine."""
    sheets = _sheets()
    for s in sheets:
        s[1][:, 2] -= 0.3   # (falling onto the colliders of the coupled path)
    M = _cm(**M_FIELDS)
    cols = _contact_colliders() if path == "coupled" else None
    bodies = 2 if path == "coupled" else 0
    ref = _engine(sheets, engine_material=M_FIELDS, fast_math=fast_math, bodies=bodies)
    multi = _engine(sheets, materials=[M, M], fast_math=fast_math, bodies=bodies)
    own = _engine(sheets, materials=[None, M], engine_material=M_FIELDS, fast_math=fast_math, bodies=bodies)
    _far_from_power_of_two(ref)
    for g in (ref, multi, own):
        _run(g, path, 20, cols)
    sr = _state(ref)
    if path == "coupled":
        assert np.abs(sr["f"]).max() > 0   # (the cloth did touch the colliders)
    _same(sr, _state(multi), f"{path} per-cloth M")
    _same(sr, _state(own), f"{path} engine's own material")


def test_same_material_same_bits_outside_deterministic_mode():
    """without deterministic mode ParticleToGrid's float sums depend on the order of arrival, so whole substeps are not
    reproducible run to run on any engine; CalcFemStateAndForce is (fixed summation order): after it the forces, taus,
    F and masses are equal to the bit, and one whole substep agrees to float rounding"""
    A = hs.ARR()
    sheets = _sheets()
    M = _cm(**M_FIELDS)
    for fast_math in (False, True):
        ref = _engine(sheets, engine_material=M_FIELDS, deterministic=False, fast_math=fast_math)
        multi = _engine(sheets, materials=[M, M], deterministic=False, fast_math=fast_math)
        for g in (ref, multi):
            g.rebuild_mapping(False)
            g.calc_fem_state_and_force(DT)
        _same(_state(ref, grid=False), _state(multi, grid=False), f"fem fast_math={fast_math}")
        for g in (ref, multi):
            g.particle_to_grid(DT)
            g.update_grid(-1)
            g.grid_to_particle(DT)
        a, b = ref.download(A.VELOCITIES), multi.download(A.VELOCITIES)
        close(b, a, scale=max(float(np.abs(a).max()), 1e-2), rtol=1e-5, what="vel, determinism off")


def _by_pid(g, arr):
    pid = g.download(hs.ARR().PIDS)
    out = np.empty_like(arr)
    out[pid] = arr
    return out


def _two_sheets_scaled():
    """sheet A with x in [0.52, 0.66] and B = A + 0.25 x: one binade per coordinate (translations are exact); 7 cells
    apart"""
    from drake_amd import scenes
    (pa, va, ia), = scenes.cloth_stack(1, 14, 6, z0=0.5, side=0.14, seed=11, vel_amp=0.1, center=(0.595, 0.5))
    pa = pa.astype(np.float32)
    assert pa[:, 0].min() >= 0.52 and pa[:, 0].max() <= 0.66, (pa[:, 0].min(), pa[:, 0].max())
    pb = pa.copy()
    pb[:, 0] += np.float32(0.25)
    assert np.array_equal(pb[:, 0] - np.float32(0.25), pa[:, 0])
    base = dict(youngs_modulus=3e5, poisson_ratio=0.3, density=1500.0, gamma=20.0, K=1e5, c_F=0.0)
    dbl = dict(base, youngs_modulus=6e5, density=3000.0, gamma=40.0, K=2e5)
    return [(pa, va, ia), (pb, va.copy(), ia)], _cm(**base), _cm(**dbl)


def _scaling_check(g, nfa, nva, what):
    A = hs.ARR()
    nf = g.n_faces
    f, tau, m = (_by_pid(g, g.download(a)) for a in (A.FORCES, A.TAUS, A.MASSES))
    ia = np.concatenate([np.arange(nfa), nf + np.arange(nva)])   # A's particle ids ...
    ib = np.concatenate([nfa + np.arange(nfa), nf + nva + np.arange(nva)])   # ... and B's
    assert np.abs(f[ia]).max() > 0 and np.abs(tau[ia]).max() > 0
    assert np.array_equal(f[ib], 2 * f[ia]), (what, "forces")
    assert np.array_equal(tau[ib], 2 * tau[ia]), (what, "taus")
    assert np.array_equal(m[ib], 2 * m[ia]), (what, "masses")


def test_exact_power_of_two_scaling():
    """B has E, K, gamma and rho doubled, the same nu, c_F = 0: after CalcFemStateAndForce its vertex forces, taus and
    masses are exactly twice A's; again after 30 substeps with re-sorts, with A's state uploaded into both sheets (the
    per-face lookup after the slots have been shuffled)"""
    A = hs.ARR()
    sheets, ma, mb = _two_sheets_scaled()
    nva, nfa = sheets[0][0].shape[0], sheets[0][2].size // 3
    g = _engine(sheets, materials=[ma, mb])
    g.rebuild_mapping(False)
    g.calc_fem_state_and_force(DT)
    _scaling_check(g, nfa, nva, "first")
    # MPM_ARR_VOLUMES still returns volumes: mass / rho within one float ulp, the same for both sheets
    nf = g.n_faces
    vol, mass = _by_pid(g, g.download(A.VOLUMES)), _by_pid(g, g.download(A.MASSES))
    ia = np.concatenate([np.arange(nfa), nf + np.arange(nva)])
    ib = np.concatenate([nfa + np.arange(nfa), nf + nva + np.arange(nva)])
    assert np.array_equal(vol[ib], vol[ia])
    assert np.all(np.abs(vol[ia] - mass[ia].astype(np.float64) / ma.density) <= np.spacing(vol[ia]))
    for k in range(30):
        hs.phases(g, DT)
        if k % 7 == 0:
            g.rebuild_mapping(True)   # (a slot sort as well: the API order moves too)
    g.gpu_sync()
    assert g.stats()["error_flags"] == 0
    assert g.stats()["rebuilds"] >= 1
    nf = g.n_faces
    pid = g.download(A.PIDS)
    st = {a: _by_pid(g, g.download(a)) for a in (A.POSITIONS, A.VELOCITIES, A.AFFINE, A.VOLUMES)}
    ia = np.concatenate([np.arange(nfa), nf + np.arange(nva)])
    ib = np.concatenate([nfa + np.arange(nfa), nf + nva + np.arange(nva)])
    new = {}
    for a, arr in st.items():
        arr = arr.copy()
        arr[ib] = arr[ia]
        if a == A.POSITIONS:
            arr[ib, 0] += np.float32(0.25)
            assert arr[:, 0].min() >= 0.5 and arr[:, 0].max() < 1.0
        new[a] = arr[pid]   # (back to slot order)
    F = g.download(A.DEFORMATION_GRADIENTS)
    F[nfa:] = F[:nfa]
    g.upload_particle_state(pos=new[A.POSITIONS], vel=new[A.VELOCITIES], affine=new[A.AFFINE], volumes=new[A.VOLUMES],
                            deformation_gradients=F)
    g.rebuild_mapping(False)
    g.calc_fem_state_and_force(DT)
    g.gpu_sync()
    _scaling_check(g, nfa, nva, "after upload")


def test_three_materials_against_single_sheet_oracles():
    """three sheets at least 8 cells apart, each with its own E, nu, rho, gamma, K and c_F: after 1 and after 20 substeps
    every sheet matches a CPU oracle that holds only that sheet, with that material"""
    from oracle import oracle as orc
    from tests.helpers import _MATERIAL_FIELDS
    A = hs.ARR()
    mats = [dict(youngs_modulus=2e5, poisson_ratio=0.25, density=800.0, gamma=0.0, K=1e5, c_F=0.0),
            dict(youngs_modulus=6e5, poisson_ratio=0.35, density=2500.0, gamma=50.0, K=3e5, c_F=20.0),
            dict(youngs_modulus=1e6, poisson_ratio=0.1, density=4000.0, gamma=10.0, K=5e4, c_F=5.0)]
    from drake_amd import scenes
    sheets = []
    for k, cx in enumerate((0.2, 0.5, 0.8)):
        sheets += scenes.cloth_stack(1, 12, 6, z0=0.5, side=0.14, seed=20 + k, vel_amp=0.2, center=(cx, 0.5))
    g = _engine(sheets, materials=[_cm(**m) for m in mats], deterministic=False)
    oracles = []
    for (pos, vel, idx), m in zip(sheets, mats):
        o = orc.OracleMpm(6)
        for k, v in m.items():
            setattr(o.p, _MATERIAL_FIELDS[k], v)
        o.add_qr_cloth(pos, vel, idx)
        o.finalize()
        oracles.append(o)
    info = [g.cloth_info(c) for c in range(3)]
    nf = g.n_faces
    for n_done, n in ((0, 1), (1, 20)):
        scs = [natural_scales(o, DT) for o in oracles]
        for _ in range(n - n_done):
            hs.phases(g, DT)
            for o in oracles:
                o.substep(DT, -1)
        g.gpu_sync()
        assert g.stats()["error_flags"] == 0
        st = {a: _by_pid(g, g.download(a)) for a in (A.POSITIONS, A.VELOCITIES, A.MASSES, A.VOLUMES)}
        xs = []
        for c, (o, sc, inf, m) in enumerate(zip(oracles, scs, info, mats)):
            ids = np.concatenate([inf["first_face"] + np.arange(inf["n_faces"]),
                                  nf + inf["first_vertex"] + np.arange(inf["n_verts"])])
            so = o.state_in_original_order()
            close(st[A.POSITIONS][ids], so["pos"], scale=1.0, rtol=1e-5, what=f"sheet {c} pos after {n}")
            close(st[A.VELOCITIES][ids], so["vel"], scale=sc["vel"], rtol=3e-4 if n > 1 else 1e-5,
                  what=f"sheet {c} vel after {n}")
            close(st[A.VOLUMES][ids], so["vol"], what=f"sheet {c} vol after {n}")
            close(st[A.MASSES][ids], so["vol"] * m["density"], what=f"sheet {c} mass after {n}")
            xs.append(st[A.POSITIONS][ids][:, 0])
        for c in range(2):   # (still 8 cells apart)
            assert xs[c + 1].min() - xs[c].max() >= 8 / 64


def _balance(g, boxes, ids, faces, dt, n_settle, n_win):
    """coupled substeps: settle, then a window of n_win; -> per sheet (impulse on its body over the window,
    m g T - (p(T) - p(0)) + sum of d, mass)"""
    A = hs.ARR()
    corners = g.download(A.INDICES).reshape(-1, 3)
    g.run_coupled_substeps(n_settle, dt, boxes, 0.5, 1e5, 1e-4)

    def state():
        v = _by_pid(g, g.download(A.VELOCITIES)).astype(np.float64)
        m = _by_pid(g, g.download(A.MASSES)).astype(np.float64)
        p = [(m[i, None] * v[i]).sum(axis=0) for i in ids]
        d = [(m[f, None] * (v[corners[f]].mean(axis=1) - v[f])).sum(axis=0) for f in faces]
        return p, d, [float(m[i].sum()) for i in ids]

    p0, _, mass = state()
    _, f0 = g.external_body_force_to_host()
    d_sum = [np.zeros(3) for _ in ids]
    for _ in range(n_win):
        _, d, _ = state()
        for c in range(len(ids)):
            d_sum[c] += d[c]
        g.run_coupled_substeps(1, dt, boxes, 0.5, 1e5, 1e-4)
    g.gpu_sync()
    assert g.stats()["error_flags"] == 0
    p1, _, _ = state()
    _, f1 = g.external_body_force_to_host()
    T = n_win * float(np.float32(dt))
    gvec = np.array([0.0, 0.0, -9.8])
    return [((f1[b] - f0[b]).astype(np.float64), mass[c] * gvec * T - (p1[c] - p0[c]) + d_sum[c], mass[c])
            for c, b in enumerate(sorted({int(x.body) for x in boxes}))]


def test_contact_momentum_balance_two_densities():
    """two sheets of density rho and 3 rho, each resting on its own box (bodies 0 and 1, mpm_bc = -1, coupled
    substeps).  Over the last window T, with m_c = sum of rho_c vol and p_c from the downloaded velocities and
    MPM_ARR_MASSES, the impulse on body c is compared with m_c g T - (p_c(T) - p_c(0)) + sum of d: d is the momentum
    CalcFemStateAndForce adds each substep by putting every face particle's velocity at the mean of its corners'
    (tests/pin_reference.py: face_recentring).
    The contact impulse is the sum over contact points of m (v_after - v_before) of the contact solve, which is not
    exactly the momentum the grid nodes receive: on this scene the balance closes to about 6 % in a single-material
    engine too.  So each sheet's impulse and balance are held to 1 % of m_c g T against a single-material engine of
    density rho_c that holds that sheet and its box alone, and the balance itself to 10 %."""
    from drake_amd import Collider, scenes
    dt, n_settle, n_win = 5e-4, 150, 100
    rho = 1000.0
    base = dict(youngs_modulus=4e5, poisson_ratio=0.3, gamma=0.0, K=1e5, c_F=0.0)
    sheets, boxes = [], []
    for c, cx in enumerate((0.3, 0.7)):
        sheets += scenes.cloth_stack(1, 14, 6, z0=0.5, side=0.16, seed=30 + c, vel_amp=0.0, center=(cx, 0.5))
        boxes.append(Collider(2, body=c, p_WB=(cx, 0.5, 0.5 - 0.004 - 0.1), dims=(0.12, 0.12, 0.1)))
    dens = (rho, 3 * rho)
    g = _engine(sheets, materials=[_cm(density=d, **base) for d in dens], bodies=2)
    nf = g.n_faces
    info = [g.cloth_info(c) for c in range(2)]
    faces = [i["first_face"] + np.arange(i["n_faces"]) for i in info]
    ids = [np.concatenate([f, nf + i["first_vertex"] + np.arange(i["n_verts"])]) for f, i in zip(faces, info)]
    vols = _by_pid(g, g.download(hs.ARR().VOLUMES)).astype(np.float64)
    multi = _balance(g, boxes, ids, faces, dt, n_settle, n_win)
    T = n_win * float(np.float32(dt))
    for c in range(2):
        m_c = float(vols[ids[c]].sum()) * dens[c]
        got, want, mass = multi[c]
        assert abs(m_c - mass) <= 1e-5 * m_c
        tol = 0.01 * m_c * 9.8 * T
        assert -got[2] > 0.5 * m_c * 9.8 * T   # (the box does carry the sheet)
        assert np.abs(got - want).max() <= 10 * tol, (c, got, want)
        single = _engine([sheets[c]], engine_material=dict(base, density=dens[c]), bodies=2)
        nf1 = single.n_faces
        f1 = np.arange(nf1)
        s_got, s_want, s_mass = _balance(single, [boxes[c]], [np.concatenate([f1, nf1 + np.arange(single.n_verts)])],
                                         [f1], dt, n_settle, n_win)[0]
        assert abs(s_mass - mass) <= 1e-5 * m_c
        assert np.abs(got - s_got).max() <= tol, (c, got, s_got)
        assert np.abs((got - want) - (s_got - s_want)).max() <= tol, (c, got - want, s_got - s_want)
    assert multi[1][2] > 2.9 * multi[0][2]


def test_refusals_and_getters():
    from drake_amd import GpuMpm, MpmError, scenes

    def refused(fn, says=None):
        with pytest.raises(MpmError) as e:
            fn()
        assert e.value.code == ERR_INVALID
        if says is not None:
            assert says in str(e.value), str(e.value)
        return str(e.value)

    sheets = scenes.cloth_stack(2, 10, 6, z0=0.5, side=0.2, seed=1, vel_amp=0.1)
    good = dict(M_FIELDS)
    h = GpuMpm(6)
    pos, vel, idx = sheets[0]
    bad = [dict(good, youngs_modulus=0.0), dict(good, youngs_modulus=-1.0), dict(good, poisson_ratio=0.5),
           dict(good, poisson_ratio=-0.01), dict(good, density=0.0), dict(good, gamma=-1.0), dict(good, K=-1.0),
           dict(good, c_F=-1.0)]
    for f in good:
        bad += [dict(good, **{f: np.nan}), dict(good, **{f: np.inf})]
    for b in bad:
        refused(lambda: h.add_qr_cloth(pos, vel, idx, material=_cm(**b)))
    assert h.cloth_count() == 0
    h.add_qr_cloth(pos, vel, idx)
    h.add_qr_cloth(*sheets[1], material=_cm(**good))
    assert h.cloth_count() == 2
    i0, i1 = h.cloth_info(0), h.cloth_info(1)
    nv0, nf0 = pos.shape[0], idx.size // 3
    assert (i0["first_vertex"], i0["n_verts"], i0["first_face"], i0["n_faces"]) == (0, nv0, 0, nf0)
    assert (i1["first_vertex"], i1["n_verts"], i1["first_face"], i1["n_faces"]) == (nv0, sheets[1][0].shape[0], nf0,
                                                                                       sheets[1][2].size // 3)
    d = GpuMpm.default_material()
    assert i0["material"].as_dict() == {f: float(np.float32(getattr(d, f))) for f in good}
    assert i1["material"].as_dict() == {f: float(np.float32(v)) for f, v in good.items()}
    refused(lambda: h.cloth_info(2))
    h.finalize()
    refused(lambda: h.add_qr_cloth(pos, vel, idx, material=_cm(**good)))
    refused(lambda: h.add_qr_cloth(pos, vel, idx))
    assert h.cloth_count() == 2
    # partitioned and multi-rank calls on a multi-material engine: refused as such, before any prerequisite is looked at
    # (most of these calls fail on a plain engine too, for a missing mpm_dist_init / mpm_chain_init / begin_halo: the
    # message tells the two refusals apart)
    from drake_amd import Collider
    nb = 64 // 4
    calls = dict(
        dist_init=lambda g: g.dist_init(0, 1, [0, nb], 2, 2, 2),
        chain_init=lambda g: g.chain_init(None, 0, 1, 0, nb, 0, 2, 64),
        chain_direct_prepare=lambda g: g.chain_direct_prepare(),
        chain_enable_migration=lambda g: g.chain_enable_migration(4, 1024),
        chain_substeps=lambda g: g.chain_substeps(1, DT),
        team_prepare=lambda g: g.team_prepare(),
        world_coupled_substeps=lambda g: GpuMpm.world_coupled_substeps(
            [g], 1, DT, [Collider(0, body=0, p_WB=(0.5, 0.5, 0.1))], 0.5, 1e5, 1e-4),
        substep_mid_halo=lambda g: g.substep_mid_halo(DT),
    )
    plain = GpuMpm(6)
    plain.add_qr_cloth(pos, vel, idx)
    plain.finalize()
    plain.reallocate_external_bodies(1)
    h.reallocate_external_bodies(1)
    for name, call in calls.items():
        refused(lambda: call(h), says="multi-material engine")
        if name not in ("dist_init", "chain_init"):   # (these two succeed on a plain engine)
            assert "multi-material" not in refused(lambda: call(plain)), name
    plain.destroy()
    h.destroy()
    # the 257th cloth
    tiny = (np.array([[0.5, 0.5, 0.5], [0.51, 0.5, 0.5], [0.5, 0.51, 0.5]], np.float32), np.zeros((3, 3), np.float32),
            np.array([0, 1, 2], np.int32))
    t = GpuMpm(6)
    for _ in range(256):
        t.add_qr_cloth(*tiny, material=_cm(**good))
    refused(lambda: t.add_qr_cloth(*tiny, material=_cm(**good)))
    refused(lambda: t.add_qr_cloth(*tiny))
    assert t.cloth_count() == 256
    t.destroy()
    # refused calls leave nothing behind: the engine finalizes and runs as one that never saw them
    a = GpuMpm(6)
    b = GpuMpm(6)
    for g in (a, b):
        g.set_deterministic(True)
    for k, s in enumerate(sheets):
        refused(lambda: a.add_qr_cloth(*s, material=_cm(**dict(good, density=-5.0))))
        a.add_qr_cloth(*s, material=_cm(**good))
        b.add_qr_cloth(*s, material=_cm(**good))
    for g in (a, b):
        g.finalize()
        for _ in range(5):
            hs.phases(g, DT)
        g.gpu_sync()
    _same(_state(a), _state(b), "after refusals")
