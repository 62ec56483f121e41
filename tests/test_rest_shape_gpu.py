"""Rest shape apart from the pose (mpm_set_rest_shape; k_rest_faces, k_rest_vertices) on the engine, 64^3 grid.  The cases,
their float64 rest states and the sheets are tests/rest_shape.py's; the bounds are tests/rest_meshes.py's, unchanged.

1. Twin finalized on R.  Engine B is added at the pose P and given set_rest_shape(R), engine A is added at R: Dm^-1, the face
   and vertex volumes and the masses are the same bits by original id -- one material or one per cloth, 1 to 40 faces
   around a vertex, and again when the call comes after substeps and a sort that moved every slot.  B's arrays also lie
   within rest_meshes' bounds of float64; its positions, velocities, F, C and particle order are what they were.  The two
   exact kinds need no twin: twice Dm^-1 and a quarter of the volumes of an untouched engine (double), its very bits (shift).
2. Same dynamics.  A gets B's positions, velocities and F: then x, v, C, F and the vertex forces are the same bits by
   original id after one CalcFemStateAndForce, whatever the particle order, and after the 48 substeps of every runner
   of tests/substep_paths.py in deterministic mode.  EVERY path's trajectory depends on the particle order inside a
   cell in its last bits (k_p2g adds a 64-particle group in float ahead of the fixed-point tile; the coupled path also
   sums its contact rows in slot order): with the orders Finalize gave the twins -- A sorted at R, B at P -- 185 of the
   1158 position words differed after 48 substeps on each path.  So the twins are first given one particle order, by a
   re-sort of a state with one particle per cell (tests/rest_shape.py: spread); the scene keeps its 5 % stretch and
   0.08 shear.
3. Off means off.  4. Features set afterwards follow the rest shape.  5. Refusals.  6. Physics."""
import functools

import numpy as np
import pytest

from tests import harness as hs
from tests import rest_meshes as rm
from tests import rest_shape as rs
from tests import substep_paths as sp

pytestmark = pytest.mark.gpu

CQ, CD, CV = (rm.ENGINE_FACTOR * c for c in (rm.ORACLE_CQ, rm.ORACLE_CD, rm.ORACLE_CV))
REST_FIELDS = ("Dm", "vol", "mass")
_CACHE = {}


_engine = functools.partial(hs.engine, bits=rs.BITS, deterministic=None)


def _same(a, b, fields, what=""):
    for f in fields:
        assert a[f].dtype == b[f].dtype and a[f].shape == b[f].shape, (what, f)
        bad = np.flatnonzero(np.any((hs.bits(a[f]) != hs.bits(b[f])).reshape(len(a[f]), -1), axis=1))
        assert bad.size == 0, (what, f, int(bad.size), bad[:8])


def _state_by_id(g):
    """x, v, C by original id, F by face, the slot order"""
    A = hs.ARR()
    return dict(x=hs.by_id(g, A.POSITIONS), v=hs.by_id(g, A.VELOCITIES), C=hs.by_id(g, A.AFFINE), F=g.download(A.DEFORMATION_GRADIENTS),
                pids=g.download(A.PIDS))


def _cloths(case, which):
    k = 0 if which == "rest" else 1
    if case["parts"] is not None:
        return [p[k].sheet() for p in case["parts"]]
    return [case[which].sheet()]


def refused(call, says=None):
    from drake_amd import MpmError
    with pytest.raises(MpmError) as e:
        call()
    assert e.value.code == -1, e.value
    if says:
        assert says in str(e.value), e.value


def _untouched(name):
    """the rest state of an untouched engine at the mesh `name` of rest_meshes (made once, left unchanged)"""
    if name not in _CACHE:
        g = _engine(_cloths(rs.case(name, "shift"), "pose"))
        _CACHE[name] = rm.of_engine(g, masses=True)
        g.destroy()
    return _CACHE[name]


# ---- 1 -------------------------------------------------------------------------------------------------------------------
def _twin(name, kind, multi, moved=False):
    """-> (a, b, before, after): the rest states of A and B by original id, B's state before and after the call"""
    c = rs.case(name, kind)
    n_cloths = len(c["parts"]) if c["parts"] is not None else 1
    mats = [dict(density=d) for d in rs.DENSITIES[:n_cloths]] if multi else None
    A = _engine(_cloths(c, "rest"), mats=mats)
    B = _engine(_cloths(c, "pose"), mats=mats, env={"MPM_RESORT_EVERY": "1", "MPM_QUIET_FACTOR": "0"} if moved else None)
    if moved:
        # five cells along x, a dozen substeps with their re-sort, then the full sort: every slot has moved
        pid0, before_rebuilds = B.download(hs.ARR().PIDS), B.stats()["rebuilds"]
        hs.upload(B, c["pose"].pos + np.array([5.0 / 64, 0.0, 0.0], np.float32), np.array([3.0, 0.5, 0.0], np.float32))
        B.run_substeps(12, 1e-4, -1)
        B.gpu_sync()
        B.rebuild_mapping(True)
        assert B.stats()["rebuilds"] > before_rebuilds and not np.array_equal(B.download(hs.ARR().PIDS), pid0), "no slot moved"
    before = _state_by_id(B)
    assert B.get_rest_shape()[1] is False and np.array_equal(B.get_rest_shape()[0], c["pose"].pos)
    B.set_rest_shape(c["rest"].pos)
    got, is_set = B.get_rest_shape()
    assert is_set and np.array_equal(hs.bits(got), hs.bits(c["rest"].pos))
    after = _state_by_id(B)
    a, b = rm.of_engine(A, masses=True), rm.of_engine(B, masses=True)
    for g in (A, B):
        assert g.stats()["error_flags"] == 0, g.stats()
        g.destroy()
    return a, b, before, after


@pytest.mark.parametrize("multi", [False, True], ids=["one_material", "materials"])
@pytest.mark.parametrize("name,kind", rs.CASES)
def test_twin_finalized_on_the_rest_shape(name, kind, multi):
    c = rs.case(name, kind)
    a, b, before, after = _twin(name, kind, multi)
    _same(a, b, REST_FIELDS, (name, kind, multi))
    # what the call leaves alone
    for k in before:
        assert np.array_equal(hs.bits(before[k]), hs.bits(after[k])), (name, kind, k)
    assert np.array_equal(b["pos"][c["rest"].nf:], c["pose"].pos)
    # ... and against float64, under rest_meshes' bounds (F0 is the twin's: B's F stays the pose's)
    if not multi:
        got = dict(F0=a["F0"], Dm=b["Dm"], pos=a["pos"], vel=a["vel"], vol=b["vol"])
        ratios = rm.bound_ratios(got, c["ref"], CQ, CD, CV)
        for field in ("Dm", "volf", "volv"):
            r = ratios[field]
            i = int(np.argmax(r)) if r.size else 0
            print(f"rest shape {name} {kind} {field}: worst error / allowed {float(r[i]) if r.size else 0.0:.3f} at {i}")
            assert r.size == 0 or r[i] <= 1.0, (name, kind, field, i, float(r[i]))
        assert np.array_equal(b["mass"], b["vol"] * np.float32(rm.DENSITY))
    else:
        # k_init_masses' rounding: the float32 product of the single-material volume and the cloth's density
        parts = c["parts"] if c["parts"] is not None else [(c["rest"], c["pose"])]
        rho = np.concatenate([np.full(r.nf, d, np.float32) for (r, _), d in zip(parts, rs.DENSITIES)] +
                             [np.full(r.nv, d, np.float32) for (r, _), d in zip(parts, rs.DENSITIES)])
        one = _twin(name, kind, False)[1]
        expect = one["vol"] * rho
        bad = np.flatnonzero(hs.bits(b["mass"]) != hs.bits(expect))
        assert bad.size == 0, (name, kind, bad[:8])
        _same(one, b, ("Dm",), (name, kind, "Dm of one material"))


@pytest.mark.parametrize("multi", [False, True], ids=["one_material", "materials"])
def test_twin_after_substeps_that_moved_every_slot(multi):
    a, b, before, after = _twin("valence", "scale", multi, moved=True)
    _same(a, b, REST_FIELDS, ("valence", "scale", multi, "moved"))
    for k in before:
        assert np.array_equal(hs.bits(before[k]), hs.bits(after[k])), k
    assert not np.array_equal(before["x"][rs.case("valence", "scale")["rest"].nf:], rs.case("valence", "scale")["pose"].pos)


@pytest.mark.parametrize("name", ["valence", "slivers", "scales"])
def test_exact_kinds_against_an_untouched_engine(name):
    """double: the rest shape is the pose halved, so Dm^-1 doubles and the volumes and masses quarter, to the bit;
    shift: the rest shape is the pose moved by -1/16 exactly, so nothing changes, to the bit"""
    u = _untouched(name)
    for kind in ("double", "shift"):
        c = rs.case(name, kind)
        B = _engine(_cloths(c, "pose"))
        B.set_rest_shape(c["rest"].pos)
        b = rm.of_engine(B, masses=True)
        assert B.stats()["error_flags"] == 0
        B.destroy()
        s_dm, s_vol = (np.float32(2.0), np.float32(0.25)) if kind == "double" else (np.float32(1.0), np.float32(1.0))
        want = dict(Dm=u["Dm"] * s_dm, vol=u["vol"] * s_vol, mass=u["mass"] * s_vol)
        _same(want, b, REST_FIELDS, (name, kind))
        _same(u, b, ("F0", "pos", "vel"), (name, kind))


# ---- 2 -------------------------------------------------------------------------------------------------------------------
def _dyn_sheets():
    """(rest, pose, vel, idx) of the dynamics twins: a jittered 12 x 12 sheet, its pose stretched by 5 % and sheared by
    0.08, moving sideways at 2 m/s"""
    from drake_amd import scenes
    rest, idx = rs.sheet(side=0.2, z=0.5, jitter=0.05)
    x = rs.scaled(rest, 1.05).astype(np.float64)
    x[:, 0] += 0.08 * (x[:, 1] - 0.5)
    pose = x.astype(np.float32)
    vel = np.float32(0.2) * np.stack([scenes.hash_uniform(5, len(rest), 3 + c) for c in range(3)], -1)
    vel[:, 0] += np.float32(2.0)
    return rest, pose, vel.astype(np.float32), idx


def _dyn_twins(env=None, same_order=True):
    """A added at the rest shape, B at the pose with set_rest_shape, both holding B's positions, velocities and F.
    same_order: both are first taken through tests/rest_shape.py's spread state, one particle per cell, whose re-sort
    leaves them in ONE particle order (Finalize sorted A by the rest shape's cells and B by the pose's).  Every substep
    path needs that: k_p2g adds the particles of a 64-particle group in float before the sum reaches the fixed-point tile,
    so a trajectory's last bits follow the order inside a cell (tests/test_parity_gpu.py says the same of two runs that
    re-sort at different substeps), and the coupled path generates and sums its contact rows in slot order."""
    rest, pose, vel, idx = _dyn_sheets()
    A = _engine([(rest, vel, idx)], deterministic=True, env=env)
    B = _engine([(pose, vel, idx)], deterministic=True, env=env)
    B.set_rest_shape(rest)
    _same(rm.of_engine(A, masses=True), rm.of_engine(B, masses=True), REST_FIELDS, "dynamics twins")
    sb = _state_by_id(B)
    assert B.n_faces == 242
    if same_order:
        wide = rs.spread(idx)
        assert rs.one_per_cell(wide, idx)
        for g in (A, B):
            before = g.stats()["rebuilds"]
            hs.upload(g, wide)
            g.rebuild_mapping(True)
            assert g.stats()["rebuilds"] > before
        assert np.array_equal(A.download(hs.ARR().PIDS), B.download(hs.ARR().PIDS))
    for g in (A, B):            # (B too: both then owe the same re-sort)
        pids = g.download(hs.ARR().PIDS)
        g.upload_particle_state(sb["x"][pids], sb["v"][pids], np.zeros((len(pids), 9), np.float32), None, sb["F"])
    return A, B


def _fresh_forces(g):
    g.rebuild_mapping(False)
    g.calc_fem_state_and_force(sp.DT)
    return hs.by_id(g, hs.ARR().FORCES)


def _compare(A, B, what):
    sa, sb = _state_by_id(A), _state_by_id(B)
    for k in ("x", "v", "C", "F"):
        bad = int((hs.bits(sa[k]) != hs.bits(sb[k])).sum())
        assert bad == 0, (what, k, bad)
    fa, fb = _fresh_forces(A), _fresh_forces(B)
    assert np.array_equal(hs.bits(fa), hs.bits(fb)), (what, "forces")
    _same(dict(F=A.download(hs.ARR().DEFORMATION_GRADIENTS)), dict(F=B.download(hs.ARR().DEFORMATION_GRADIENTS)), ("F",), what)
    return sa, fa


def test_same_forces_after_one_fem_pass():
    """(a face's F and its corner records, and a vertex's sum over them in ascending face id, do not depend on the
    particle order: here the twins keep the orders Finalize gave them)"""
    A, B = _dyn_twins(same_order=False)
    x0 = _state_by_id(B)["x"]
    sa, fa = _compare(A, B, "one CalcFemStateAndForce")
    nf = B.n_faces
    assert np.abs(fa[nf:]).max() > 0 and not fa[:nf].any()
    # the pre-strain is in the forces: the sheet pulls inwards, towards its centre, at its boundary
    bnd = rs.boundary()
    inward = -(x0[nf:][bnd, :2] - x0[nf:][:, :2].mean(axis=0))
    pull = np.sign(np.einsum("ij,ij->i", fa[nf:][bnd, :2].astype(np.float64), inward.astype(np.float64)))
    assert pull[0] != 0 and (pull == pull[0]).all()
    for g in (A, B):
        assert g.stats()["error_flags"] == 0
        g.destroy()


@pytest.mark.parametrize("name", list(sp.PATHS))
def test_same_dynamics_on_every_substep_path(name):
    family, runner, kw = sp.PATHS[name]
    env = {"MPM_DEFER_PHASES": "0"} if kw.get("defer_phases") is False else None
    A, B = _dyn_twins(env=env)
    x0 = _state_by_id(B)["x"]
    for g in (A, B):
        runner(g)
        g.gpu_sync()
    sa, _ = _compare(A, B, name)
    for g in (A, B):
        st = g.stats()
        assert st["error_flags"] == 0 and st["substeps"] == sp.N and st["rebuilds"] > 1, (name, st)
    assert np.abs(sa["x"] - x0).max() > 2.0 * sp.N * sp.DT * 0.9 and np.all(np.isfinite(sa["x"])) and sa["C"].any()
    for g in (A, B):
        g.destroy()


# ---- 3 -------------------------------------------------------------------------------------------------------------------
EVERY_ARRAY = ("POSITIONS", "VELOCITIES", "VOLUMES", "MASSES", "AFFINE", "PIDS", "INDEX_MAPPINGS", "SORT_KEYS", "FORCES",
               "DEFORMATION_GRADIENTS", "DM_INVERSES", "INDICES")


def _everything(g):
    A = hs.ARR()
    return {k: g.download(getattr(A, k)) for k in EVERY_ARRAY}


@pytest.mark.parametrize("multi", [False, True], ids=["one_material", "materials"])
def test_off_means_off(multi):
    """never called == called with the positions as added == a real rest shape and then NULL: every downloadable array,
    then a 20-substep trajectory through a re-sort and the launch counters, to the bit"""
    rest, pose, vel, idx = _dyn_sheets()
    vel = vel + np.array([2.0, 0.3, 0.0], np.float32)          # (4 m/s: a cell in 8 substeps of 5e-4 s)
    mats = [dict(density=rs.DENSITIES[0])] if multi else None
    es = [_engine([(pose, vel, idx)], mats=mats, deterministic=True) for _ in range(3)]
    es[1].set_rest_shape(pose)
    es[2].set_rest_shape(rest)
    assert not np.array_equal(es[2].download(hs.ARR().DM_INVERSES), es[0].download(hs.ARR().DM_INVERSES))
    es[2].set_rest_shape(None)
    assert [g.get_rest_shape()[1] for g in es] == [False, True, False]
    for g in es:
        assert np.array_equal(g.get_rest_shape()[0], pose)
    before = es[0].stats()["rebuilds"]
    first = [_everything(g) for g in es]          # (the last call before the substeps is the same on all three)
    for g in es:
        for _ in range(2):
            g.run_substeps(10, sp.DT, -1)
        g.gpu_sync()
        assert g.stats()["error_flags"] == 0
    assert es[0].stats()["rebuilds"] - before >= 1, es[0].stats()
    last = [_everything(g) for g in es]
    for k in (1, 2):
        for when in (first, last):
            for key in EVERY_ARRAY:
                assert np.array_equal(when[0][key].view(np.uint32), when[k][key].view(np.uint32)), (k, key)
        for key in ("substeps", "rebuilds", "resort_checks"):
            assert es[0].stats()[key] == es[k].stats()[key], (k, key)
    assert not np.array_equal(first[0]["POSITIONS"], last[0]["POSITIONS"])
    for g in es:
        g.destroy()


# ---- 4 -------------------------------------------------------------------------------------------------------------------
def test_bending_set_afterwards_is_the_twins():
    rest, pose, vel, idx = _dyn_sheets()
    A, B = _engine([(rest, None, idx)]), _engine([(pose, None, idx)])
    B.set_rest_shape(rest)
    bump = pose.copy()
    bump[:, 2] += np.float32(0.01) * np.sin(40.0 * pose[:, 0]).astype(np.float32) * np.cos(31.0 * pose[:, 1]).astype(np.float32)
    out = []
    for g in (A, B):
        g.set_bending([1e-4])
        hs.upload(g, bump)
        out.append((g.bending_forces(), g.bending_max_stable_dt()))
    assert np.array_equal(hs.bits(out[0][0]), hs.bits(out[1][0])) and out[0][1] == out[1][1] and np.isfinite(out[0][1])
    assert np.abs(out[0][0]).max() > 0
    # an engine at the pose without the call has other weights (the pose is sheared: other cotangents)
    Cg = _engine([(pose, None, idx)])
    Cg.set_bending([1e-4])
    hs.upload(Cg, bump)
    assert not np.array_equal(Cg.bending_forces(), out[0][0])
    for g in (A, B, Cg):
        assert g.stats()["error_flags"] == 0
        g.destroy()


def test_weave_axes_are_the_rest_shapes():
    from drake_amd import weave, weave_face_axes
    rest, pose, vel, idx = _dyn_sheets()
    B = _engine([(pose, None, idx)])
    B.set_rest_shape(rest)
    d = (1.0, 0.3, 0.1)
    B.set_weave([weave(E_warp=2e5, E_weft=1e5, nu=0.1, G=5e4, warp_dir=d)])
    got = B.weave_axes()
    want, bad = weave_face_axes(rest[idx], d)
    assert bad == -1 and np.array_equal(hs.bits(got), hs.bits(want))
    assert not np.array_equal(got, weave_face_axes(pose[idx], d)[0])
    # ... and the limit was formed from the rest shape's Dm^-1, volumes and masses: the twin's
    A = _engine([(rest, None, idx)])
    A.set_weave([weave(E_warp=2e5, E_weft=1e5, nu=0.1, G=5e4, warp_dir=d)])
    assert A.weave_max_stable_dt() == B.weave_max_stable_dt() and np.array_equal(hs.bits(A.weave_axes()), hs.bits(got))
    for g in (A, B):
        g.destroy()


def test_shell_bending_defaults_to_the_rest_shape():
    flat, idx = rs.sheet(side=0.2, z=0.55)
    rest = rs.arc(flat, 0.15)
    B = _engine([(flat, None, idx)])
    B.set_rest_shape(rest)
    B.set_shell_bending([1e-4])
    assert np.abs(B.shell_hinges()[2]).max() > 0.01          # psibar: the arc's hinge angles (0.09 rad across an edge)
    hs.upload(B, rest)
    assert not B.shell_forces().any()
    hs.upload(B, flat)
    assert np.abs(B.shell_forces()).max() > 0
    # without the call the default is the pose: zeros on the flat sheet
    Cg = _engine([(flat, None, idx)])
    Cg.set_shell_bending([1e-4])
    assert not Cg.shell_forces().any() and np.abs(Cg.shell_hinges()[2]).max() < 1e-6
    for g in (B, Cg):
        assert g.stats()["error_flags"] == 0
        g.destroy()


def test_gas_pressure_checks_the_winding_on_the_rest_shape():
    from drake_amd import PRESSURE_DTYPE, PRESSURE_GAS
    X, T = rs.octahedron()
    mirror = X.copy()
    mirror[:, 0] = np.float32(1.0) - X[:, 0]
    gas = np.zeros(1, PRESSURE_DTYPE)
    gas["mode"], gas["pv"], gas["p_ambient"], gas["p_max"] = PRESSURE_GAS, 1.0, 0.0, 1e4
    g = _engine([(X, None, T)])
    g.set_pressure(gas)
    g.set_pressure([])
    g.set_rest_shape(mirror)                                    # the pose is wound outwards, the rest shape inwards
    refused(lambda: g.set_pressure(gas), says="rest volume is not positive")
    g.set_rest_shape(None)
    g.set_pressure(gas)
    g.destroy()
    g = _engine([(mirror, None, T)])                            # and the other way round
    refused(lambda: g.set_pressure(gas), says="rest volume is not positive")
    g.set_rest_shape(X)
    g.set_pressure(gas)
    assert g.stats()["error_flags"] == 0
    g.destroy()


# ---- 5 -------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from drake_amd import PRESSURE_CONSTANT, PRESSURE_DTYPE, Anchor, GpuMpm, Pin, links, weave
    rest, pose, vel, idx = _dyn_sheets()
    g0 = GpuMpm(rs.BITS)
    g0.add_qr_cloth(pose, np.zeros_like(pose), idx)
    refused(lambda: g0.set_rest_shape(rest), says="finalize")
    refused(lambda: g0.get_rest_shape(), says="finalize")
    g0.destroy()

    g = _engine([(pose, None, idx)])
    g.reallocate_external_bodies(1)
    other = rs.scaled(rest, 0.9)
    g.set_rest_shape(other)                                     # the rest state in force is not Finalize's
    held = rm.of_engine(g, masses=True)

    def unchanged(what):
        _same(held, rm.of_engine(g, masses=True), ("F0", "Dm", "pos", "vel", "vol", "mass"), what)
        got, is_set = g.get_rest_shape()
        assert is_set and np.array_equal(hs.bits(got), hs.bits(other)), what

    const = np.zeros(1, PRESSURE_DTYPE)
    const["mode"], const["p"] = PRESSURE_CONSTANT, 10.0
    tables = (("mpm_set_bending", lambda: g.set_bending([1e-6]), lambda: g.set_bending([])),
              ("mpm_set_shell_bending", lambda: g.set_shell_bending([1e-6]), lambda: g.set_shell_bending([])),
              ("mpm_set_weave", lambda: g.set_weave([weave(E_warp=1e4, E_weft=1e4, G=1e3)]), lambda: g.set_weave([])),
              ("mpm_set_damping", lambda: g.set_damping([[1e-5, 0.0]]), lambda: g.set_damping([])),
              ("mpm_set_pressure", lambda: g.set_pressure(const), lambda: g.set_pressure([])),
              ("mpm_set_links", lambda: g.set_links(links([0], [143], 10.0, rest_length=0.1)), lambda: g.set_links(links([], [], 0.0))),
              ("mpm_set_anchors", lambda: g.set_anchors([Anchor(0, 0, (0.4, 0.4, 0.5), stiffness=10.0)]), lambda: g.set_anchors([])),
              ("mpm_set_pins", lambda: g.set_pins([Pin(0, 0, pose[0])]), lambda: g.set_pins([])))
    for says, setter, clear in tables:
        setter()
        refused(lambda: g.set_rest_shape(rest), says=says)
        refused(lambda: g.set_rest_shape(None), says=says)
        unchanged(says)
        clear()
    # what holds nothing derived from the rest shape is accepted
    from drake_amd import FF_ACCEL, ForceField
    g.set_force_fields([ForceField(kind=FF_ACCEL, u0=(0.0, 0.0, -1.0))])
    g.set_tearing([1.5])
    g.set_rest_shape(other)
    unchanged("accepted tables")
    g.set_force_fields([])
    g.set_tearing([0.0])
    # a NaN, a face without area, a face without a first edge: decided on the host, the first face named
    bad = rest.copy()
    bad[5, 1] = np.nan
    refused(lambda: g.set_rest_shape(bad), says="not finite")
    unchanged("NaN")
    flat = rest.copy()
    f = 100
    flat[idx[f, 2]] = flat[idx[f, 0]] + np.float32(2.0) * (flat[idx[f, 1]] - flat[idx[f, 0]])
    from drake_amd import rest_shape_check
    ok, first = rest_shape_check(flat, idx)
    if first == f:      # (the corner landed on the line exactly; else the face is thin and is accepted, as Finalize would)
        refused(lambda: g.set_rest_shape(flat), says=f"face {first}")
        unchanged("zero area")
    edge = rest.copy()
    edge[idx[f, 1]] = edge[idx[f, 0]]
    ok, first = rest_shape_check(edge, idx)
    assert not ok and 0 <= first <= f
    refused(lambda: g.set_rest_shape(edge), says=f"face {first}:")
    unchanged("zero edge")
    with pytest.raises(ValueError):
        g.set_rest_shape(rest[:-1])
    # a partitioned engine, in both directions
    nb = 64 // 4
    refused(lambda: g.dist_init(0, 1, [0, nb], 2, 2, 2), says="rest shape")
    refused(lambda: g.team_prepare(), says="rest shape")
    refused(lambda: g.chain_substeps(1, sp.DT), says="rest shape")
    unchanged("multi-rank set-up")
    g.run_substeps(2, 1e-4, -1)
    g.gpu_sync()
    assert g.stats()["error_flags"] == 0
    g.set_rest_shape(None)
    g.dist_init(0, 1, [0, nb], 2, 2, 2)
    refused(lambda: g.set_rest_shape(rest), says="partitioned")
    assert g.get_rest_shape()[1] is False
    g.destroy()


# ---- 6 -------------------------------------------------------------------------------------------------------------------
# The physics scenes: zero gravity unless said otherwise, membrane damping on (set AFTER the rest shape: its table holds
# the rest shape's row sums).  The figures of the first run on an MI355X are in profiles/rest_shape.txt.
PHYS_DT = 1e-4
PHYS_BETA = 1e-3             # s: damping ratio ~ 0.1 of the sheet's lowest in-plane mode (~220 rad/s)
RELAX_STEPS = 3000           # 0.3 s: about seven decay times of that mode
# The twin added at R and moved to 1.25 R by an upload is the engine without the feature doing the same thing.  Its mean
# edge ends RELAX_TWIN of the rest length away from it (measured on an MI355X, profiles/rest_shape.txt, rounded up to
# one digit); the engine with the feature is allowed twice that.
RELAX_TWIN = 5e-6
RELAX_FRACTION = 2.0 * RELAX_TWIN


def _relaxed(pos, idx, rest=None, upload=None, gravity=0.0, steps=RELAX_STEPS, pins=None):
    from drake_amd import BodyMotion, Pin
    g = _engine([(pos, None, idx)], deterministic=True, material={"gravity": gravity})
    if rest is not None:
        g.set_rest_shape(rest)
    g.set_damping([[PHYS_BETA, 0.0]])
    assert g.damping_max_stable_dt() >= PHYS_DT
    if pins is not None:
        at = pos if upload is None else upload
        g.reallocate_external_bodies(1)
        g.set_body_motions([BodyMotion(0, p_WB=(0, 0, 0))])
        g.set_pins([Pin(int(v), 0, at[v]) for v in pins])
    if upload is not None:
        hs.upload(g, upload)
    left = steps
    while left > 0:
        g.run_substeps(min(500, left), PHYS_DT, -1)
        left -= 500
    g.gpu_sync()
    nf = g.n_faces
    x = hs.by_id(g, hs.ARR().POSITIONS)[nf:]
    rows, total = g.measure()
    assert g.stats()["error_flags"] == 0, g.stats()
    g.destroy()
    return x, total


def test_a_sheet_added_stretched_relaxes_to_its_rest_length():
    rest, idx = rs.sheet(side=0.16, z=0.5)
    pose = rs.scaled(rest, 1.25)
    L0 = rs.mean_edge(rest, idx)
    xb, _ = _relaxed(pose, idx, rest=rest)
    xa, _ = _relaxed(rest, idx, upload=pose)                       # the twin added at R and perturbed the same way
    x0, _ = _relaxed(rest, idx)                                    # the untouched twin
    rb, ra = rs.mean_edge(xb, idx) / L0, rs.mean_edge(xa, idx) / L0
    moved0 = float(np.abs(x0.astype(np.float64) - rest).max())
    kappa = float(rm.rest_state(rm.Mesh("sheet", rest, np.zeros_like(rest), idx))["kappa"].max())
    still = 2.0 * 0.16 * rm.ENGINE_FACTOR * (rm.ORACLE_CQ + rm.ORACLE_CD) * rm.U24 * kappa + 4 * float(np.spacing(np.float32(0.58)))
    print(f"rest shape physics: mean edge / rest after {RELAX_STEPS} substeps: with set_rest_shape {rb:.9f}, twin {ra:.9f}; "
          f"untouched twin moved {moved0:.3g} (allowed {still:.3g})")
    assert abs(rb - 1.0) <= RELAX_FRACTION, (rb, ra)
    assert abs(rs.mean_edge(pose, idx) / L0 - 1.25) < 1e-5
    # an untouched sheet at rest stays: the residual strain of its own Dm^-1 (rest_meshes' bound) over the sheet's side is
    # how far its equilibrium lies from where it stands; it starts at rest, so it swings within twice that; and a few
    # ulps of its coordinates
    assert moved0 <= still, (moved0, still)


def test_a_pre_stretched_pinned_sheet_sags_less():
    pose, idx = rs.sheet(side=0.2, z=0.6)
    rest = rs.scaled(pose, 1.0 / 1.05)
    bnd = rs.boundary()
    xs, _ = _relaxed(pose, idx, rest=rest, gravity=-9.8, steps=2000, pins=bnd)
    xu, _ = _relaxed(pose, idx, gravity=-9.8, steps=2000, pins=bnd)
    sag_s, sag_u = float(0.6 - xs[:, 2].min()), float(0.6 - xu[:, 2].min())
    print(f"rest shape physics: sag of the pinned sheet under gravity: pre-stretched by 5 % {sag_s:.5f}, unstretched {sag_u:.5f}; "
          f"pinned vertices off their pins by at most {max(float(np.abs(x[bnd] - pose[bnd]).max()) for x in (xs, xu)):.3g}")
    for x in (xs, xu):
        assert np.abs(x[bnd] - pose[bnd]).max() < 1e-5       # (pinned: a thousandth of the sag's scale)
    assert 0.0 < sag_s < sag_u, (sag_s, sag_u)


def test_measured_mass_is_the_rest_shapes():
    """mpm_measure's total mass against the float64 sum of the masses of the rest shape -- the twin's, promoted, as
    tests/test_measure_gpu.py takes its masses from the engine --, within tests/measure.py's bound for a sum of masses
    (1e-9 of the sum); and against the float64 geometry of R under rest_meshes' volume bound"""
    from tests import measure as ms
    rest, pose, vel, idx = _dyn_sheets()
    A, B = _engine([(rest, None, idx)]), _engine([(pose, None, idx)])
    B.set_rest_shape(rest)
    want = float(hs.by_id(A, hs.ARR().MASSES).astype(np.float64).sum())
    got = float(B.measure()[1]["mass"])
    print(f"rest shape: measured mass {got!r}, the twin's {want!r}")
    assert abs(got - want) <= ms.bound_of("mass", want)
    ref = rm.rest_state(rm.Mesh("sheet", rest, np.zeros_like(rest), idx))
    m64 = float(ref["mass"].sum())
    # (a face's quarter volume enters four times -- its own particle and three vertex sums --, each within cV u of float64;
    # a vertex sum of at most six terms rounds five times, the product with the density once, the downloads not at all)
    allowed = float(4.0 * (CV * rm.U24 * ref["kappa"] * ref["mass"][:ref["nf"]]).sum() + 8.0 * rm.U24 * m64)
    assert abs(got - m64) <= allowed, (got, m64, allowed)
    pose_mass = float(rm.rest_state(rm.Mesh("sheet", pose, np.zeros_like(pose), idx))["mass"].sum())
    assert abs(pose_mass - m64) > 100 * allowed
    for g in (A, B):
        g.destroy()
