"""Finalize on the device -- k_init_faces, k_init_vertex_adjacency, k_init_vertex_volumes, k_init_masses, the host half of
mpm_finalize (index offsets per cloth, the vertex -> face CSR) and the volume / mass downloads -- per face and per vertex
against the float64 restatement of tests/rest_meshes.py, on its meshes:

    |F0 - F0_64| <= 4 cQ u     |Dm^-1 - Dm^-1_64| <= 4 cD u ||Dm^-1||_2     |vol - vol_64| <= 4 cV u vol_64     (u = 2^-24 kappa)

with cQ, cD, cV the constants MEASURED on the float oracle (rest_meshes.ORACLE_C*, asserted by tests/test_rest_meshes.py)
and 4 the allowance for another float evaluation of the same formula; the face particle's position and velocity within
3 2^-24 of the largest corner component; the vertex volumes within the faces' share plus (valence - 1) 2^-24 of the sum.
No face and no vertex is left out of any comparison.  Then what needs no constant: the signs and the zero of Dm^-1, the
orthogonality of F0 without kappa, det F0 > 0, the vertex volume as THE float32 sum of the downloaded face volumes in
ascending face id, bit for bit; that the rest state has no strain ([D0 D1] Dm^-1 = the in-plane columns of F0, what k_fem
forms on the first substep); and bit-exact metamorphic checks: one cloth or three, one material or three, masses,
the deterministic mode.  test_zz_margins lists the worst ratio per mesh and field (profiles/rest_state_margins.txt)."""
import numpy as np
import pytest

from tests import rest_meshes as rm

pytestmark = pytest.mark.gpu

NAMES = ("orientations", "slivers", "scales", "valence") + tuple(f"tails_{n}" for n in rm.TAILS)
CQ, CD, CV = (rm.ENGINE_FACTOR * c for c in (rm.ORACLE_CQ, rm.ORACLE_CD, rm.ORACLE_CV))
DENSITIES = (500.0, 2000.0, 7300.0)
WORST = {}       # (mesh, field) -> (worst error / allowed, face or vertex, kappa)
_STATES = {}


def _finalized(cloths, deterministic=False, densities=None):
    """the rest state of an engine holding `cloths` (meshes), in original order; densities: one per cloth, through
    add_qr_cloth(material=...) (a multi-material engine)"""
    from drake_amd import ClothMaterial, GpuMpm
    g = GpuMpm(rm.BITS)
    if deterministic:
        g.set_deterministic(True)
    for i, m in enumerate(cloths):
        mat = None
        if densities is not None:
            mat = ClothMaterial.of(GpuMpm.default_material())
            mat.density = densities[i]
        g.add_qr_cloth(*m.sheet(), material=mat)
    g.finalize()
    assert (g.n_faces, g.n_verts) == (sum(m.nf for m in cloths), sum(m.nv for m in cloths))
    out = rm.of_engine(g, masses=True)
    assert g.stats()["error_flags"] == 0
    g.destroy()
    return out


def _state(name):
    if name not in _STATES:
        _STATES[name] = _finalized([rm.meshes()[name][0]])
    return _STATES[name]


def _three(kind):
    if kind not in _STATES:
        parts, whole = rm.three_cloths()
        _STATES[kind] = dict(merged=lambda: _finalized([whole]), three=lambda: _finalized(parts),
                             materials=lambda: _finalized(parts, densities=DENSITIES),
                             deterministic=lambda: _finalized(parts, deterministic=True))[kind]()
    return _STATES[kind]


def _kappa_of(ref, field, i):
    return float(ref["kappa"][i]) if field != "volv" else float(max((ref["kappa"][f] for f in ref["vfaces"][i]), default=0))


@pytest.mark.parametrize("name", NAMES)
def test_fields_against_float64(name):
    mesh, ref = rm.meshes()[name]
    got = _state(name)
    ratios = rm.bound_ratios(got, ref, CQ, CD, CV)
    failures = []
    for field, r in ratios.items():
        assert r.size == (mesh.nv if field == "volv" else mesh.nf)
        i = int(np.argmax(r))
        WORST[name, field] = (float(r[i]), i, _kappa_of(ref, field, i))
        print(f"{name} {field}: worst error / allowed {r[i]:.3f} at {i} (kappa {WORST[name, field][2]:.3g})")
        if not r[i] <= 1.0:
            failures.append(f"{name} {field}: {'vertex' if field == 'volv' else 'face'} {i}, kappa "
                            f"{WORST[name, field][2]:.4g}, {r[i]:.3f} x allowed; {int((r > 1).sum())} over the bound")
    # the vertices themselves come back as they went in
    assert np.array_equal(got["pos"][mesh.nf:], mesh.pos) and np.array_equal(got["vel"][mesh.nf:], mesh.vel)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("name", NAMES)
def test_properties_without_a_constant(name):
    mesh, ref = rm.meshes()[name]
    got = _state(name)
    Dm, F = got["Dm"], got["F0"].astype(np.float64).reshape(-1, 3, 3)
    assert Dm.dtype == np.float32 and np.all(np.isfinite(Dm)) and np.all(np.isfinite(F))
    assert np.all(Dm[:, 0] > 0) and np.all(Dm[:, 3] > 0)
    assert np.all(Dm[:, 2] == 0)
    # a product of three rotations stays orthogonal however thin the triangle: no kappa here
    orth = np.abs(np.einsum("fki,fkj->fij", F, F) - np.eye(3)).reshape(mesh.nf, -1).max(axis=1)
    WORST[name, "orthogonality / (16 2^-24)"] = (float(orth.max() / (16 * rm.U24)), int(np.argmax(orth)),
                                                 float(ref["kappa"][np.argmax(orth)]))
    assert orth.max() <= 16 * rm.U24, (int(np.argmax(orth)), float(orth.max() / rm.U24))
    assert np.all(np.linalg.det(F) > 0)


@pytest.mark.parametrize("name", NAMES)
def test_rest_means_zero_strain(name):
    """[D0 D1] Dm^-1, in float64 from the engine's own Dm^-1 and the uploaded positions, is the in-plane part of the
    engine's own F0 within (cQ + cD) 4 u"""
    mesh, ref = rm.meshes()[name]
    got = _state(name)
    Dm, F = got["Dm"].astype(np.float64), got["F0"].astype(np.float64).reshape(-1, 3, 3)
    c0 = ref["D0"] * Dm[:, 0, None]
    c1 = ref["D0"] * Dm[:, 1, None] + ref["D1"] * Dm[:, 3, None]
    err = np.maximum(np.abs(c0 - F[:, :, 0]).max(axis=1), np.abs(c1 - F[:, :, 1]).max(axis=1))
    r = err / ((rm.ORACLE_CQ + rm.ORACLE_CD) * rm.ENGINE_FACTOR * rm.U24 * ref["kappa"])
    i = int(np.argmax(r))
    WORST[name, "zero strain"] = (float(r[i]), i, float(ref["kappa"][i]))
    assert np.all(np.isfinite(r)) and r[i] <= 1.0, (name, i, float(ref["kappa"][i]), float(r[i]))


@pytest.mark.parametrize("name", NAMES)
def test_vertex_volume_is_the_float_sum_in_ascending_face_id(name):
    mesh, ref = rm.meshes()[name]
    got = _state(name)
    vol = got["vol"]
    assert vol.dtype == np.float32
    expect = rm.f32_sum_ascending(vol[:mesh.nf], ref["vfaces"])
    bad = np.flatnonzero(vol[mesh.nf:].view(np.uint32) != expect.view(np.uint32))
    assert bad.size == 0, (name, bad[:8], ref["valence"][bad[:8]])
    if name == "valence":
        assert vol[mesh.nf + mesh.info["isolated"]] == 0 and not np.signbit(vol[mesh.nf + mesh.info["isolated"]])


@pytest.mark.parametrize("name", NAMES)
def test_single_material_masses(name):
    got = _state(name)
    assert np.array_equal(got["mass"], got["vol"] * np.float32(rm.DENSITY))      # (a float32 product)
    assert got["mass"].dtype == np.float32


def _same(a, b, fields=("F0", "Dm", "pos", "vel", "vol", "mass")):
    for f in fields:
        assert a[f].dtype == b[f].dtype and a[f].shape == b[f].shape, f
        bad = np.flatnonzero(np.any((a[f].view(np.uint32) != b[f].view(np.uint32)).reshape(len(a[f]), -1), axis=1))
        assert bad.size == 0, (f, bad[:8])


def test_three_cloths_equal_the_merged_cloth():
    _same(_three("merged"), _three("three"))


def test_merged_cloth_against_float64():
    """(the cloth of the metamorphic tests is itself right: slivers and valence with their indices offset)"""
    _, whole = rm.three_cloths()
    r = rm.bound_ratios(_three("merged"), rm.rest_state(whole), CQ, CD, CV)
    for field, a in r.items():
        assert a.max() <= 1.0, (field, int(np.argmax(a)), float(a.max()))


def test_per_cloth_materials():
    parts, whole = rm.three_cloths()
    one, mat = _three("three"), _three("materials")
    _same(one, mat, ("F0", "Dm", "pos", "vel"))
    rho = np.concatenate([np.full(p.nf, d, np.float32) for p, d in zip(parts, DENSITIES)] +
                         [np.full(p.nv, d, np.float32) for p, d in zip(parts, DENSITIES)])
    # k_init_masses: the float32 product of the volume (as the single-material engine has it) and the cloth's density
    expect = one["vol"] * rho
    bad = np.flatnonzero(mat["mass"].view(np.uint32) != expect.view(np.uint32))
    assert bad.size == 0, (bad[:8], rho[bad[:8]])
    # the volume comes back as mass / density: within one ulp
    ulp = np.spacing(one["vol"])
    bad = np.flatnonzero(~(np.abs(mat["vol"].astype(np.float64) - one["vol"].astype(np.float64)) <= ulp))
    assert bad.size == 0, (bad[:8], mat["vol"][bad[:8]], one["vol"][bad[:8]])
    assert mat["vol"][whole.nf + parts[0].nv + parts[1].nv + parts[2].info["isolated"]] == 0


def test_deterministic_mode_has_the_same_rest_state():
    _same(_three("three"), _three("deterministic"))


def _vertex_forces(mesh, x_deformed):
    """CalcFemStateAndForce's vertex forces (nv, 3), by original vertex id, of `mesh` finalized at rest and then moved to
    x_deformed (float32 vertex positions)"""
    from drake_amd import ARR as A, GpuMpm
    g = GpuMpm(rm.BITS)
    g.add_qr_cloth(*mesh.sheet())
    g.finalize()
    pos = np.concatenate([(x_deformed.astype(np.float64)[mesh.idx].sum(axis=1) / 3).astype(np.float32), x_deformed])
    g.upload_particle_state(pos[g.download(A.PIDS)])
    g.rebuild_mapping(True)
    g.calc_fem_state_and_force(1e-3)
    g.gpu_sync()
    f = np.empty((g.n_particles, 3), np.float32)
    f[g.download(A.PIDS)] = g.download(A.FORCES)
    assert g.stats()["error_flags"] == 0
    g.destroy()
    return f[mesh.nf:]


def test_adjacency_tables_gather_every_corner_in_ascending_face_id():
    """The tables Finalize's host half makes -- the corners' ranks around their vertices, the mark of a vertex with more
    than eight faces, the vertex -> face CSR -- are what CalcFemStateAndForce sums vertex forces through.  The valence
    mesh, strained, against the same faces as disjoint triangles (whose vertex forces ARE the corner records): the force
    on every shared vertex is, bit for bit, the float32 sum of its corners' in ascending face id (mpm_step.h:
    vertex_force_value).  Probes the tables only; the forces' values are tests/test_fem_regimes_gpu.py's."""
    mesh, ref = rm.meshes()["valence"]
    A = np.array([[1.08, 0.03, 0.0], [0.0, 0.94, 0.02], [0.01, 0.0, 1.03]])
    x = (0.5 + (mesh.pos.astype(np.float64) - 0.5) @ A.T).astype(np.float32)
    apart = rm.Mesh("valence, disjoint", mesh.pos[mesh.idx], mesh.vel[mesh.idx], np.arange(3 * mesh.nf))
    corner = _vertex_forces(apart, x[mesh.idx].reshape(-1, 3)).reshape(mesh.nf, 3, 3)      # [face, corner, component]
    got = _vertex_forces(mesh, x)
    assert np.all(np.isfinite(corner)) and np.all(np.abs(corner).max(axis=2) > 0)
    expect = np.zeros((mesh.nv, 3), np.float32)
    for v, fs in enumerate(ref["vfaces"]):
        s = np.zeros(3, np.float32)
        for f in fs:
            s = s + corner[f, int(np.flatnonzero(mesh.idx[f] == v)[0])]
        expect[v] = s
    bad = np.flatnonzero(np.any(got != expect, axis=1))
    assert bad.size == 0, ("vertices", bad[:8], "valence", ref["valence"][bad[:8]])
    assert np.all(got[mesh.info["isolated"]] == 0)
    for k, _, v in mesh.info["hubs"]:                      # (no hub's force is a cancellation to nothing)
        assert np.abs(got[v]).max() > 0, k


def test_vertex_in_no_face_stays_a_particle():
    """A vertex in no face has volume 0 and no mass; it is a particle all the same (the reference keeps it and moves it
    with the grid).  The first re-sort must not take it for a slot that a migration released: after Finalize, and after
    one substep, it is where the oracle has it, and so is everything else."""
    from drake_amd import ARR as A
    from tests.helpers import build_pair, close, natural_scales
    mesh, ref = rm.meshes()["valence"]
    o, g = build_pair(domain_bits=rm.BITS, sheets=[mesh.sheet()])
    iso = mesh.nf + mesh.info["isolated"]
    pid = g.download(A.PIDS)
    assert np.array_equal(np.sort(pid), np.arange(mesh.nf + mesh.nv))         # every particle has a slot
    assert np.array_equal(g.download(A.POSITIONS)[pid == iso][0], mesh.pos[mesh.info["isolated"]])
    sc = natural_scales(o, 1e-3)
    o.substep(1e-3, -1)
    g.substep(1e-3, -1)
    g.gpu_sync()
    assert g.stats()["error_flags"] == 0
    so = o.state_in_original_order()
    pid = g.download(A.PIDS)
    x, v = np.empty_like(so["pos"]), np.empty_like(so["vel"])
    x[pid], v[pid] = g.download(A.POSITIONS), g.download(A.VELOCITIES)
    close(x, so["pos"], scale=1.0, what="valence mesh, one substep: pos")
    close(v, so["vel"], scale=sc["vel"], what="valence mesh, one substep: vel")
    close(x[iso], so["pos"][iso], scale=1.0, what="vertex in no face, one substep: pos")
    close(v[iso], so["vel"][iso], scale=sc["vel"], what="vertex in no face, one substep: vel")
    g.destroy()


def test_zz_margins():
    """(prints the table of the worst ratios; run after the tests above)"""
    lines = ["Finalize's rest state on the engine against float64 (tests/test_rest_state_gpu.py): worst error / allowed "
             "per mesh and field.",
             f"allowed = {rm.ENGINE_FACTOR:g} x the float oracle's measured constant (cQ {rm.ORACLE_CQ}, cD {rm.ORACLE_CD}, "
             f"cV {rm.ORACLE_CV}) x u, u = 2^-24 kappa;",
             "so ratio x 4 x constant is the engine's own constant on that mesh, and 0.25 is where the float oracle's "
             "worst face lies.",
             "  ratio   engine's constant   at (face / vertex)   kappa      mesh, field"]
    const = dict(F0=rm.ORACLE_CQ, Dm=rm.ORACLE_CD, volf=rm.ORACLE_CV)
    for (name, field), (r, i, kappa) in sorted(WORST.items(), key=lambda kv: (NAMES.index(kv[0][0]), kv[0][1])):
        own = f"{r * rm.ENGINE_FACTOR * const[field]:8.3f}" if field in const else "       -"
        lines.append(f"  {r:6.3f}  {own}            {i:6d}               {kappa:9.3g}  {name}, {field}")
    print("\n".join(lines))
