"""tests/rest_meshes.py against the oracle, without a GPU: the float64 restatement of Finalize's rest state against the
double build of the oracle (1e-12 kappa in the units of the bound), the float build against the restatement (this
MEASURES the constants cQ, cD, cV that the module records and the GPU test allows the engine four times of), and the
properties the meshes are made for."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import rest_meshes as rm

NAMES = ("orientations", "slivers", "scales", "valence") + tuple(f"tails_{n}" for n in rm.TAILS)
_ORACLES = {}


def _oracle(name, real):
    if (name, real) not in _ORACLES:
        o = orc.OracleMpm(rm.BITS, real=real)
        o.add_qr_cloth(*rm.meshes()[name][0].sheet())
        o.finalize()
        _ORACLES[name, real] = rm.of_oracle(o)
    return _ORACLES[name, real]


def test_mesh_names():
    assert tuple(rm.meshes()) == NAMES


@pytest.mark.parametrize("name", NAMES)
def test_restatement_matches_the_double_oracle(name):
    mesh, ref = rm.meshes()[name]
    got = _oracle(name, np.float64)
    # 1e-12 kappa in the bound's units: the constants of bound_ratios are 1e-12 / 2^-24 (u = 2^-24 kappa)
    c = 1e-12 / rm.U24
    r = rm.bound_ratios(got, ref, c, c, c)
    for field in ("F0", "Dm", "volf"):
        assert r[field].size == mesh.nf
        assert r[field].max(initial=0.0) <= 1.0, (field, int(np.argmax(r[field])), float(r[field].max()))
    # (vertex volumes: the faces' share alone, the summation term of the float bound left out)
    kv = ref["kappa"] * ref["vol"][:mesh.nf]
    allowed = np.array([1e-12 * kv[fs].sum() for fs in ref["vfaces"]])
    assert np.all(np.abs(got["vol"][mesh.nf:] - ref["vol"][mesh.nf:]) <= allowed)
    # (the means and the vertices themselves: 1e-12 of the largest corner component)
    for field, scale in (("pos", "xmax"), ("vel", "vmax")):
        d = np.abs(got[field][:mesh.nf] - ref[field][:mesh.nf]).max(axis=1)
        assert np.all(d <= 1e-12 * ref[scale])
        assert np.array_equal(got[field][mesh.nf:], ref[field][mesh.nf:])


def _measured():
    worst = dict(F0=(0.0, None), Dm=(0.0, None), volf=(0.0, None))
    for name in NAMES:
        mesh, ref = rm.meshes()[name]
        r = rm.unit_ratios(_oracle(name, np.float32), ref)
        for k in worst:
            assert np.all(np.isfinite(r[k])), (name, k)
            f = int(np.argmax(r[k]))
            if r[k][f] > worst[k][0]:
                worst[k] = (float(r[k][f]), (name, f, float(ref["kappa"][f])))
    return worst


def test_float_oracle_constants():
    """cQ, cD, cV of the float build of the oracle: at most 32, and the values the module records"""
    w = _measured()
    print("measured on the float oracle (constant, (mesh, face, kappa)):", w)
    for k, recorded in (("F0", rm.ORACLE_CQ), ("Dm", rm.ORACLE_CD), ("volf", rm.ORACLE_CV)):
        assert w[k][0] <= rm.C_LIMIT, (k, w[k])
        assert round(w[k][0], 2) == recorded, (k, w[k], recorded)
    for k in (rm.ORACLE_CQ, rm.ORACLE_CD, rm.ORACLE_CV):
        assert f"= {k:.2f}" in rm.__doc__


@pytest.mark.parametrize("name", NAMES)
def test_float_oracle_within_its_own_bound(name):
    """every field of the float oracle, vertex volumes and face means included, under the bound with its own constants"""
    mesh, ref = rm.meshes()[name]
    got = _oracle(name, np.float32)
    r = rm.bound_ratios(got, ref, rm.ORACLE_CQ + 0.005, rm.ORACLE_CD + 0.005, rm.ORACLE_CV + 0.005)
    for field, a in r.items():
        assert a.max(initial=0.0) <= 1.0, (field, int(np.argmax(a)), float(a.max()))
    # the oracle's vertex volume IS the float32 sum of its face volumes in ascending face id
    assert np.array_equal(got["vol"][mesh.nf:], rm.f32_sum_ascending(got["vol"][:mesh.nf], ref["vfaces"]))


@pytest.mark.parametrize("name", NAMES)
def test_every_mesh_is_inside_the_domain_and_well_posed(name):
    mesh, ref = rm.meshes()[name]
    assert 1 <= mesh.nf <= 4000
    assert mesh.pos.dtype == np.float32 and mesh.vel.dtype == np.float32
    assert ref["pos"].min() >= rm.LO and ref["pos"].max() <= rm.HI          # face particles and vertices
    assert np.all(np.isfinite(ref["kappa"])) and ref["kappa"].max() <= rm.KAPPA_MAX and ref["kappa"].min() >= 1.0
    assert np.all(ref["vol"][:mesh.nf] > 0)
    # no index repeated within a face, every index in range
    i = mesh.idx
    assert i.min() >= 0 and i.max() < mesh.nv
    assert np.all((i[:, 0] != i[:, 1]) & (i[:, 1] != i[:, 2]) & (i[:, 0] != i[:, 2]))
    # 1 / sigma_min is the 2-norm of the restated Dm^-1
    D = ref["Dm"].reshape(-1, 2, 2)
    assert np.allclose(np.linalg.norm(D, 2, axis=(1, 2)), ref["inv_smin"], rtol=1e-9)
    if name in ("orientations", "slivers", "scales"):
        assert np.array_equal(i, np.arange(3 * mesh.nf).reshape(-1, 3))     # three vertices of their own


def test_orientations_take_the_zero_branches():
    mesh, ref = rm.meshes()["orientations"]
    b = rm.givens_branches(mesh)
    assert b["first_c_plus"] > 0 and b["first_c_minus"] > 0, b
    assert b["second"] == 0 and b["third"] == 0, b     # (degenerate faces only: module docstring)
    x = mesh.pos[mesh.idx]
    D0, D1 = x[:, 1] - x[:, 0], x[:, 2] - x[:, 0]
    for ax in range(3):
        o1, o2 = (ax + 1) % 3, (ax + 2) % 3
        for sg in (1, -1):
            assert np.any((D0[:, o1] == 0) & (D0[:, o2] == 0) & (np.sign(D0[:, ax]) == sg)), (ax, sg)
        # D0 in the plane, D1 not; D1 with one and with two zero components; the whole triangle in the plane, both ways
        assert np.any((D0[:, ax] == 0) & (D0[:, o1] != 0) & (D0[:, o2] != 0) & (D1[:, ax] != 0))
        assert np.any((D1[:, ax] == 0) & (D1[:, o1] != 0) & (D1[:, o2] != 0) & np.all(D0 != 0, axis=1))
        assert np.any((D1[:, ax] != 0) & (D1[:, o1] == 0) & (D1[:, o2] == 0) & np.all(D0 != 0, axis=1))
        flat = (D0[:, ax] == 0) & (D1[:, ax] == 0)
        nz = ref["F0"][:, 3 * ax + 2]                   # the normal's component along the axis: +-1
        assert np.any(flat & (nz > 0.5)) and np.any(flat & (nz < -0.5))
    assert mesh.info["tags"].count("random rotation") == 500
    # on the random part nothing is special: every entry of F0 is used
    assert np.all(np.abs(ref["F0"][mesh.info["n_fixed"]:]).min(axis=0) < 0.05)


def test_slivers_cover_every_decade_in_every_corner_order():
    mesh, ref = rm.meshes()["slivers"]
    dec = np.floor(np.log10(ref["kappa"])).astype(int)
    counts = {d: int((dec == d).sum()) for d in range(4)}
    assert all(c >= 20 for c in counts.values()), counts
    assert ref["kappa"].max() >= 5e3
    kind = np.array(mesh.info["kind"])
    for k in np.unique(kind):
        assert set(dec[kind == k]) >= {0, 1, 2, 3}, k
    assert len(np.unique(kind)) == 6
    # the three orders of one triangle hold the same three points
    n = mesh.nf // 6
    a, b = mesh.pos[mesh.idx[:n]], mesh.pos[mesh.idx[n:2 * n]]
    assert np.array_equal(a[:, [1, 2, 0]], b)


def test_scales_span_more_than_eight_decades_of_volume():
    mesh, ref = rm.meshes()["scales"]
    v = ref["vol"][:mesh.nf]
    assert v.max() / v.min() > 1e8
    x = mesh.pos[mesh.idx].astype(np.float64)
    edges = np.stack([np.linalg.norm(x[:, (c + 1) % 3] - x[:, c], axis=1) for c in range(3)], 1)
    assert edges.max() <= 0.3 * (1 + 1e-6) and edges.max() > 0.29
    assert edges.min() < 1.01e-3 * rm.DX and edges.min() > 0.3e-3 * rm.DX
    assert ref["kappa"].max() < 10


def test_valence_mesh():
    mesh, ref = rm.meshes()["valence"]
    val = ref["valence"]
    assert set(rm.HUB_VALENCES) <= set(val) and 0 in val
    assert val[mesh.info["isolated"]] == 0 and int((val == 0).sum()) == 1
    assert mesh.nv > 256 and mesh.nv % 256 and mesh.nv % rm.VF_CHUNK and mesh.nv > 10 * rm.VF_CHUNK
    assert val[255] == 9 and mesh.info["isolated"] == 256 and val[mesh.nv - 1] == 40
    spans = []
    for k, kind, v in mesh.info["hubs"]:
        fs = np.array(ref["vfaces"][v])
        assert len(fs) == k == val[v]
        assert np.all(np.diff(fs) > 1) if k > 1 else True                  # interleaved with the other hubs' faces
        corner = [int(np.flatnonzero(mesh.idx[f] == v)[0]) for f in fs]
        assert k < 3 or set(corner) == {0, 1, 2}
        vols = ref["vol"][fs]
        spans.append((k, kind, vols.max() / vols.min()))
        if kind == "petals" and k > 1:
            assert vols.max() / vols.min() > 1e3 * 0.999, spans[-1]
            # ... and the float32 sum of that hub does depend on its order
    order_matters = 0
    vol32 = ref["vol"][:mesh.nf].astype(np.float32)
    for k, kind, v in mesh.info["hubs"]:
        fs = ref["vfaces"][v]
        order_matters += rm.f32_sum_ascending(vol32, [fs])[0] != rm.f32_sum_ascending(vol32, [fs[::-1]])[0]
    assert order_matters >= 4, order_matters


def test_tails():
    for n in rm.TAILS:
        mesh, ref = rm.meshes()[f"tails_{n}"]
        assert mesh.nf == n and mesh.nv == n + 2
        assert set(ref["valence"]) <= {1, 2, 3}


def test_three_cloths_are_the_merged_mesh():
    parts, whole = rm.three_cloths()
    assert len(parts) == 3 and whole.nf == sum(p.nf for p in parts) and whole.nv == sum(p.nv for p in parts)
    sl, va = rm.meshes()["slivers"][0], rm.meshes()["valence"][0]
    assert np.array_equal(whole.pos, np.concatenate([sl.pos, va.pos]))
    assert np.array_equal(whole.idx, np.concatenate([sl.idx, va.idx + sl.nv]))
