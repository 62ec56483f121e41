"""tests/harness.py against a stub engine: what upload hands to upload_particle_state, what engine leaves in _tri, the
views by original id, the bit compare, the environment manager and the margin record.  No library, no GPU."""
import os
import sys
import types

import numpy as np
import pytest

from tests import harness as hs

# two cloths: 4 vertices and 2 faces, 3 vertices and 1 face -- the second cloth's faces are offset by 4 in _tri
X0 = np.array([[0.1, 0.2, 0.3], [0.7, 0.2, 0.3], [0.1, 0.9, 0.3], [0.7, 0.9, 1.0 / 3.0]], np.float32)
T0 = np.array([[0, 1, 2], [1, 3, 2]], np.int32)
X1 = np.array([[0.25, 0.5, 0.125], [1.0 / 7.0, 0.5, 0.6], [0.3, 1.0 / 9.0, 0.6]], np.float32)
T1 = np.array([[0, 1, 2]], np.int32)
TRI = np.array([[0, 1, 2], [1, 3, 2], [4, 5, 6]])
NF, NV = 3, 7
PIDS = np.array([4, 0, 9, 2, 7, 1, 8, 3, 6, 5], np.uint32)      # slot -> original id: faces 0..2, vertices 3..9


class _Arr:
    PIDS, POSITIONS = "pids", "positions"


class _Stub:
    """records upload_particle_state, serves download(PIDS) and download(POSITIONS) (row i of slot s: the id in slot s)"""
    n_faces, n_verts = NF, NV

    def __init__(self):
        self.uploads = []

    def download(self, which):
        if which == _Arr.PIDS:
            return PIDS.copy()
        assert which == _Arr.POSITIONS
        return np.repeat(PIDS.astype(np.float32)[:, None], 3, axis=1)

    def upload_particle_state(self, *args):
        self.uploads.append(args)


class _Engine(_Stub):
    """what harness.engine drives: the calls in order"""
    def __init__(self, bits, mat):
        super().__init__()
        self.calls = [("create", bits, mat.gravity, os.environ.get("HARNESS_TEST_VAR"))]

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        return lambda *a: self.calls.append((name,) + a)

    @staticmethod
    def default_material():
        return types.SimpleNamespace(gravity=-9.8, density=1000.0)


class _ClothMaterial(types.SimpleNamespace):
    @staticmethod
    def of(mat):
        return _ClothMaterial(density=mat.density)


@pytest.fixture
def stub(monkeypatch):
    monkeypatch.setitem(sys.modules, "drake_amd", types.SimpleNamespace(ARR=_Arr, GpuMpm=_Engine, ClothMaterial=_ClothMaterial))
    g = _Stub()
    g._tri = TRI
    return g


def _vertex_rows():
    r = np.random.default_rng(5)
    return (np.concatenate([X0, X1]), r.uniform(-3, 3, (NV, 3)).astype(np.float32))


def test_upload_face_rows_permutation_and_c(stub):
    x, v = _vertex_rows()
    F = np.arange(NF * 9, dtype=np.float32).reshape(NF, 9)
    hs.upload(stub, x, v, F)
    pos, vel, C, vol, Fgot = stub.uploads[0]
    for got, a in ((pos, x), (vel, v)):
        faces = np.array([[np.float32((float(a[i, k]) + float(a[j, k]) + float(a[l, k])) / 3.0) for k in range(3)] for i, j, l in TRI])
        want = np.concatenate([a[TRI].astype(np.float64).mean(axis=1).astype(np.float32), a])
        assert np.array_equal(hs.bits(want[:NF]), hs.bits(faces))          # (float64 mean, rounded once)
        assert got.dtype == np.float32 and np.array_equal(hs.bits(got), hs.bits(want[PIDS]))
        assert not np.array_equal(hs.bits(got), hs.bits(want))             # (the permutation is not the identity)
    assert C.shape == (NF + NV, 9) and C.dtype == np.float32 and not C.any()
    assert vol is None and Fgot is F


def test_upload_broadcasts_one_velocity(stub):
    x, _ = _vertex_rows()
    one = np.array([0.3, -0.2, 1.0 / 3.0], np.float32)
    hs.upload(stub, x, one)
    hs.upload(stub, x, np.repeat(one[None], NV, axis=0))
    hs.upload(stub, x)
    a, b, c = stub.uploads
    assert a[1].shape == (NF + NV, 3) and np.array_equal(hs.bits(a[1]), hs.bits(b[1]))
    assert np.array_equal(hs.bits(a[1]), hs.bits(np.broadcast_to(one, (NF + NV, 3))))    # (the mean of three equal numbers)
    assert not c[1].any() and a[4] is None and np.array_equal(hs.bits(a[0]), hs.bits(c[0]))


@pytest.mark.parametrize("flat", [False, True])
def test_engine_tri_and_calls(stub, flat):
    T = (lambda t: t.reshape(-1)) if flat else (lambda t: t)
    v1 = np.ones_like(X1)
    g = hs.engine([(X0, T(T0)), (X1, v1, T(T1))], bits=7, material=dict(gravity=0.0), mats=[None, dict(density=2.0)],
                  deterministic=None, fast_math=False, bodies=2, env={"HARNESS_TEST_VAR": "1"})
    assert g._tri.shape == (NF, 3) and np.array_equal(g._tri, TRI)
    assert "HARNESS_TEST_VAR" not in os.environ
    names = [c[0] for c in g.calls]
    assert names == ["create", "set_fast_math", "add_qr_cloth", "add_qr_cloth", "finalize", "reallocate_external_bodies"]
    assert g.calls[0] == ("create", 7, 0.0, "1") and g.calls[1] == ("set_fast_math", False) and g.calls[5][1] == 2
    (_, p0, w0, i0, m0), (_, p1, w1, i1, m1) = g.calls[2:4]
    assert p0 is X0 and not w0.any() and w0.shape == X0.shape and m0 is None
    assert p1 is X1 and w1 is v1 and m1.density == 2.0
    # the defaults: deterministic on, fast math untouched, no bodies
    g = hs.engine([(X0, T0)])
    assert [c[0] for c in g.calls] == ["create", "set_deterministic", "add_qr_cloth", "finalize"]
    assert g.calls[0] == ("create", 6, -9.8, None) and g.calls[1] == ("set_deterministic", True)


def test_vertices_and_by_id_invert_the_permutation(stub):
    ids = np.repeat(np.arange(NF + NV, dtype=np.float32)[:, None], 3, axis=1)
    assert np.array_equal(hs.by_id(stub, _Arr.POSITIONS), ids)
    f, v = hs.by_id(stub, _Arr.POSITIONS, split=True)
    assert np.array_equal(f, ids[:NF]) and np.array_equal(v, ids[NF:])
    assert np.array_equal(hs.vertices(stub, _Arr.POSITIONS), ids[NF:])


def test_bits_and_same_bits():
    a32, a64 = np.array([1.5, -0.0], np.float32), np.array([1.5, -0.0], np.float64)
    assert hs.bits(a32).dtype == np.uint32 and hs.bits(a64).dtype == np.uint64 and hs.bits(a32).shape == hs.bits(a64).shape
    assert hs.bits(a32)[1] == 0x80000000 and hs.bits(np.arange(3, dtype=np.int64)).dtype == np.uint64
    assert hs.bits(np.ones((4, 3), np.float32)[:, ::2]).shape == (4, 2)                    # (not contiguous: copied, not cast)
    for other in (np.zeros(4, np.uint8), np.zeros(4, np.float16)):
        with pytest.raises(KeyError):
            hs.bits(other)
    hs.same_bits(dict(x=a32, y=a64), dict(x=a32.copy(), y=a64.copy()), "equal")
    with pytest.raises(AssertionError):
        hs.same_bits(dict(x=a32), dict(x=np.array([1.5, 0.0], np.float32)), "the sign of zero")


def test_environ_restores(monkeypatch):
    monkeypatch.setenv("HARNESS_WAS_SET", "old")
    monkeypatch.delenv("HARNESS_WAS_UNSET", raising=False)
    env = {"HARNESS_WAS_SET": "new", "HARNESS_WAS_UNSET": "1"}
    with hs.environ(env):
        assert os.environ["HARNESS_WAS_SET"] == "new" and os.environ["HARNESS_WAS_UNSET"] == "1"
    assert os.environ["HARNESS_WAS_SET"] == "old" and "HARNESS_WAS_UNSET" not in os.environ
    with pytest.raises(RuntimeError):
        with hs.environ(env):
            raise RuntimeError
    assert os.environ["HARNESS_WAS_SET"] == "old" and "HARNESS_WAS_UNSET" not in os.environ
    for nothing in (None, {}):
        before = dict(os.environ)
        with hs.environ(nothing):
            assert dict(os.environ) == before
        assert dict(os.environ) == before


def test_record_appends_the_margin_row(monkeypatch):
    fake = types.SimpleNamespace(MARGINS=[], TAG=" [tag]")
    import tests
    monkeypatch.setitem(sys.modules, "tests.helpers", fake)
    monkeypatch.setattr(tests, "helpers", fake, raising=False)
    hs.record("what", 0.25)
    hs.record("what", 0.5, prefix="weave: ")
    assert fake.MARGINS == [(0.25, "what [tag]", 1.0, 0.25, 0.25), (0.5, "weave: what [tag]", 1.0, 0.5, 0.5)]
