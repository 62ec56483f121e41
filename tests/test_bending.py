"""Bending stiffness on the CPU: the library exports the entry points, mpm_bending_matrix (the host assembly of Q that
mpm_set_bending uses) agrees with the numpy restatement of tests/bending.py -- pattern, values, zero row sums,
symmetry --, refuses a face of zero area, the restatement's force is the gradient of its energy and vanishes on affine
images, and the float32 restatement of the engine's row evaluation stays inside the bound R_i 2^-24 B_i on every mesh
and state.  No GPU."""
import numpy as np
import pytest

from tests import bending as bd

K = 2.5e-5
PAIRS = [(m, s) for m in bd.MESHES for s in bd.STATES]


def _model(name):
    X, T = bd.mesh(name)
    H = bd.hinges(X, T)
    Q, P = bd.q_dense(len(X), H)
    return X, T, H, Q, P


def test_library_exports_the_bending_entry_points():
    from drake_amd import capi
    lib = capi.load_library()
    for name in ("mpm_set_bending", "mpm_get_bending", "mpm_bending_forces", "mpm_bending_max_stable_dt",
                 "mpm_bending_matrix"):
        assert hasattr(lib, name), name
        assert name in capi.SYMBOLS
    for name in ("set_bending", "get_bending", "bending_forces", "bending_max_stable_dt"):
        assert hasattr(capi.GpuMpm, name), name


def test_mesh_shapes():
    """the meshes are what the tests say they are"""
    assert len(bd.hinges(*bd.mesh("strip"))) == 1 and len(bd.hinges(*bd.mesh("triangle"))) == 0
    X, T = bd.mesh("fan")
    assert np.bincount(T.reshape(-1))[0] == 12 and len(X) > 64
    _, _, _, _, P = _model("fan")
    n = P.sum(axis=1) - 1
    assert n[0] == 24 and n[1:64].max() < n[0]           # a slice wider than its neighbours
    _, _, _, _, P = _model("regular")
    assert (P.sum(axis=1)).max() == 13                   # 13 entries per row on a regular valence-6 mesh
    _, T, _, _, _ = _model("jittered")
    assert np.bincount(T.reshape(-1)).max() == 8


@pytest.mark.parametrize("name", list(bd.MESHES))
def test_matrix_against_numpy(name):
    from drake_amd import bending_matrix
    X, T, H, Q, P = _model(name)
    off, cols, vals = bending_matrix(X, T)
    n = len(X)
    assert off.shape == (n + 1,) and off[0] == 0 and off[-1] == len(cols) == len(vals)
    got, pat = np.zeros((n, n)), np.zeros((n, n), bool)
    for i in range(n):
        c = cols[off[i]:off[i + 1]]
        assert np.all(np.diff(c) > 0), "columns ascend"
        got[i, c] = vals[off[i]:off[i + 1]]
        pat[i, c] = True
    assert np.array_equal(pat, P), "pattern"
    scale = np.abs(Q).sum(axis=1)
    err = np.abs(got - Q).max(axis=1) if n else np.zeros(0)
    assert np.all(err <= 1e-12 * scale), float((err / np.maximum(scale, 1e-300)).max())
    assert np.all(np.abs(got.sum(axis=1)) <= 1e-12 * scale), "rows sum to zero"
    assert np.all(np.abs(got - got.T) <= 1e-12 * np.minimum(scale[:, None], scale[None, :]) + 0.0), "symmetric"
    if name == "triangle":
        assert len(cols) == 0


def test_matrix_refuses_a_zero_area_face():
    from drake_amd import MpmError, bending_matrix
    X, T = bd.mesh("regular")
    X = X.copy()
    a, b, c = T[7]
    X[c] = 0.5 * (X[a] + X[b])          # face 7 collapses onto its edge; it has interior edges
    with pytest.raises(MpmError) as e:
        bending_matrix(X, T)
    assert e.value.code == -1 and "face" in str(e.value) and "zero rest area" in str(e.value), e.value
    # a degenerate face without a hinge is nobody's business
    Xt = np.array([(0, 0, 0), (1, 0, 0), (2, 0, 0)], np.float32)
    off, cols, _ = bending_matrix(Xt, np.array([(0, 1, 2)], np.int32))
    assert len(cols) == 0 and off[-1] == 0
    with pytest.raises(MpmError):
        bending_matrix(Xt, np.array([(0, 1, 3)], np.int32))   # an index out of range


@pytest.mark.parametrize("name", ["jittered", "fan", "strip"])
def test_force_is_the_gradient_of_the_energy(name):
    X, T, H, Q, P = _model(name)
    x = bd.state("cylinder3", X).astype(np.float64)
    f = bd.force64(K, H, x)
    assert np.abs(f + K * Q @ x).max() <= 1e-9 * np.abs(f).max(), "hinge by hinge == through Q"
    eps = 1e-6
    g = np.zeros_like(x)
    for i in range(len(x)):
        for d in range(3):
            e = np.zeros_like(x)
            e[i, d] = eps
            g[i, d] = (bd.energy64(K, H, x + e) - bd.energy64(K, H, x - e)) / (2 * eps)
    assert np.abs(f + g).max() <= 1e-5 * np.abs(f).max(), float(np.abs(f + g).max() / np.abs(f).max())
    # total force and total torque vanish
    tot = np.abs(f).sum()
    assert np.abs(f.sum(axis=0)).max() <= 1e-12 * tot
    assert np.abs(np.cross(x - bd.CENTER, f).sum(axis=0)).max() <= 1e-12 * tot


@pytest.mark.parametrize("name", list(bd.MESHES))
def test_affine_images_have_no_force(name):
    X, T, H, Q, P = _model(name)
    x = bd.affine(X)
    B = bd.bound(K, H, x)
    f = bd.force64(K, H, x)
    # (float64 roundings of the restatement itself: a few 2^-53 of B_i)
    assert np.all(np.abs(f).max(axis=1) <= 64 * 2.0 ** -53 * B + 0.0)
    # and the bound means something: on the cylinder the force is far above 2^-24 B_i
    if H:
        xc = bd.state("cylinder3", X)
        assert np.abs(bd.force64(K, H, xc)).max() > 1e3 * bd.U * bd.bound(K, H, xc).max()


@pytest.mark.parametrize("name,st", PAIRS)
def test_float32_rows_stay_inside_the_bound(name, st):
    X, T, H, Q, P = _model(name)
    x32 = bd.state(st, X)
    f32 = bd.rows32(K, Q, P, x32)
    ref = bd.force64(float(np.float32(K)), H, x32)
    B, R = bd.bound(float(np.float32(K)), H, x32), bd.rounding_count(P)
    w = bd.margin(f32 - ref, B, R)
    print(f"bending float32 rows: {name} {st}: {w:.3g} of the bound, {bd.margin(f32 - ref, B, 1.0):.3g} of 2^-24 B_i")
    assert w <= 1.0, w
    # B_i dominates S_i = sum_j |k Q_ij| |x_j - x_i|
    x, kf = x32.astype(np.float64), float(np.float32(K))
    for i in range(len(x)):
        S = float(np.sum(np.abs(kf * Q[i]) * np.linalg.norm(x - x[i], axis=1)))
        assert S <= B[i] * (1 + 1e-9)
