"""Cloth FEM states in labelled constitutive regimes, and a float64 restatement of the constitutive chain that says which
branch every face of such a state takes.  Used by tests/test_fem_regimes.py (CPU) and tests/test_fem_regimes_gpu.py.

CalcFemStateAndForce (cuda_mpm_kernels.cuh:183-294; drake_amd/csrc/mpm_fem_face.inc) branches on the deformation of each
face: the return mapping (:146-181) on the normal stretch R[8] of the QR of the updated deformation gradient and on the
friction-cone test, the 2 x 2 polar decomposition and SVD (math_tools.cuh:512-597) on det, |S[1]|, tau and s1 < s2, the
Givens QR (math_tools.cuh:456-510) on q2 > 0.  A scene of flat sheets near their rest shape visits one side of each.  The
scenes made here are disconnected triangles (three vertices of their own per face, so that every vertex force comes from
one face), each given an in-plane map G (regimes I1 - I6) through its vertex positions and a target normal column
(r13, r23, r33) in the Q frame of its in-plane columns (regimes N1 - N5) through the uploaded deformation gradient and the
face particle's affine matrix C.

In-plane regimes (G: 2 x 2, in the triangle's plane):
  I1 near identity |G - I| < 1e-3    I2 stretch x1.2 - 2        I3 compression x0.3 - 0.8
  I4 shear, off-diagonal 0.1 - 0.6   I5 reflected, det G in [-1, -0.05]  I6 nearly flat, det G in [1e-3, 1e-2]
Normal regimes (r33 = R[8] of the QR that the return mapping sees):
  N1 r33 in [1.05, 1.5]: capped            N2 r33 in [0.3, 0.95], shear inside the friction cone (f < 0)
  N3 as N2, shear outside the cone (f > 0)  N4 r33 in [-1.5, -0.05]: clamped to >= -1, shear zeroed
  N5 r33 in [-1.5, 0.95], |r33| >= 0.05, gamma = 0: the first branch (capped at 1, below -1 left alone)

The restatement follows oracle/mpm_oracle.c operation by operation (its double build, libmpm_oracle_f64.so, is what it is
checked against): the material parameters cross into it as float32, gok = gamma / K is a float32 quotient, the Lame
parameters are formed in double.  It is vectorised over faces; 3 x 3 matrices are rows of 9 (row-major).

Two facts the branch statistics show and the tests rely on:
* Both diagonal entries R[0], R[4] of the Givens QR are >= 0 by construction (each rotation maps (a, b) to
  (a^2 + b^2) / sqrt(a^2 + b^2)), so the 2 x 2 block that reaches polar2 has det = R[0] R[4] - R[1] R[3] with R[3] the
  rounding residue of a zeroed entry: polar2's detA < 0 branch is reachable only when R[0] R[4] is itself at rounding
  level (a collinear triangle).  A reflected in-plane map (I5) reaches polar2 with a positive det all the same: how a
  triangle lies against its normal fibre is the sign of R[8], which the normal regimes set (N4, N5).
* svd2_rotation's branches (|S[1]| < 1e-5, the sign of tau, s1 < s2) choose between two factorisations whose U V^T is
  the same polar rotation: crossing one of them on the last bit of an input changes the stress by rounding only."""
import numpy as np

DT = 1e-3
BITS = 6
DX = 1.0 / (1 << BITS)
EPS32 = 2.0 ** -23

# I5 is a REFLECTED in-plane map (det G < 0).  In 3D a reflection of the plane followed by a rotation is another
# rotation, and the normal column is set apart from it, so the kernel does not see an inverted triangle there: it sees
# the same positive-det 2 x 2 block as for |G| (module docstring).  A face lying against its normal fibre is N4 / N5.
I_LABELS = ("I1", "I2", "I3", "I4", "I5", "I6")
N_LABELS = ("N1", "N2", "N3", "N4", "N5")

# (engine field name, value): materials (a) - (d) of the regimes; (a) is mpm_default_material / orc_default_params
DEFAULT = dict(youngs_modulus=4e5, poisson_ratio=0.3, density=2000.0, gamma=0.0, K=1e5, c_F=0.0)
MATERIALS = {
    "a": dict(DEFAULT),
    "b": dict(DEFAULT, gamma=40.0, K=2e5, c_F=15.0, youngs_modulus=2.5e5, poisson_ratio=0.22),
    "c": dict(DEFAULT, gamma=10.0, K=5e4, c_F=5.0, youngs_modulus=1e6, poisson_ratio=0.1),
    "d": dict(DEFAULT, gamma=40.0, K=2e5, c_F=1e-3, youngs_modulus=4e5, poisson_ratio=0.3),
}
# the normal regimes each material can produce: with gamma = 0 every face takes the return mapping's first branch; under
# (b) and (c) the cone's edge, c_F (1 - r33)^2 K / gamma, is 75000 (1 - r33)^2 and 25000 (1 - r33)^2: out of reach
N_OF = {"a": ("N1", "N5"), "b": ("N1", "N2", "N4"), "c": ("N1", "N2", "N4"), "d": ("N1", "N2", "N3", "N4")}
REL_BAND = 1e-4   # a face whose branch quantity lies within this relative distance of its threshold is excluded


def f32(x):
    return np.asarray(x, np.float32).astype(np.float64)


class Mat:
    """the material as the double oracle sees it: float32 fields, Lame parameters formed in double (mpm_oracle.c:114-117)"""

    def __init__(self, m):
        self.E, self.nu = float(np.float32(m["youngs_modulus"])), float(np.float32(m["poisson_ratio"]))
        self.gamma, self.K, self.cF = float(np.float32(m["gamma"])), float(np.float32(m["K"])), float(np.float32(m["c_F"]))
        self.mu = self.E / (2.0 * (1.0 + self.nu))
        # (E nu is a product of two floats, rounded to float before the double division)
        self.la = float(np.float32(self.E) * np.float32(self.nu)) / ((1.0 + self.nu) * (1.0 - 2.0 * self.nu))
        # (a float32 quotient in both builds of the oracle and in the engine)
        self.gok = float(np.float32(m["gamma"]) / np.float32(m["K"])) if self.gamma != 0.0 else 0.0


def oracle_material(o, m):
    """set an OracleMpm's parameters to material dict m"""
    from tests.helpers import _MATERIAL_FIELDS
    for k, v in m.items():
        setattr(o.p, _MATERIAL_FIELDS[k], v)


def engine_material(m):
    from drake_amd import GpuMpm
    gm = GpuMpm.default_material()
    for k, v in m.items():
        setattr(gm, k, v)
    return gm


def cloth_material(m):
    from drake_amd import ClothMaterial
    return ClothMaterial(*[float(m[f]) for f, _ in ClothMaterial._fields_])


# ---- float64 restatement (mpm_oracle.c, which cites cuda_mpm_kernels.cuh / math_tools.cuh) ------------------------
def givens_qr3(A, rnd=None):
    """QR of n 3 x 3 matrices by Givens rotations (mpm_oracle.c:181-216, math_tools.cuh:456-510): column by column,
    bottom row upwards.  -> Q, R (n, 9) and the three q2 = a^2 + b^2 with their scale (n, 3) each.
    rnd(a) (sensitivity only): a rounding applied to R and Q^T after every rotation"""
    A = np.asarray(A, np.float64).reshape(-1, 9)
    n = A.shape[0]
    R = A.copy()
    Qt = np.tile(np.eye(3).ravel(), (n, 1))
    q2s, q2scale = [], []
    for ri, rk, col in ((1, 2, 0), (0, 1, 0), (1, 2, 1)):
        a, b = R[:, ri * 3 + col].copy(), R[:, rk * 3 + col].copy()
        d = a * a + b * b
        sq = np.sqrt(d)
        ok = sq > 0.0
        with np.errstate(divide="ignore", invalid="ignore"):
            t = 1.0 / np.where(ok, sq, 1.0)
        c = np.where(ok, a * t, 1.0)
        s = np.where(ok, -b * t, 0.0)
        for M in (R, Qt):
            for j in range(3):
                t1, t2 = M[:, ri * 3 + j].copy(), M[:, rk * 3 + j].copy()
                M[:, ri * 3 + j] = c * t1 - s * t2
                M[:, rk * 3 + j] = s * t1 + c * t2
        if rnd is not None:
            R[:], Qt[:] = rnd(R), rnd(Qt)
        q2s.append(d)
        q2scale.append(np.sum(A[:, col::3] ** 2, axis=1))
    Q = Qt.reshape(n, 3, 3).transpose(0, 2, 1).reshape(n, 9)
    return Q, R, np.stack(q2s, 1), np.stack(q2scale, 1)


def _mm(a, b):      # c = a b, n 3 x 3 each, sums in index order from 0 (mpm_oracle.c:127-134)
    a, b = a.reshape(-1, 3, 3), b.reshape(-1, 3, 3)
    c = np.zeros_like(a)
    for j in range(3):
        c = c + a[:, :, j, None] * b[:, None, j, :]
    return c.reshape(-1, 9)


def _mmT(a, b):     # c = a b^T (mpm_oracle.c:136-143)
    return _mm(a, b.reshape(-1, 3, 3).transpose(0, 2, 1).reshape(-1, 9))


def polar2(A):
    """mpm_oracle.c:218-239 (math_tools.cuh:512-549): rotation U and symmetric S of n 2 x 2 matrices; and det A"""
    A = np.asarray(A, np.float64).reshape(-1, 4)
    a0, a1, a2, a3 = A.T
    detA = a0 * a3 - a1 * a2
    adet = np.abs(detA)
    neg = detA < 0.0
    B = np.stack([np.where(neg, a0 - a3, a0 + a3), np.where(neg, a1 + a2, a1 - a2),
                  np.where(neg, a2 + a1, a2 - a1), np.where(neg, a3 - a0, a3 + a0)], 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        k = 1.0 / np.sqrt(np.abs(B[:, 0] * B[:, 3] - B[:, 1] * B[:, 2]))
    U = B * k[:, None]
    s01 = (a0 * a1 + a2 * a3) * k
    S = np.stack([(a0 * a0 + a2 * a2 + adet) * k, s01, s01, (a1 * a1 + a3 * a3 + adet) * k], 1)
    zero = (a0 == 0) & (a1 == 0) & (a2 == 0) & (a3 == 0)
    U[zero] = (1.0, 0.0, 0.0, 1.0)
    S[zero] = A[zero]
    return U, S, detA


def svd2_rotation(A):
    """U V^T of the 2 x 2 SVD of mpm_oracle.c:241-265 (math_tools.cuh:551-597) and its branch quantities:
    dict(S1 = S[1], tao, s12 = s1 - s2, s_scale = max|S|, detA, det_scale = |A0 A3| + |A1 A2|)"""
    P, S, detA = polar2(A)
    small = np.abs(S[:, 1]) < 1e-5
    tao = 0.5 * (S[:, 0] - S[:, 3])
    w = np.sqrt(tao * tao + S[:, 1] * S[:, 1])
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(tao > 0.0, S[:, 1] / (tao + w), S[:, 1] / (tao - w))
        c = 1.0 / np.sqrt(t * t + 1.0)
    s = -t * c
    s1 = c * c * S[:, 0] - 2.0 * c * s * S[:, 1] + s * s * S[:, 3]
    s2 = s * s * S[:, 0] + 2.0 * c * s * S[:, 1] + c * c * S[:, 3]
    c, s = np.where(small, 1.0, c), np.where(small, 0.0, s)
    s1, s2 = np.where(small, S[:, 0], s1), np.where(small, S[:, 3], s2)
    sw = s1 < s2
    V = np.stack([np.where(sw, -s, c), np.where(sw, c, s), np.where(sw, -c, -s), np.where(sw, -s, c)], 1)
    U = np.stack([P[:, 0] * V[:, 0] + P[:, 1] * V[:, 2], P[:, 0] * V[:, 1] + P[:, 1] * V[:, 3],
                  P[:, 2] * V[:, 0] + P[:, 3] * V[:, 2], P[:, 2] * V[:, 1] + P[:, 3] * V[:, 3]], 1)
    R = np.stack([U[:, 0] * V[:, 0] + U[:, 1] * V[:, 1], U[:, 0] * V[:, 2] + U[:, 1] * V[:, 3],
                  U[:, 2] * V[:, 0] + U[:, 3] * V[:, 1], U[:, 2] * V[:, 2] + U[:, 3] * V[:, 3]], 1)
    A = np.asarray(A, np.float64).reshape(-1, 4)
    info = dict(S1=S[:, 1], tao=tao, s12=s1 - s2, s_scale=np.abs(S).max(axis=1), detA=detA,
                det_scale=np.abs(A[:, 0] * A[:, 3]) + np.abs(A[:, 1] * A[:, 2]), svd_small=small, swap=sw)
    return R, info


def pk1_2d(mat, F):
    """fixed-corotated PK1 of n 2 x 2 matrices (mpm_oracle.c:386-399, cuda_mpm_kernels.cuh:72-86)"""
    F = np.asarray(F, np.float64).reshape(-1, 4)
    R, info = svd2_rotation(F)
    J = F[:, 0] * F[:, 3] - F[:, 1] * F[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        di = 1.0 / J
    Fi = np.stack([F[:, 3] * di, -F[:, 1] * di, -F[:, 2] * di, F[:, 0] * di], 1)
    b = mat.la * (J - 1.0) * J
    P = np.stack([2.0 * mat.mu * (F[:, 0] - R[:, 0]) + b * Fi[:, 0], 2.0 * mat.mu * (F[:, 1] - R[:, 1]) + b * Fi[:, 2],
                  2.0 * mat.mu * (F[:, 2] - R[:, 2]) + b * Fi[:, 1], 2.0 * mat.mu * (F[:, 3] - R[:, 3]) + b * Fi[:, 3]], 1)
    return P, info


def inv33(m):
    """mpm_oracle.c:120-132 (math_tools.cuh:113-134)"""
    m = np.asarray(m, np.float64).reshape(-1, 9).T
    det = m[0] * (m[4] * m[8] - m[7] * m[5]) - m[3] * (m[1] * m[8] - m[7] * m[2]) + m[6] * (m[1] * m[5] - m[4] * m[2])
    with np.errstate(divide="ignore", invalid="ignore"):
        di = 1.0 / det
    o = [(m[4] * m[8] - m[5] * m[7]) * di, (m[2] * m[7] - m[1] * m[8]) * di, (m[1] * m[5] - m[2] * m[4]) * di,
         (m[5] * m[6] - m[3] * m[8]) * di, (m[0] * m[8] - m[2] * m[6]) * di, (m[2] * m[3] - m[0] * m[5]) * di,
         (m[3] * m[7] - m[4] * m[6]) * di, (m[1] * m[6] - m[0] * m[7]) * di, (m[0] * m[4] - m[1] * m[3]) * di]
    return np.stack(o, 1)


def project_strain(mat, F, rnd=None):
    """the return mapping of mpm_oracle.c:430-457 (cuda_mpm_kernels.cuh:146-181) -> projected F and
    dict(R8 (before the mapping), f, f_scale, q2, q2_scale, branch: 0 first / 1 R8 <= 0 / 2 inside / 3 cone return)"""
    F = np.asarray(F, np.float64).reshape(-1, 9)
    Q, R, q2, q2s = givens_qr3(F, rnd)
    R8 = R[:, 8].copy()
    rr = R[:, 2] * R[:, 2] + R[:, 5] * R[:, 5]
    zz = mat.cF * (R8 - 1.0) * (R8 - 1.0)
    f = (mat.gok * mat.gok) * rr - zz * zz
    first = np.full(R8.shape, mat.gamma == 0.0) | (R8 > 1.0)
    clamp = ~first & (R8 <= 0.0)
    cone = ~first & ~clamp & (f > 0.0)
    Rn = R.copy()
    Rn[first, 8] = np.minimum(R8[first], 1.0)
    Rn[first | clamp, 2] = 0.0
    Rn[first | clamp, 5] = 0.0
    Rn[clamp, 8] = np.maximum(R8[clamp], -1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = zz / (mat.gok * np.sqrt(rr))
    Rn[cone, 2] *= c[cone]
    Rn[cone, 5] *= c[cone]
    branch = np.where(first, 0, np.where(clamp, 1, np.where(cone, 3, 2)))
    info = dict(R8=R8, f=f, f_scale=(mat.gok * mat.gok) * rr + zz * zz, q2=q2, q2_scale=q2s, branch=branch)
    return _mm(Q, Rn), info


def cloth_dphi_dF(mat, F, rnd=None):
    """dPsi/dF of mpm_oracle.c:401-428 (cuda_mpm_kernels.cuh:88-144) -> P (n, 9) and the branch quantities of its
    QR and 2 x 2 SVD (svd2_rotation's dict plus R8, q2, q2_scale)"""
    F = np.asarray(F, np.float64).reshape(-1, 9)
    Q, R, q2, q2s = givens_qr3(F, rnd)
    P2, info = pk1_2d(mat, R[:, [0, 1, 3, 4]])
    if rnd is not None:
        P2 = rnd(P2)
    z = np.zeros(len(F))
    Pplane = _mm(Q, np.stack([P2[:, 0], P2[:, 1], z, P2[:, 2], P2[:, 3], z, z, z, z], 1))
    gp = mat.gamma
    fp = np.where(R[:, 8] < 1.0, -mat.K * (1.0 - R[:, 8]) * (1.0 - R[:, 8]), 0.0)
    A = np.zeros_like(R)
    A[:, 0] = gp * R[:, 2] * R[:, 2]
    A[:, 1] = gp * R[:, 2] * R[:, 5]
    A[:, 2] = gp * R[:, 8] * R[:, 2]
    A[:, 4] = gp * R[:, 5] * R[:, 5]
    A[:, 5] = gp * R[:, 8] * R[:, 8]
    A[:, 8] = fp * R[:, 8]
    A[:, 3], A[:, 6], A[:, 7] = A[:, 1], A[:, 2], A[:, 5]
    Ri = inv33(R) if rnd is None else rnd(inv33(R))
    Pn = _mmT(_mm(Q, A), Ri)
    info.update(R8=R[:, 8].copy(), q2=q2, q2_scale=q2s)
    return Pplane + Pn, info


# ---- the scene -------------------------------------------------------------------------------------------------------
def _rot3(rng, n):
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(n, 3, 3)


def _rot2(phi):
    c, s = np.cos(phi), np.sin(phi)
    return np.stack([np.stack([c, -s], -1), np.stack([s, c], -1)], -2)


def in_plane_map(rng, label, n):
    """n 2 x 2 maps G of in-plane regime `label`"""
    phi, psi = rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 2 * np.pi, n)
    Rp, Rq = _rot2(phi), _rot2(psi)
    diag = lambda a, b: np.stack([np.stack([a, 0 * a], -1), np.stack([0 * b, b], -1)], -2)
    if label == "I1":
        # half of them within the float32 resolution of the edges (|S[1]| < 1e-5 of svd2 for some), half up to 1e-3
        amp = np.where(np.arange(n) % 2 == 0, 1e-6, 3e-4)[:, None, None]
        return np.eye(2) + np.clip(rng.normal(size=(n, 2, 2)), -3, 3) * amp
    if label == "I2":
        return Rp @ diag(rng.uniform(1.2, 2.0, n), np.ones(n)) @ Rp.transpose(0, 2, 1)
    if label == "I3":
        return Rp @ diag(rng.uniform(0.3, 0.8, n), np.ones(n)) @ Rp.transpose(0, 2, 1)
    if label == "I4":
        sig = rng.uniform(0.1, 0.6, n) * rng.choice((-1.0, 1.0), n)
        up = rng.random(n) < 0.5
        G = np.tile(np.eye(2), (n, 1, 1))
        G[up, 0, 1] = sig[up]
        G[~up, 1, 0] = sig[~up]
        return Rp @ G @ Rp.transpose(0, 2, 1)
    a = rng.uniform(0.5, 1.5, n)
    if label == "I5":
        d = rng.uniform(0.05, 1.0, n)
        return Rp @ diag(a, -d / a) @ Rq
    if label == "I6":
        d = np.exp(rng.uniform(np.log(1e-3), np.log(1e-2), n))
        return Rp @ diag(a, d / a) @ Rq
    raise ValueError(label)


def normal_target(rng, label, n, mat):
    """n target columns (r13, r23, r33) of normal regime `label` under material `mat` (a Mat)"""
    alpha = rng.uniform(0, 2 * np.pi, n)
    logu = lambda lo, hi: np.exp(rng.uniform(np.log(lo), np.log(hi)))
    if label in ("N1", "N4", "N5"):
        r33 = {"N1": lambda: rng.uniform(1.05, 1.5, n), "N4": lambda: rng.uniform(-1.5, -0.05, n),
               "N5": lambda: np.where(rng.random(n) < 0.5, rng.uniform(-1.5, -0.05, n), rng.uniform(0.05, 0.95, n))}[label]()
        s = rng.uniform(0.0, 0.5, n)
    else:
        r33 = rng.uniform(0.3, 0.95, n) if label == "N2" else rng.uniform(0.45, 0.95, n)
        edge = mat.cF * (1.0 - r33) ** 2 / mat.gok          # |shear| at the cone's edge
        s = np.empty(n)
        for i in range(n):
            if label == "N2":
                s[i] = min(logu(0.1, 0.9) * edge[i], logu(0.01, 2.0))
            else:
                s[i] = logu(1.2 * edge[i], max(1.25 * edge[i], min(2.0, 4.0 * edge[i])))
    return np.stack([s * np.cos(alpha), s * np.sin(alpha), r33], 1)


class Scene:
    """n_per_cell disconnected triangles for every (I, N) cell that material key `mk` reaches, at random orientations
    and positions at least `margin` cells inside the walls of a 64^3 domain (x restricted to `xrange`, so that several
    scenes can share one domain).  Arrays in original order: vertices 3k, 3k + 1, 3k + 2 belong to face k."""

    def __init__(self, mk, n_per_cell=130, seed=0, xrange=(0.0, 1.0), margin=6):
        self.mk, self.m, self.mat = mk, MATERIALS[mk], Mat(MATERIALS[mk])
        rng = np.random.default_rng(seed)
        cells = [(i, nl) for i in I_LABELS for nl in N_OF[mk]]
        self.I = np.repeat([c[0] for c in cells], n_per_cell)
        self.N = np.repeat([c[1] for c in cells], n_per_cell)
        nf = self.nf = len(self.I)
        # rest triangles: edges of 0.3 - 0.5 dx at 50 - 130 degrees, randomly oriented
        L0, L1 = rng.uniform(0.3, 0.5, nf) * DX, rng.uniform(0.3, 0.5, nf) * DX
        th = rng.uniform(np.radians(50), np.radians(130), nf)
        E2 = np.stack([np.stack([L0, L1 * np.cos(th)], -1), np.stack([0 * L0, L1 * np.sin(th)], -1)], -2)  # columns: edges
        Rot = _rot3(rng, nf)
        lo, hi = margin * DX, 1.0 - margin * DX
        cen = rng.uniform(lo, hi, (nf, 3))
        cen[:, 0] = rng.uniform(max(lo, xrange[0] + 2 * DX), min(hi, xrange[1] - 2 * DX), nf)
        corners2 = np.stack([np.zeros((nf, 2)), E2[:, :, 0], E2[:, :, 1]], 1)          # (nf, 3, 2)
        corners2 -= corners2.mean(axis=1, keepdims=True)
        rest = cen[:, None, :] + np.einsum("fij,fcj->fci", Rot[:, :, :2], corners2)
        self.rest_pos = rest.reshape(-1, 3).astype(np.float32)
        self.indices = np.arange(3 * nf, dtype=np.int32).reshape(nf, 3)
        # deformation: x = c + Rd [G; 0] (rest corners in the rest plane), Rd a fresh rotation
        G = np.empty((nf, 2, 2))
        for lab in I_LABELS:
            k = self.I == lab
            G[k] = in_plane_map(rng, lab, int(k.sum()))
        self.G = G
        Rd = _rot3(rng, nf)
        self.def_pos = (cen[:, None, :] + np.einsum("fij,fcj->fci", Rd[:, :, :2], np.einsum("fij,fcj->fci", G, corners2))
                        ).reshape(-1, 3)
        self.r = np.empty((nf, 3))
        for lab in N_OF[mk]:
            k = self.N == lab
            self.r[k] = normal_target(rng, lab, int(k.sum()), self.mat)
        # velocities; the face particle's C with |dt C| ~ 1e-2, the vertices' ten times smaller
        self.vel = rng.uniform(-0.1, 0.1, (3 * nf, 3)).astype(np.float32)
        Cf = rng.normal(size=(nf, 9))
        self.C_face = (Cf * (1e-2 / DT) / np.abs(Cf).max(axis=1, keepdims=True)).astype(np.float32)
        self.C_vert = (rng.normal(size=(3 * nf, 9)) * (1e-3 / DT)).astype(np.float32).clip(-3e-3 / DT, 3e-3 / DT)

    def sheet(self):
        """(pos, vel, indices) for add_qr_cloth"""
        return self.rest_pos, self.vel, self.indices


def upload_F(x32, indices, DmInv, r, C_face):
    """F (nf, 9, float32) whose in-plane columns are the deformed edges of the faces times their Dm^-1 and whose normal
    column is (I + dt C)^-1 Q r, Q the (float64) Givens frame of the in-plane columns: the updated column that the
    return mapping sees is then Q r.  x32: vertex positions (float32), indices (nf, 3) into them."""
    X = f32(x32)[np.asarray(indices)]
    Dm = f32(DmInv)
    e0, e1 = X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]
    F = np.zeros((len(X), 9))
    F[:, 0::3] = e0 * Dm[:, 0, None]
    F[:, 1::3] = e0 * Dm[:, 1, None] + e1 * Dm[:, 3, None]
    Q, _, _, _ = givens_qr3(F)
    tgt = np.einsum("fij,fj->fi", Q.reshape(-1, 3, 3), r)
    M = np.eye(3) + DT * f32(C_face).reshape(-1, 3, 3)
    F[:, 2::3] = np.linalg.solve(M, tgt[:, :, None])[:, :, 0]
    return F.astype(np.float32)


def deformed_state(sc, DmInv):
    """The float32 arrays to upload for Scene `sc` after Finalize, given its faces' Dm^-1 (float32, (nf, 4)): vertex
    positions (3 nf, 3), face centroids and mean velocities (nf, 3), F (nf, 9) (upload_F)"""
    x = sc.def_pos.astype(np.float32)
    F32 = upload_F(x, sc.indices, DmInv, sc.r, sc.C_face)
    cen = ((f32(x).reshape(-1, 3, 3).sum(axis=1)) / 3.0).astype(np.float32)
    vmean = (f32(sc.vel).reshape(-1, 3, 3).sum(axis=1) / 3.0).astype(np.float32)
    return x, cen, vmean, F32


def updated_normal(F, C):
    """F with its normal column carried by the affine velocity field, (I + dt C) F[:, 2] (mpm_oracle.c:510-518,
    cuda_mpm_kernels.cuh:216-226), in double from the given values"""
    F, C = np.asarray(F, np.float64).reshape(-1, 9), np.asarray(C, np.float64).reshape(-1, 9)
    cF = F.copy()
    cF[:, 2] = (1.0 + DT * C[:, 0]) * F[:, 2] + DT * C[:, 1] * F[:, 5] + DT * C[:, 2] * F[:, 8]
    cF[:, 5] = DT * C[:, 3] * F[:, 2] + (1.0 + DT * C[:, 4]) * F[:, 5] + DT * C[:, 5] * F[:, 8]
    cF[:, 8] = DT * C[:, 6] * F[:, 2] + DT * C[:, 7] * F[:, 5] + (1.0 + DT * C[:, 8]) * F[:, 8]
    return cF


def in_plane(x, DmInv):
    """the in-plane columns of the faces, (x1 - x0, x2 - x0) Dm^-1 with Dm^-1[2] = 0 (mpm_oracle.c:522-529):
    x (nf, 3 corners, 3) -> (nf, 3 rows, 2 columns)"""
    X, Dm = np.asarray(x, np.float64), np.asarray(DmInv, np.float64)
    e0, e1 = X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]
    return np.stack([e0 * Dm[:, 0, None], e0 * Dm[:, 1, None] + e1 * Dm[:, 3, None]], 2)


def branch_quantities(sc, F32, x32, DmInv):
    """What decides every face's branches, from the float32 inputs (in double): the return mapping on
    (I + dt C) F, cloth_dphi_dF on [deformed edges Dm^-1 | projected normal column].  -> (dict of arrays, excluded mask)"""
    mat = sc.mat
    Fp, ps = project_strain(mat, updated_normal(F32, sc.C_face))
    ip = in_plane(f32(x32).reshape(-1, 3, 3), f32(DmInv))
    Fp[:, 0::3], Fp[:, 1::3] = ip[:, :, 0], ip[:, :, 1]
    _, ds = cloth_dphi_dF(mat, Fp)
    near = lambda x, t, scale: np.abs(x - t) <= REL_BAND * scale
    ex = np.zeros(sc.nf, bool)
    if mat.gamma != 0.0:
        ex |= near(ps["R8"], 1.0, 1.0) | near(ps["R8"], 0.0, 1.0)
        inner = (ps["R8"] > 0) & (ps["R8"] <= 1)
        ex |= inner & near(ps["f"], 0.0, ps["f_scale"])
    for d in (ps, ds):   # (|(a, b)| against the length of the column it is taken from)
        ex |= np.any(near(np.sqrt(d["q2"]), 0.0, np.sqrt(d["q2_scale"])), axis=1)
    ex |= near(ds["detA"], 0.0, ds["det_scale"])
    ex |= near(np.abs(ds["S1"]), 1e-5, 1e-5)
    # tau and s1 - s2 against w = sqrt(tau^2 + S[1]^2), half the distance of S's eigenvalues (|s1 - s2| = 2 w exactly)
    w = np.sqrt(ds["tao"] ** 2 + ds["S1"] ** 2)
    big = ~ds["svd_small"]
    ex |= big & (near(ds["tao"], 0.0, w) | near(ds["s12"], 0.0, 2.0 * w))
    q = dict(R8=ps["R8"], f=ps["f"], ps_branch=ps["branch"], detA=ds["detA"], S1=ds["S1"], tao=ds["tao"],
             s12=ds["s12"], svd_small=ds["svd_small"], swap=ds["swap"], R8_dphi=ds["R8"],
             q2_min=np.minimum(ps["q2"].min(axis=1), ds["q2"].min(axis=1)))
    return q, ex


# ---- putting the state in place ----------------------------------------------------------------------------------
def combined_state(parts, nf_total, nv_total):
    """parts: list of (Scene, first_face, first_vertex, DmInv of its faces).  -> particle arrays in original order
    (faces, then vertices): pos, vel, C; F (nf_total, 9); and per part (x32, F32) for branch_quantities"""
    n = nf_total + nv_total
    pos, vel, C = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32), np.zeros((n, 9), np.float32)
    F = np.zeros((nf_total, 9), np.float32)
    per = []
    for sc, ff, fv, Dm in parts:
        x, cen, vmean, F32 = deformed_state(sc, Dm)
        fs, vs = slice(ff, ff + sc.nf), slice(nf_total + fv, nf_total + fv + 3 * sc.nf)
        pos[fs], vel[fs], C[fs], F[fs] = cen, vmean, sc.C_face, F32
        pos[vs], vel[vs], C[vs] = x, sc.vel, sc.C_vert
        per.append((x, F32))
    return pos, vel, C, F, per


def set_oracle_state(o, pos, vel, C, F):
    """write original-order arrays into an OracleMpm by slot (o.pids)"""
    o.pos[:] = pos[o.pids]
    o.vel[:] = vel[o.pids]
    o.C[:] = C[o.pids]
    o.F[:] = F


def set_engine_state(g, pos, vel, C, F):
    from drake_amd import ARR
    pids = g.download(ARR.PIDS)
    g.upload_particle_state(pos[pids], vel[pids], C[pids], None, F)


def oracle_pair(sc):
    """float and double oracle holding Scene `sc` in its deformed state, re-sorted, ready for CalcFemStateAndForce;
    -> o32, o64, (x32, F32), branch quantities, excluded mask"""
    from oracle import oracle as orc
    from tests.helpers import oracle_copy
    o32 = orc.OracleMpm(BITS)
    oracle_material(o32, sc.m)
    o32.add_qr_cloth(*sc.sheet())
    o32.finalize()
    pos, vel, C, F, per = combined_state([(sc, 0, 0, o32.DmInv)], sc.nf, 3 * sc.nf)
    set_oracle_state(o32, pos, vel, C, F)
    o64 = oracle_copy(o32, np.float64)
    for o in (o32, o64):
        o.rebuild_mapping(True)
    q, ex = branch_quantities(sc, per[0][1], per[0][0], o32.DmInv)
    return o32, o64, per[0], q, ex


# ---- per-face fields ---------------------------------------------------------------------------------------------
FIELDS = ("F", "tau", "force", "x", "v")


def original_order(F, taus, forces, pos, vel, vol, pids):
    """CalcFemStateAndForce's outputs un-permuted to original particle order (float64)"""
    def un(a):
        o = np.empty(a.shape, np.float64)
        o[pids] = a
        return o
    return dict(F=np.asarray(F, np.float64), tau=un(taus), force=un(forces), x=un(pos), v=un(vel), vol=un(vol))


def of_oracle(o):
    return original_order(o.F, o.taus, o.forces, o.pos, o.vel, o.vol, o.pids)


def of_engine(g):
    from drake_amd import ARR as A
    return original_order(*(g.download(a) for a in (A.DEFORMATION_GRADIENTS, A.TAUS, A.FORCES, A.POSITIONS,
                                                      A.VELOCITIES, A.VOLUMES, A.PIDS)))


def face_view(orig, nf_total, ff=0, fv=0, nf=None):
    """per face of one scene (faces ff.., vertices fv.. of it): F (nf, 9), tau (nf, 9), force (nf, 3, 3: corner,
    component), face particle x, v (nf, 3), the corners' x, v (nf, 3, 3) and the face particle's volume"""
    nf = nf_total if nf is None else nf
    faces = slice(ff, ff + nf)
    verts = nf_total + fv + np.arange(3 * nf).reshape(nf, 3)
    return dict(F=orig["F"][faces], tau=orig["tau"][faces], force=orig["force"][verts], x=orig["x"][faces],
                v=orig["v"][faces], xc=orig["x"][verts], vc=orig["v"][verts], vol=orig["vol"][faces])


def face_scales(view64, E):
    """the natural size of every field of every face: max|F| for F; vol E max(1, |F|^2) for tau, over dx for the
    corner forces; the corners' max |x| and |v| for the face particle's centroid and mean velocity"""
    Fm = np.abs(view64["F"]).max(axis=1)
    t = view64["vol"] * E * np.maximum(1.0, Fm * Fm)
    return dict(F=Fm, tau=t, force=t / DX, x=np.abs(view64["xc"]).max(axis=(1, 2)),
                v=np.maximum(np.abs(view64["vc"]).max(axis=(1, 2)), 1e-30))


def face_errors(view, view64):
    """max over the components of |view - view64| per face and field"""
    out = {}
    for f in FIELDS:
        d = np.abs(np.asarray(view[f], np.float64) - view64[f])
        out[f] = d.reshape(d.shape[0], -1).max(axis=1)
    return out


def run_fem_copy(o, DmInv=None):
    """CalcFemStateAndForce on a copy of oracle o (o itself stays as it is); DmInv (nf, 4): the faces' Dm^-1 to use
    instead of the oracle's own (the engine's, so that both sides are given the same inputs)"""
    from tests.helpers import oracle_copy
    c = oracle_copy(o, o.real)
    if DmInv is not None:
        c.DmInv[:] = DmInv
    c.calc_fem_state_and_force(DT)
    return c


# ---- the whole face in double, and its sensitivity to the last bit of its inputs --------------------------------
def face64(mat, F, C, x, DmInv, vol, perturb=None):
    """CalcFemStateAndForce of n faces in double (mpm_oracle.c:495-566): F (uploaded, nf x 9), the face particle's C,
    corner positions x (nf, 3, 3), Dm^-1 (nf, 4), the face particle's volume.  -> the projected F, tau (nf, 9) and the
    corner forces (nf, 3 corners, 3).  perturb(a): one rounding of every computed stage -- the updated F, the projected F,
    the in-plane columns, R and Q^T after each Givens rotation, the 2 x 2 stress and R^-1 (the given inputs are exact
    floats; the deformed edges, differences of nearby floats, are exact too)."""
    p = perturb or (lambda a: a)
    Fp, _ = project_strain(mat, p(updated_normal(F, C)), perturb)
    Fp = p(Fp)
    ip = p(in_plane(x, DmInv))
    Fp[:, 0::3], Fp[:, 1::3] = ip[:, :, 0], ip[:, :, 1]
    P, _ = cloth_dphi_dF(mat, Fp, perturb)
    VP = (P * np.asarray(vol, np.float64)[:, None]).reshape(-1, 3, 3)
    tau = (VP[:, :, 2, None] * Fp.reshape(-1, 3, 3)[:, None, :, 2]).reshape(-1, 9)
    Dm = p(DmInv)
    DmiT = np.stack([np.stack([Dm[:, 0], Dm[:, 2]], -1), np.stack([Dm[:, 1], Dm[:, 3]], -1)], -2)
    gN = DmiT @ np.array([[-1.0, 1.0, 0.0], [-1.0, 0.0, 1.0]])
    G = VP[:, :, :2] @ gN                                   # (nf, 3 components, 3 corners)
    return dict(F=Fp, tau=tau, force=-G.transpose(0, 2, 1))


SENS_DRAWS = 16


def sensitivity(mat, F, C, x, DmInv, vol, seed=0):
    """How far a float evaluation of each face may land from the double one for no other reason than that the inputs of
    its stages are rounded to float: the largest change of every field (max over components) over SENS_DRAWS draws of
    independent perturbations of every component of every stage (face64) by +-2^-24 of the largest entry of that
    matrix, in double.  (Normwise, not entrywise: an entry that a rotation zeroes -- R[3], and R[2], R[5] after the
    return mapping -- keeps a rounding residue of the size of its column, and R^-1 carries it divided by R[4].)  Where the face is ill-conditioned (the normal of a nearly flat triangle, R^-1 with R[4] ~ 1e-3)
    this is many ulps of its natural size, and one float evaluation's distance from double is just one draw of it."""
    rng = np.random.default_rng(seed)
    ref = face64(mat, F, C, x, DmInv, vol)
    out = {f: np.zeros(len(ref["F"])) for f in ref}
    for _ in range(SENS_DRAWS):
        def pert(a):
            a = np.asarray(a, np.float64)
            size = np.abs(a.reshape(len(a), -1)).max(axis=1).reshape((-1,) + (1,) * (a.ndim - 1))
            return a + rng.choice((-1.0, 1.0), a.shape) * 2.0 ** -24 * size
        d = face64(mat, F, C, x, DmInv, vol, pert)
        for f in ref:
            out[f] = np.maximum(out[f], np.abs(d[f] - ref[f]).reshape(len(ref[f]), -1).max(axis=1))
    return out
