"""Shell bending about a curved rest shape (mpm_set_shell_bending; drake_amd/csrc/mpm_shell.h) on the CPU: the model
restated in numpy float64 from its definition, independently of the product -- hinges from an edge map, the dihedral
angle by arctan2, psi = 2 sin(theta / 2), forces by the gradient of theta --, a float32 restatement of the engine's hinge
function and gather, the meshes and states of the tests, and their bound.

The model.  Every edge shared by exactly two faces is a hinge (x0, x1 | x2, x3): x0 -> x1 as face A (the lower id) runs
the edge, x2 opposite it in A, x3 in B; hinges in ascending (min(v0, v1), max(v0, v1)).  e = x1 - x0, a = x2 - x0,
b = x3 - x0, nA = e x a, nB = b x e, theta = atan2(e^ . (nA x nB), nA . nB),
    E_h = 1/2 k cbar (psi - psibar)^2,  cbar = 3 |ebar|^2 / (Abar_A + Abar_B),  f_j = -k cbar (psi - psibar) cos(theta / 2) G_j,
    G2 = -|e| nA / |nA|^2,  G3 = -|e| nB / |nB|^2,  G0 = -(((x1 - x2) . e / |e|^2) G2 + ((x1 - x3) . e / |e|^2) G3),
    G1 = -(((x2 - x0) . e / |e|^2) G2 + ((x3 - x0) . e / |e|^2) G3).

The bound.  B_i = sum_{h contains i} |kc_h| |G_hi| (kappa_hA + kappa_hB) (1 + |psi_h| + |psibar_h|), kappa_hA =
|e| |a| / |nA|, kappa_hB = |e| |b| / |nB| the conditioning of the two normals.  The engine's force must lie within
R_i 2^-24 B_i of the float64 force of the float positions, R_i = R + n_i: R = 46 counted from shell_hinge in mpm_shell.h
(psi 12.75, dpsi 7, the scalar 1, G2 / G3 18, the record 0.5, the corners 0 and 1 another 6, second order 0.75), n_i the
records the row adds.  psi itself within 13 (kappa_A + kappa_B) (1 + |psi|) 2^-24.  R is a count, not a fit:
tests/test_shell_bending.py pushes the float32 restatement below through the same bound on every mesh and state; its
worst is 0.0086 of the bound (the book, affine), psi's worst 0.072 of its bound (the jittered sheet, rigid); one hinge's
records alone, from the host compile mpm_shell_hinge, reach 0.13 of R 2^-24 of their unit (the jittered sheet, perturbed)."""
import math

import numpy as np

from tests import bending as bd
from tests import pressure as pr

U = 2.0 ** -24
H0 = bd.H0
R_SHELL = 46.0
R_PSI = 13.0
GATE = 1e-30
K = 1e-6                       # N m, the stiffness of the tests
REST_SHAPE, REST_FLAT = 0, 1
CENTER = bd.CENTER


# ---- meshes: (X float32 as added, T int32, rest_pos float32 or None) ---------------------------------------------------
def tube(around=12, along=5, radius=2 * H0, h=H0):
    """an open tube about an axis parallel to y: boundary edges at both ends, psibar of one sign around"""
    X = []
    for j in range(along):
        for i in range(around):
            a = 2 * math.pi * i / around
            X.append((radius * math.cos(a), (j - 0.5 * (along - 1)) * h, radius * math.sin(a)))
    v = lambda j, i: j * around + i % around   # noqa: E731
    T = []
    for j in range(along - 1):
        for i in range(around):
            T += [(v(j, i), v(j + 1, i), v(j + 1, i + 1)), (v(j, i), v(j + 1, i + 1), v(j, i + 1))]
    return (np.array(X) + CENTER).astype(np.float32), np.array(T, np.int32)


def fold(X, angle=1.0):
    """the part of a sheet beyond the plane x = CENTER[0] turned by `angle` about the line x = CENTER[0], z = its z
    (float64)"""
    X = np.asarray(X, np.float64).copy()
    z0 = X[:, 2].mean()
    far = X[:, 0] > CENTER[0] + 1e-9
    u = X[far, 0] - CENTER[0]
    X[far, 0] = CENTER[0] + u * math.cos(angle)
    X[far, 2] = z0 + u * math.sin(angle)
    return X


def _book():
    X, T = bd.sheet(5, 5)
    return X, T, fold(X).astype(np.float32)


MESHES = {
    "strip": lambda: bd.mesh("strip") + (None,),
    "fan": lambda: bd.mesh("fan") + (None,),
    "jittered": lambda: bd.mesh("jittered") + (None,),
    "triangle": lambda: bd.mesh("triangle") + (None,),
    "icosphere1": lambda: pr.icosphere(CENTER, 3 * H0, subdivisions=1) + (None,),     # 42 vertices
    "icosphere2": lambda: pr.icosphere(CENTER, 4 * H0, subdivisions=2) + (None,),     # 162: three slices, valence 5 and 6
    "tube": lambda: tube() + (None,),
    "book": _book,
}
_MESH = {}


def mesh(name):
    if name not in _MESH:
        _MESH[name] = MESHES[name]()
    return _MESH[name]


def rest_shape(name):
    X, T, rest = mesh(name)
    return X if rest is None else rest


# ---- states: current float64 positions from the rest shape ---------------------------------------------------------------
def rigid(X, seed=4):
    r = np.random.default_rng(seed)
    Q = np.linalg.qr(r.normal(size=(3, 3)))[0]
    Q *= np.sign(np.linalg.det(Q))
    return (np.asarray(X, np.float64) - CENTER) @ Q.T + CENTER + np.array([0.02, -0.01, 0.03])


def folded(X, theta):
    """the strip with its one hinge at the dihedral angle theta: vertex 3 turned about the edge (1, 2)"""
    X = np.asarray(X, np.float64).copy()
    x0, x1 = X[1], X[2]                      # face A = (0, 1, 2) runs the edge 1 -> 2
    e = (x1 - x0) / np.linalg.norm(x1 - x0)
    b = X[3] - x0
    par, perp = e * (b @ e), b - e * (b @ e)
    X[3] = x0 + par + perp * math.cos(theta) + np.cross(e, perp) * math.sin(theta)
    return X


def collinear(X):
    """the strip with x2 of its hinge (vertex 0) moved onto the edge, at x0 (vertex 1): nA is an exact zero"""
    X = np.asarray(X, np.float64).copy()
    X[0] = X[1]
    return X


STATES = {
    "rest": lambda X: np.asarray(X, np.float64).copy(),
    "rigid": rigid,
    "perturbed": lambda X: bd.perturbed(X, seed=3),
    "affine": lambda X: bd.affine(X, seed=2),
}
STRIP_STATES = {
    "folded+": lambda X: folded(X, 3.1),
    "folded-": lambda X: folded(X, -3.1),
    "collinear": collinear,
}
CASES = [(m, s) for m in MESHES for s in STATES] + [("strip", s) for s in STRIP_STATES]


def state(name, st):
    """float32 positions of mesh `name` in state `st`"""
    X = rest_shape(name)
    x = (STATES.get(st) or STRIP_STATES[st])(X)
    assert x.min() > 0.1 and x.max() < 0.9
    return x.astype(np.float32)


# ---- the model in float64 --------------------------------------------------------------------------------------------------
def hinges(T):
    """(n, 4) int: x0, x1 | x2, x3 of every edge with exactly two faces, in ascending (min, max)"""
    E = {}
    for t, (a, b, c) in enumerate(np.asarray(T).reshape(-1, 3)):
        for u, v, w in ((a, b, c), (b, c, a), (c, a, b)):
            E.setdefault((min(int(u), int(v)), max(int(u), int(v))), []).append((t, int(u), int(v), int(w)))
    H = []
    for key, faces in sorted(E.items()):
        if len(faces) != 2 or key[0] == key[1]:
            continue
        (_, u, v, w2), (_, _, _, w3) = sorted(faces)
        H.append((u, v, w2, w3))
    return np.array(H, np.int64).reshape(-1, 4)


def _geometry(x, H):
    x = np.asarray(x, np.float64)
    x0, x1, x2, x3 = (x[H[:, j]] for j in range(4))
    e, a, b = x1 - x0, x2 - x0, x3 - x0
    return x0, x1, x2, x3, e, a, b, np.cross(e, a), np.cross(b, e)


def theta64(x, H):
    _, _, _, _, e, _, _, nA, nB = _geometry(x, H)
    eh = e / np.linalg.norm(e, axis=1)[:, None]
    return np.arctan2((eh * np.cross(nA, nB)).sum(axis=1), (nA * nB).sum(axis=1))


def active(x32, H):
    """the gate on the float differences, as the engine decides it (products and sums in float32)"""
    x = np.asarray(x32, np.float32)
    e, a, b = x[H[:, 1]] - x[H[:, 0]], x[H[:, 2]] - x[H[:, 0]], x[H[:, 3]] - x[H[:, 0]]
    nA, nB = _cross32(e, a), _cross32(b, e)
    return (_dot32(e, e) >= np.float32(GATE)) & (_dot32(nA, nA) >= np.float32(GATE)) & (_dot32(nB, nB) >= np.float32(GATE))


def psi64(x, H):
    return 2.0 * np.sin(0.5 * theta64(x, H))


def cbar64(X_rest, H):
    _, _, _, _, e, _, _, nA, nB = _geometry(X_rest, H)
    return 3.0 * (e * e).sum(axis=1) / (0.5 * np.linalg.norm(nA, axis=1) + 0.5 * np.linalg.norm(nB, axis=1))


def grad_theta64(x, H):
    """G (n, 4, 3)"""
    x0, x1, x2, x3, e, _, _, nA, nB = _geometry(x, H)
    le, ee = np.linalg.norm(e, axis=1), (e * e).sum(axis=1)
    G2 = -(le / (nA * nA).sum(axis=1))[:, None] * nA
    G3 = -(le / (nB * nB).sum(axis=1))[:, None] * nB
    w = lambda p: ((p * e).sum(axis=1) / ee)[:, None]   # noqa: E731
    G0 = -(w(x1 - x2) * G2 + w(x1 - x3) * G3)
    G1 = -(w(x2 - x0) * G2 + w(x3 - x0) * G3)
    return np.stack([G0, G1, G2, G3], axis=1)


def hinge_forces64(x, H, kc, psibar, act=None):
    """the corner records (n, 4, 3) and psi (n,); hinges with act False give zeros"""
    if len(H) == 0:
        return np.zeros((0, 4, 3)), np.zeros(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        th = theta64(x, H)
        psi = 2.0 * np.sin(0.5 * th)
        rec = (-np.asarray(kc, np.float64) * (psi - np.asarray(psibar, np.float64)) * np.cos(0.5 * th))[:, None, None] * grad_theta64(x, H)
    if act is not None:
        rec[~act], psi[~act] = 0.0, 0.0
    return rec, psi


def force64(x, H, kc, psibar, act=None):
    rec, _ = hinge_forces64(x, H, kc, psibar, act)
    f = np.zeros((len(x), 3))
    for j in range(4):
        np.add.at(f, H[:, j], rec[:, j])
    return f


def energy64(x, H, kc, psibar, act=None):
    """per hinge (n,)"""
    if len(H) == 0:
        return np.zeros(0)
    with np.errstate(invalid="ignore"):
        E = 0.5 * np.asarray(kc, np.float64) * (psi64(x, H) - np.asarray(psibar, np.float64)) ** 2
    if act is not None:
        E[~act] = 0.0
    return E


def kappas(x, H):
    _, _, _, _, e, a, b, nA, nB = _geometry(x, H)
    n = lambda q: np.linalg.norm(q, axis=1)   # noqa: E731
    with np.errstate(divide="ignore", invalid="ignore"):
        return n(e) * n(a) / n(nA), n(e) * n(b) / n(nB)


def bound(x, H, kc, psibar, act=None):
    """(B_i (n_verts,), n_i (n_verts,) the records per vertex, psi's bound per hinge without its R)"""
    nv = len(x)
    B, N = np.zeros(nv), np.zeros(nv)
    if len(H) == 0:
        return B, N, np.zeros(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        kA, kB = kappas(x, H)
        psi = psi64(x, H)
        G = np.linalg.norm(grad_theta64(x, H), axis=2)
        unit = np.abs(np.asarray(kc, np.float64))[:, None] * G * ((kA + kB) * (1.0 + np.abs(psi) + np.abs(np.asarray(psibar, np.float64))))[:, None]
        pb = (kA + kB) * (1.0 + np.abs(psi))
    if act is not None:
        unit[~act], pb[~act] = 0.0, 0.0
    for j in range(4):
        np.add.at(B, H[:, j], unit[:, j])
        np.add.at(N, H[:, j], 1.0)
    return B, N, pb


def margin(err, B, R):
    """the worst |err| / (R 2^-24 B) over the vertices (0 where the error vanishes)"""
    e = np.abs(np.asarray(err, np.float64))
    e = e.max(axis=1) if e.ndim == 2 else e
    b = R * U * B
    w = np.where(e == 0, 0.0, e / np.maximum(b, 1e-300))
    return float(w.max()) if len(w) else 0.0


def energy_bound(x, H, kc, psibar, act=None):
    """per hinge: the float term 1/2 kc (psi - psibar)^2 against float64 -- psi's error d = 13 (kappa_A + kappa_B)
    (1 + |psi|) 2^-24 and one rounding of the difference enter as kc (|psi - psibar| d' + d'^2 / 2), d' = d + 2^-24
    (|psi| + |psibar|); the three products round E itself: 3 2^-24 E (4 allowed)"""
    if len(H) == 0:
        return np.zeros(0)
    _, _, pb = bound(x, H, kc, psibar, act)
    with np.errstate(invalid="ignore"):
        psi = np.nan_to_num(psi64(x, H))
    pbar, kc = np.asarray(psibar, np.float64), np.abs(np.asarray(kc, np.float64))
    d = R_PSI * U * pb + U * (np.abs(psi) + np.abs(pbar))
    return kc * (np.abs(psi - pbar) * d + 0.5 * d * d) + 4 * U * 0.5 * kc * (psi - pbar) ** 2


# ---- the engine's arithmetic restated in float32 ---------------------------------------------------------------------------
F = np.float32


def _cross32(u, v):
    u, v = np.asarray(u, F), np.asarray(v, F)
    return np.stack([u[..., 1] * v[..., 2] - u[..., 2] * v[..., 1], u[..., 2] * v[..., 0] - u[..., 0] * v[..., 2],
                     u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]], axis=-1)


def _dot32(u, v):
    u, v = np.asarray(u, F), np.asarray(v, F)
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def hinges32(x32, H, kc, psibar):
    """shell_hinge on every hinge, operation by operation in float32 (numpy rounds every operation once; nothing is
    contracted): (records (n, 4, 3) float32, psi (n,) float32, acts (n,) bool)"""
    x = np.asarray(x32, F)
    kc, psibar = np.asarray(kc, F), np.asarray(psibar, F)
    if len(H) == 0:
        return np.zeros((0, 4, 3), F), np.zeros(0, F), np.zeros(0, bool)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        e, a, b = x[H[:, 1]] - x[H[:, 0]], x[H[:, 2]] - x[H[:, 0]], x[H[:, 3]] - x[H[:, 0]]
        nA, nB = _cross32(e, a), _cross32(b, e)
        ee, AA, BB = _dot32(e, e), _dot32(nA, nA), _dot32(nB, nB)
        on = (ee >= F(GATE)) & (AA >= F(GATE)) & (BB >= F(GATE))
        le, lA, lB = np.sqrt(ee), np.sqrt(AA), np.sqrt(BB)
        rA, rB = F(1) / lA, F(1) / lB
        hA, hB = nA * rA[:, None], nB * rB[:, None]
        d, s = hA - hB, hA + hB
        t = _dot32(e, _cross32(nA, nB))
        mag = np.sqrt(_dot32(d, d))
        psi = np.where(t >= 0, mag, -mag).astype(F)
        dpsi = F(0.5) * np.sqrt(_dot32(s, s))
        m = -(kc * (psi - psibar)) * dpsi
        gA, gB = le / AA, le / BB
        re = F(1) / ee
        wA, wB = _dot32(a, e) * re, _dot32(b, e) * re
        uA, uB = F(1) - wA, F(1) - wB
        f2 = m[:, None] * -(gA[:, None] * nA)
        f3 = m[:, None] * -(gB[:, None] * nB)
        f1 = -(wA[:, None] * f2 + wB[:, None] * f3)
        f0 = -(uA[:, None] * f2 + uB[:, None] * f3)
    rec = np.stack([f0, f1, f2, f3], axis=1).astype(F)
    rec[~on], psi[~on] = 0, 0
    return rec, psi, on


def gather32(rec, H, n_verts):
    """a vertex's records added in ascending hinge id, in float32, from zero"""
    f = np.zeros((n_verts, 3), F)
    for h in range(len(H)):
        for j in range(4):
            f[H[h, j]] = f[H[h, j]] + rec[h, j]
    return f


def energy_terms32(psi, kc, psibar):
    d = np.asarray(psi, F) - np.asarray(psibar, F)
    return (F(0.5) * np.asarray(kc, F)) * (d * d)


# ---- the rest quantities of a mesh as the engine forms them ----------------------------------------------------------------
def rest_table(name, k=K, rest=REST_SHAPE):
    """(H, kc float32 = float32(float64(k32) cbar), psibar float32: shell_hinge's psi on the rest positions, restated)"""
    X, T, given = mesh(name)
    H = hinges(T)
    shape = X if (given is None or rest == REST_FLAT) else given
    kc = (float(F(k)) * cbar64(shape.astype(np.float64), H)).astype(F) if len(H) else np.zeros(0, F)
    if rest == REST_FLAT:
        return H, kc, np.zeros(len(H), F)
    return H, kc, hinges32(shape, H, kc, np.zeros(len(H), F))[1]


def max_stable_dt(X_rest, H, kc, mass, flat=False):
    """2 / sqrt(max_i (1 / m_i) sum_h kc cos^2(thetabar / 2) |G_hi| sum_j |G_hj|) at the rest shape"""
    if len(H) == 0:
        return np.inf
    G = np.linalg.norm(grad_theta64(X_rest, H), axis=2)
    c2 = np.ones(len(H)) if flat else np.cos(0.5 * theta64(X_rest, H)) ** 2
    S = np.zeros(len(X_rest))
    for j in range(4):
        np.add.at(S, H[:, j], np.asarray(kc, np.float64) * c2 * G[:, j] * G.sum(axis=1))
    w2 = float(np.max(S / np.asarray(mass, np.float64)))
    return 2.0 / math.sqrt(w2) if w2 > 0 else np.inf


# ---- the gather table, restated ----------------------------------------------------------------------------------------------
PAD = 0xFFFFFFFF


def table_layout(H, row_vertex, nf, slice_=64):
    """(row_pid, slice_off, ent) as shell_rows lays them out: one row per vertex of row_vertex (ascending), its records
    hinge << 2 | corner in ascending hinge id, padding 0xFFFFFFFF, slices of `slice_` rows stored column-major"""
    row_of = {int(v): r for r, v in enumerate(row_vertex)}
    rows = [[] for _ in row_vertex]
    for h in range(len(H)):
        for j in range(4):
            rows[row_of[int(H[h, j])]].append(h << 2 | j)
    n = len(rows)
    slice_off, out = [0], []
    for s in range((n + slice_ - 1) // slice_):
        lo, hi = s * slice_, min(n, (s + 1) * slice_)
        width = max(len(r) for r in rows[lo:hi])
        block = np.full((width, slice_), PAD, np.int64)
        for lane in range(hi - lo):
            block[:len(rows[lo + lane]), lane] = rows[lo + lane]
        out.append(block.reshape(-1))
        slice_off.append(slice_off[-1] + width * slice_)
    ent = np.concatenate(out) if out else np.zeros(0, np.int64)
    return np.array([nf + int(v) for v in row_vertex], np.int64), np.array(slice_off, np.int64), ent
