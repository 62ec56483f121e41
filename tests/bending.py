"""Bending stiffness of the cloth (mpm_set_bending; drake_amd/csrc/mpm_bending.h) on the CPU: the model restated in
numpy float64 from its definition, independently of the product -- hinges from an edge map, cotangents of the rest
angles --, a float32 restatement of the engine's row evaluation, the meshes and states of the tests, and their bound.

The model (Bergou et al. 2006, Wardetzky et al. 2007; flat rest shape): every interior edge x0 x1 shared by exactly two
faces is a hinge (x0, x1 | x2, x3), x2 opposite the edge in face A, x3 in face B; a0, a1 the rest angles of A at x0, x1,
b0, b1 those of B;
    K = (cot a1 + cot b1, cot a0 + cot b0, -(cot a0 + cot a1), -(cot b0 + cot b1)),   c = 3 / (A_A + A_B),
    E = 1/2 k sum_h c_h |sum_j K_hj x_j|^2 = 1/2 x^T (k Q) x,   f = -k Q x.

The bound.  B_i = k sum_{h contains i} c_h |K_hi| (sum_j |K_hj|) d_h, d_h the largest distance between two of the
hinge's four current vertices.  Because sum_j K_hj = 0, the hinge's term sum_j K_hj x_j equals sum_j K_hj (x_j - y) for
any y, so B_i dominates S_i = sum_j |k Q_ij| |x_j - x_i| whichever vertex an implementation differences against.  The
engine's force must lie within R_i 2^-24 B_i of the float64 force of the float positions, with R_i counted from k_bend
(mpm_bending.h) for a row of n_i off-diagonal entries, first order, in units of 2^-24 S_i:
    the coefficient float(k Q_ij)                        1
    the difference x_j - x_i                             1
    one fused multiply-add per entry: n_i roundings of partial sums, each at most S_i      n_i
    second-order terms                                   1 (generous)
R_i = n_i + 3.  It is a rounding bound, not a fit: tests/test_bending.py pushes the float32 restatement below through the
same bound on every mesh and state (its worst is 0.41 of 2^-24 B_i, on the strip on the wide cylinder; 0.23 on the
jittered sheet on the tight one)."""
import numpy as np

U = 2.0 ** -24
H0 = 1.0 / 128          # the spacing of the test sheets: half a cell at domain_bits 6, a quarter at 5
CENTER = np.array([0.5, 0.5, 0.5])


# ---- meshes (float32 rest positions in the plane z = const, int32 triangles) ------------------------------------------
def sheet(n, m, h=H0, alternate=False, jitter=0.0, seed=0):
    """n x m vertices, spacing h; alternate: the diagonal of a quad flips with the parity of (i + j)"""
    r = np.random.default_rng(seed)
    X = np.zeros((n * m, 3))
    for i in range(n):
        for j in range(m):
            X[i * m + j, :2] = (i * h, j * h)
    X[:, :2] += r.uniform(-jitter, jitter, (n * m, 2)) * h
    T = []
    for i in range(n - 1):
        for j in range(m - 1):
            a, b, c, d = i * m + j, (i + 1) * m + j, (i + 1) * m + j + 1, i * m + j + 1
            T += [(a, b, c), (a, c, d)] if (not alternate or (i + j) % 2) else [(a, b, d), (b, c, d)]
    return _centered(X), np.array(T, np.int32)


def fan(spokes=12, rings=6, h=H0):
    """a hub with `spokes` faces and `rings` rings around it: 1 + spokes * rings vertices, the hub's row far longer
    than any other of its slice of 64 rows, and a second slice behind it"""
    X = [(0.0, 0.0, 0.0)]
    for r in range(1, rings + 1):
        for s in range(spokes):
            a = 2 * np.pi * (s + 0.5 * (r % 2)) / spokes
            X.append((r * h * np.cos(a), r * h * np.sin(a), 0.0))
    v = lambda r, s: 1 + (r - 1) * spokes + s % spokes   # noqa: E731
    T = [(0, v(1, s), v(1, s + 1)) for s in range(spokes)]
    for r in range(1, rings):
        o = r % 2   # ring r + 1 is turned by half a spoke against ring r
        for s in range(spokes):
            if o:
                T += [(v(r, s), v(r + 1, s), v(r, s + 1)), (v(r, s + 1), v(r + 1, s), v(r + 1, s + 1))]
            else:
                T += [(v(r, s), v(r + 1, s), v(r + 1, s + 1)), (v(r, s), v(r + 1, s + 1), v(r, s + 1))]
    return _centered(np.array(X)), np.array(T, np.int32)


def _centered(X):
    X = np.asarray(X, np.float64)
    X = X - 0.5 * (X.min(axis=0) + X.max(axis=0)) + CENTER
    return X.astype(np.float32)


def strip():
    X = np.array([(0, 0, 0), (1, 0, 0), (0.4, 1, 0), (1.5, 0.9, 0)], np.float64) * H0
    return _centered(X), np.array([(0, 1, 2), (1, 3, 2)], np.int32)


def triangle():
    X = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0)], np.float64) * H0
    return _centered(X), np.array([(0, 1, 2)], np.int32)


MESHES = {
    "jittered": lambda: sheet(9, 8, alternate=True, jitter=0.25, seed=1),
    "regular": lambda: sheet(13, 13),
    "fan": fan,
    "strip": strip,
    "triangle": triangle,
}
_MESH = {}


def mesh(name):
    if name not in _MESH:
        _MESH[name] = MESHES[name]()
    return _MESH[name]


# ---- states: current float32 positions from the rest positions --------------------------------------------------------
def cylinder(X, radius):
    """isometric wrap about an axis parallel to y: arc length along x is kept"""
    X = np.asarray(X, np.float64)
    u = X[:, 0] - CENTER[0]
    return np.stack([CENTER[0] + radius * np.sin(u / radius), X[:, 1], X[:, 2] + radius * (1.0 - np.cos(u / radius))], 1)


def affine(X, seed=2):
    """a random affine map: rotation x stretch (0.8 .. 1.2), about the centre, with a shift"""
    r = np.random.default_rng(seed)
    A = np.linalg.qr(r.normal(size=(3, 3)))[0] @ np.diag([1.2, 0.8, 1.0]) @ np.linalg.qr(r.normal(size=(3, 3)))[0]
    return (np.asarray(X, np.float64) - CENTER) @ A.T + CENTER + np.array([0.01, -0.02, 0.015])


def perturbed(X, seed=3):
    return np.asarray(X, np.float64) + 0.1 * H0 * np.random.default_rng(seed).normal(size=np.shape(X))


STATES = {
    "affine": affine,
    "cylinder3": lambda X: cylinder(X, 3 * H0),
    "cylinder30": lambda X: cylinder(X, 30 * H0),
    "perturbed": perturbed,
}


def state(name, X):
    return STATES[name](X).astype(np.float32)


# ---- the model in float64 ---------------------------------------------------------------------------------------------
def _cot(a, b, c):
    u, v = b - a, c - a
    return float(u @ v) / float(np.linalg.norm(np.cross(u, v)))


def hinges(X, T):
    """[((x0, x1, x2, x3), K (4,), c)] from the rest positions X and triangles T, sorted by edge"""
    X = np.asarray(X, np.float64)
    E = {}
    for t, (a, b, c) in enumerate(np.asarray(T).reshape(-1, 3)):
        for u, v, w in ((a, b, c), (b, c, a), (c, a, b)):
            E.setdefault((min(u, v), max(u, v)), []).append((t, int(w)))
    H = []
    for (u, v), faces in sorted(E.items()):
        if len(faces) != 2:
            continue
        w2, w3 = faces[0][1], faces[1][1]
        area = [0.5 * np.linalg.norm(np.cross(X[T[t][1]] - X[T[t][0]], X[T[t][2]] - X[T[t][0]])) for t, _ in faces]
        a0, a1 = _cot(X[u], X[v], X[w2]), _cot(X[v], X[u], X[w2])
        b0, b1 = _cot(X[u], X[v], X[w3]), _cot(X[v], X[u], X[w3])
        K = np.array([a1 + b1, a0 + b0, -(a0 + a1), -(b0 + b1)])
        H.append(((int(u), int(v), w2, w3), K, 3.0 / (area[0] + area[1])))
    return H


def q_dense(n, H):
    """(Q (n, n) float64, pattern (n, n) bool: the pairs of vertices that share a hinge, the diagonal included)"""
    Q, P = np.zeros((n, n)), np.zeros((n, n), bool)
    for idx, K, c in H:
        Q[np.ix_(idx, idx)] += c * np.outer(K, K)
        P[np.ix_(idx, idx)] = True
    return Q, P


def force64(k, H, x):
    """f = -k sum_h c_h K_h (K_h . x), hinge by hinge (not through Q)"""
    x = np.asarray(x, np.float64)
    f = np.zeros_like(x)
    for idx, K, c in H:
        g = K @ x[list(idx)]
        f[list(idx)] -= k * c * K[:, None] * g[None]
    return f


def energy64(k, H, x):
    x = np.asarray(x, np.float64)
    return 0.5 * k * sum(c * float(np.sum((K @ x[list(idx)]) ** 2)) for idx, K, c in H)


def bound(k, H, x):
    """B_i (n,)"""
    x = np.asarray(x, np.float64)
    B = np.zeros(len(x))
    for idx, K, c in H:
        P = x[list(idx)]
        d = max(float(np.linalg.norm(P[a] - P[b])) for a in range(4) for b in range(a))
        for a, i in enumerate(idx):
            B[i] += k * c * abs(K[a]) * float(np.abs(K).sum()) * d
    return B


def rounding_count(P):
    """R_i (n,) = n_i + 3, n_i the off-diagonal entries of row i of the pattern"""
    return (P.sum(axis=1) - P.diagonal()) + 3.0


def rows32(k, Q, P, x32):
    """the engine's row evaluation in float32: f_i = sum_j fma(-float(k Q_ij), x_j - x_i, .), ascending j != i.  (The
    fused multiply-add is formed in float64 and rounded to float32: the product of two floats is exact in double, the
    sum is rounded twice, which differs from a true fma in rare last bits only -- a restatement, not a bit copy.)"""
    x32 = np.asarray(x32, np.float32)
    k = float(np.float32(k))
    f = np.zeros_like(x32)
    for i in range(len(x32)):
        acc = np.zeros(3, np.float32)
        for j in np.flatnonzero(P[i]):
            if j == i:
                continue
            c = np.float32(k * Q[i, j])
            d = (x32[j] - x32[i]).astype(np.float32)
            acc = (acc.astype(np.float64) - np.float64(c) * d.astype(np.float64)).astype(np.float32)
        f[i] = acc
    return f


def max_stable_dt(k, Q, mass):
    """2 / sqrt(max_i (1 / m_i) sum_j |k Q_ij|)"""
    w2 = float(np.max(np.abs(float(np.float32(k)) * Q).sum(axis=1) / np.asarray(mass, np.float64)))
    return 2.0 / np.sqrt(w2) if w2 > 0 else np.inf


def margin(err, B, R):
    """the worst |err| / (R 2^-24 B) over the vertices (0 where both vanish)"""
    e = np.abs(np.asarray(err, np.float64)).max(axis=1)
    b = R * U * B
    w = np.where(e == 0, 0.0, e / np.maximum(b, 1e-300))
    return float(w.max()) if len(w) else 0.0
