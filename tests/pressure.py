"""Enclosed-volume pressure per cloth (mpm_set_pressure; drake_amd/csrc/mpm_pressure.h) on the CPU: the model restated in
numpy float64 from its definition, the meshes, scenes and states of the tests, and their bounds.

The model.  Per cloth a gauge pressure g: the caller's p (constant), or min(pv / V, p_max) - p_ambient where V > 0 and
p_max - p_ambient otherwise (gas), with V = 1/6 sum_faces x_a . (x_b x x_c) taken from the FLOAT positions as the engine
takes them, g formed in float64 and rounded to float32 once.  The force on vertex i is (g / 6) sum (x_b - x_i) x
(x_c - x_i) over the faces around it, each rotated to read (i, b, c).  Energy: -p V, or -pv ln V + p_ambient V while the
gas is not capped, else 0.

The bound.  A vertex's force must lie within R_i 2^-24 |g| / 6 sum_entries |d_b| |d_c| of the float64 force of the float
positions, R_i = 7 + n_i: 7 counted in mpm_pressure.h (4 for an entry's component, 2 for g / 6 and the product with it,
1 for the second order), n_i additions of the row's entries."""
import math

import numpy as np

U = 2.0 ** -24
H0 = 1.0 / 128            # spacing of the sheet: half a cell at domain_bits 6
R_PRESSURE = 7.0
OFF, CONSTANT, GAS = 0, 1, 2
PRESSURE_DTYPE = np.dtype([("mode", "<u4"), ("p", "<f4"), ("pv", "<f4"), ("p_ambient", "<f4"), ("p_max", "<f4")])


# ---- meshes: float32 rest positions, int32 triangles, outward winding (V > 0) for the closed ones ---------------------
def volume64(x32, T):
    """1/6 sum x_a . (x_b x x_c) in float64 from float32 positions (math.fsum: the exact sum of the float64 terms)"""
    x = np.asarray(x32, np.float32).astype(np.float64)
    a, b, c = x[T[:, 0]], x[T[:, 1]], x[T[:, 2]]
    return math.fsum((a * np.cross(b, c)).sum(axis=1)) / 6.0


def _finish(X, T):
    X32, T = np.asarray(X, np.float64).astype(np.float32), np.asarray(T, np.int32)
    if volume64(X32 - X32.mean(axis=0), T) < 0:
        T = T[:, [0, 2, 1]].copy()
    return X32, T


def tetrahedron(centre, edge=2 * H0):
    X = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float64) * (edge / (2 * math.sqrt(2)))
    return _finish(X + centre, [(0, 1, 2), (0, 3, 1), (0, 2, 3), (1, 3, 2)])


def icosphere(centre, radius, subdivisions=2):
    t = (1 + math.sqrt(5)) / 2
    V = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    F = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    V = [np.array(v, np.float64) / np.linalg.norm(v) for v in V]
    for _ in range(subdivisions):
        mid, out = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                w = V[a] + V[b]
                V.append(w / np.linalg.norm(w))
                mid[key] = len(V) - 1
            return mid[key]

        for a, b, c in F:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        F = out
    return _finish(np.array(V) * radius + centre, F)


def bipyramid(centre, n=20, radius=4 * H0, height=3 * H0):
    ang = 2 * math.pi * np.arange(n) / n
    X = np.concatenate([np.stack([radius * np.cos(ang), radius * np.sin(ang), np.zeros(n)], axis=1), [[0, 0, height], [0, 0, -height]]])
    T = [(k, (k + 1) % n, n) for k in range(n)] + [((k + 1) % n, k, n + 1) for k in range(n)]
    return _finish(X + centre, T)


def sheet(n, m, origin, h=H0):
    X = np.zeros((n * m, 3))
    for i in range(n):
        for j in range(m):
            X[i * m + j] = (origin[0] + i * h, origin[1] + j * h, origin[2])
    T = []
    for i in range(n - 1):
        for j in range(m - 1):
            a, b, c, d = i * m + j, (i + 1) * m + j, (i + 1) * m + j + 1, i * m + j + 1
            T += [(a, b, c), (a, c, d)]
    return X.astype(np.float32), np.array(T, np.int32)


ICO_R = 4 * H0
MESHES = {
    "tetrahedron": lambda: tetrahedron((0.3, 0.7, 0.5)),
    "icosphere": lambda: icosphere((0.3, 0.3, 0.5), ICO_R),
    "bipyramid": lambda: bipyramid((0.7, 0.3, 0.5)),
    "sheet": lambda: sheet(12, 12, (0.6, 0.6, 0.5)),
    # more than one chunk of 1024 faces (1280: two), and more than eight (8450: nine, two to a run of the final sum)
    "icosphere3": lambda: icosphere((0.5, 0.5, 0.4), 6 * H0, 3),
    "sheet66": lambda: sheet(66, 66, (0.37, 0.37, 0.6), H0 / 2),
}
CLOSED = ("tetrahedron", "icosphere", "bipyramid")
_MESH = {}


def mesh(name):
    if name not in _MESH:
        _MESH[name] = MESHES[name]()
    return _MESH[name]


def make_table(rows):
    """rows: [(mode, p, pv, p_ambient, p_max)]"""
    out = np.zeros(len(rows), PRESSURE_DTYPE)
    for i, r in enumerate(rows):
        out[i] = r
    return out


def gas_row(name, over=1.5, p_ambient=100.0, p_max=1000.0):
    """a gas whose absolute pressure at the rest volume is `over` x p_ambient"""
    X, T = mesh(name)
    return (GAS, 0.0, np.float32(over * p_ambient * volume64(X, T)), p_ambient, p_max)


# scenes: (mesh names in cloth order, the table).  mixed: an unpressurised cloth between pressurised ones.
SCENES = {
    "mixed": lambda: (("icosphere", "sheet", "bipyramid", "tetrahedron"),
                      make_table([gas_row("icosphere"), (CONSTANT, -35.0, 0, 0, 0), (OFF, 0, 0, 0, 0), (CONSTANT, 80.0, 0, 0, 0)])),
    "gas_bipyramid": lambda: (("bipyramid", "tetrahedron"), make_table([gas_row("bipyramid"), gas_row("tetrahedron", over=3.0)])),
    "constant_icosphere": lambda: (("icosphere",), make_table([(CONSTANT, 60.0, 0, 0, 0)])),
    "large": lambda: (("sheet66", "icosphere3"), make_table([(CONSTANT, 25.0, 0, 0, 0), gas_row("icosphere3")])),
}
_SCENE = {}


def scene(name):
    """(cloths [(X, T)], table, X of all vertices (n, 3) float32, T of all faces in global vertex ids, cloth of vertex,
    cloth of face)"""
    if name not in _SCENE:
        names, table = SCENES[name]()
        cloths = [mesh(n) for n in names]
        off = np.cumsum([0] + [len(X) for X, _ in cloths[:-1]])
        X = np.concatenate([X for X, _ in cloths])
        T = np.concatenate([T + o for (_, T), o in zip(cloths, off)]).astype(np.int32)
        cv = np.concatenate([np.full(len(Xc), c) for c, (Xc, _) in enumerate(cloths)])
        cf = np.concatenate([np.full(len(Tc), c) for c, (_, Tc) in enumerate(cloths)])
        _SCENE[name] = (cloths, table, X, T, cv, cf)
    return _SCENE[name]


# ---- states: float32 positions per vertex ------------------------------------------------------------------------------
STATES = ("rest", "translation", "rotation", "random", "collapsed")


def state(st, X, cloth_of_vertex):
    """rest; a rigid translation; a rigid rotation about the scene's centre; a random perturbation of 0.15 H0; collapsed:
    every cloth reflected through its own centroid (a closed cloth turns inside out: V < 0)"""
    x = np.asarray(X, np.float64).copy()
    if st == "rest":
        pass
    elif st == "translation":
        x += np.array([0.05, -0.03, 0.11])
    elif st == "rotation":
        k = np.array([1.0, 2.0, -1.5])
        k /= np.linalg.norm(k)
        K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        R = np.eye(3) + math.sin(0.7) * K + (1 - math.cos(0.7)) * K @ K
        c = x.mean(axis=0)
        x = (x - c) @ R.T + c
    elif st == "random":
        x += 0.15 * H0 * np.random.default_rng(5).normal(size=x.shape)
    elif st == "collapsed":
        for c in np.unique(cloth_of_vertex):
            sel = cloth_of_vertex == c
            x[sel] = 2 * x[sel].mean(axis=0) - x[sel]
    else:
        raise KeyError(st)
    assert x.min() > 0.1 and x.max() < 0.9
    return x.astype(np.float32)


# ---- the model in float64 -------------------------------------------------------------------------------------------------
def gauge(row, V):
    """(g float32, capped, energy float64) of one cloth from its table row and its volume"""
    mode = int(row["mode"])
    if mode == CONSTANT:
        return np.float32(row["p"]), False, -float(row["p"]) * V
    if mode == GAS:
        pv, pa, pm = float(row["pv"]), float(row["p_ambient"]), float(row["p_max"])
        free = V > 0 and pv / V < pm
        g = np.float32((pv / V if free else pm) - pa)
        return g, not free, (-pv * math.log(V) + pa * V) if free else 0.0
    return np.float32(0.0), False, 0.0


def cloth_states(table, x32, T, cloth_of_face):
    """[(V, g float32, capped, energy)] per cloth"""
    out = []
    for c in range(len(table)):
        V = volume64(x32, T[cloth_of_face == c])
        out.append((V,) + gauge(table[c], V))
    return out


def volume_bound(x32, T):
    """|engine's V - exact V| for a double sum of the terms in any fixed order: a term a . (b x c) carries 8 roundings of
    2^-53 on |a| |b| |c| at most (6 products and 3 + 2 additions bounded through Cauchy-Schwarz by 3 |a||b||c| ... counted
    generously as 8), and each of the n additions one rounding of a partial sum of at most sum |a||b||c|: (8 + n) 2^-53
    sum |a||b||c| / 6, and one more rounding for the division."""
    x = np.asarray(x32, np.float32).astype(np.float64)
    n = np.linalg.norm
    s = float((n(x[T[:, 0]], axis=1) * n(x[T[:, 1]], axis=1) * n(x[T[:, 2]], axis=1)).sum())
    return (9 + len(T)) * 2.0 ** -53 * s / 6.0


def entries(T, n_verts):
    """per vertex the list of (b, c) of the faces around it, rotated to read (i, b, c), in ascending face id"""
    out = [[] for _ in range(n_verts)]
    for f in range(len(T)):
        for k in range(3):
            out[int(T[f, k])].append((int(T[f, (k + 1) % 3]), int(T[f, (k + 2) % 3])))
    return out


def cross_sums64(x32, T, n_verts):
    """(sum (x_b - x_i) x (x_c - x_i) (n, 3), sum |d_b| |d_c| (n,), entries per vertex (n,)) in float64, vectorised"""
    x = np.asarray(x32, np.float32).astype(np.float64)
    S, A, N = np.zeros((n_verts, 3)), np.zeros(n_verts), np.zeros(n_verts)
    for k in range(3):
        i, b, c = T[:, k], T[:, (k + 1) % 3], T[:, (k + 2) % 3]
        db, dc = x[b] - x[i], x[c] - x[i]
        np.add.at(S, i, np.cross(db, dc))
        np.add.at(A, i, np.linalg.norm(db, axis=1) * np.linalg.norm(dc, axis=1))
        np.add.at(N, i, 1.0)
    return S, A, N


def vertex_forces64(table, x32, T, cloth_of_vertex, cloth_of_face, g_of_cloth=None):
    """(f (n, 3) float64, bound (n,) = R_i 2^-24 |g| / 6 sum |d_b||d_c|, accumulation bound (n,) with R_i = n_i alone)
    g_of_cloth: the gauge pressures to use (float32 per cloth); default: the restated ones"""
    n = len(cloth_of_vertex)
    S, A, N = cross_sums64(x32, T, n)
    if g_of_cloth is None:
        g_of_cloth = [s[1] for s in cloth_states(table, x32, T, cloth_of_face)]
    g = np.array([float(q) for q in g_of_cloth])[cloth_of_vertex]
    return (g / 6.0)[:, None] * S, (R_PRESSURE + N) * U * np.abs(g) / 6.0 * A, N * U * np.abs(g) / 6.0 * A


def margin(err, bound):
    """the worst |err| / bound over the vertices (0 where the error vanishes)"""
    e = np.abs(np.asarray(err, np.float64))
    e = e.max(axis=1) if e.ndim == 2 else e
    w = np.where(e == 0, 0.0, e / np.maximum(bound, 1e-300))
    return float(w.max()) if len(w) else 0.0


# ---- closedness: every directed edge exactly once, its reverse exactly once --------------------------------------------------
def first_open_edge(T):
    """None for a closed, consistently wound mesh; else the first directed edge, in face order, that does not occur
    exactly once with its reverse exactly once"""
    count = {}
    for f in T:
        for k in range(3):
            e = (int(f[k]), int(f[(k + 1) % 3]))
            count[e] = count.get(e, 0) + 1
    for f in T:
        for k in range(3):
            a, b = int(f[k]), int(f[(k + 1) % 3])
            if a == b or count[(a, b)] != 1 or count.get((b, a), 0) != 1:
                return (a, b)
    return None


# ---- the row table, restated ------------------------------------------------------------------------------------------
def table_layout(cloths, modes, slice_=64):
    """(row_pid, row_cloth, slice_off, ent (n, 2) uint32) as pressure_table lays them out; cloths: [(X, T)] with T local"""
    nf = sum(len(T) for _, T in cloths)
    row_pid, row_cloth, rows = [], [], []
    v0 = 0
    for c, (X, T) in enumerate(cloths):
        if modes[c] != OFF:
            ent = entries(T, len(X))
            for v in range(len(X)):
                row_pid.append(nf + v0 + v)
                row_cloth.append(c)
                rows.append([(nf + v0 + b, nf + v0 + cc) for b, cc in ent[v]])
        v0 += len(X)
    n = len(rows)
    slice_off, out = [0], []
    for s in range((n + slice_ - 1) // slice_):
        lo, hi = s * slice_, min(n, (s + 1) * slice_)
        width = max(len(r) for r in rows[lo:hi])
        block = np.zeros((width, slice_, 2), np.int64)
        for l in range(slice_):
            r = min(lo + l, n - 1)
            src = rows[r] if lo + l < n else []
            for q in range(width):
                block[q, l] = src[q] if q < len(src) else (row_pid[r], row_pid[r])
        out.append(block.reshape(-1, 2))
        slice_off.append(slice_off[-1] + width * slice_)
    ent = np.concatenate(out) if out else np.zeros((0, 2), np.int64)
    return np.array(row_pid, np.int64), np.array(row_cloth, np.int64), np.array(slice_off, np.int64), ent
