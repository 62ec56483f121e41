"""Links between cloth vertices (mpm_set_links; drake_amd/csrc/mpm_links.h) on the CPU: the model restated in numpy
float64 from its definition, the scenes, link mixes and states of the tests, and their bounds.

The model.  A link joins vertices a, b with stiffness k, rest length L, damping c.  With d = x_b - x_a, w = v_b - v_a the
force on a is
    seam   (L == 0)   f = k d + c w
    spring (L > 0)    f = (k (l - L) + c (w . d) / l) d / l,  l = |d|;  nothing where |d|^2 < 1e-30
    tension only      nothing unless l > L
and the force on b is its negative.  Elastic energy of a link that acts: 1/2 k (l - L)^2.  Which links act is decided
on the FLOAT differences, as the engine decides it (l from fma(d2, d2, fma(d1, d1, d0 d0)) and a float square root): the
gates are part of the model, and a float64 gate would flip a link that sits exactly on l == L.

The bound.  Per link and component S = k (l + L) + c |w| (the cancellation in l - L is at the scale of l + L, not of the
stretch); a link that does not act has S = 0.  A vertex's force must lie within R_i 2^-24 sum S of the float64 force of
the float positions and velocities, R_i = 18 + n_i: 18 counted from link_force (mpm_links.h: 17 first-order roundings
of the spring law and one for the second order), n_i additions of the row's entries."""
import math

import numpy as np

U = 2.0 ** -24
H0 = 1.0 / 128            # spacing of the sheets: half a cell at domain_bits 6
R_LINK = 18.0
TENSION = 1
LINK_DTYPE = np.dtype([("a", "<u4"), ("b", "<u4"), ("stiffness", "<f4"), ("rest_length", "<f4"), ("damping", "<f4"),
                       ("flags", "<u4")])


# ---- meshes: float32 rest positions on a dyadic lattice (differences of lattice points are exact), int32 triangles ----
def sheet(n, m, origin):
    X = np.zeros((n * m, 3))
    for i in range(n):
        for j in range(m):
            X[i * m + j] = (origin[0] + i * H0, origin[1] + j * H0, origin[2])
    T = []
    for i in range(n - 1):
        for j in range(m - 1):
            a, b, c, d = i * m + j, (i + 1) * m + j, (i + 1) * m + j + 1, i * m + j + 1
            T += [(a, b, c), (a, c, d)]
    X32 = X.astype(np.float32)
    assert np.array_equal(X32.astype(np.float64), X)
    return X32, np.array(T, np.int32)


def make_links(rows):
    """rows: [(a, b, k, L, c, flags)]"""
    out = np.zeros(len(rows), LINK_DTYPE)
    for i, r in enumerate(rows):
        out[i] = r
    return out


SEAM_GAP = 2 * H0


def scene_seam(k=37.3, c=0.013):
    """two coplanar 24 x 24 sheets a gap of 2 H0 apart along x, 24 seam links along the facing edges"""
    n = 24
    A = sheet(n, n, (0.25, 0.375, 0.5))
    B = sheet(n, n, (0.25 + (n - 1) * H0 + SEAM_GAP, 0.375, 0.5))
    rows = [((n - 1) * n + j, n * n + j, k, 0.0, c, 0) for j in range(n)]
    return [A, B], make_links(rows)


STACK_GAP = 2 * H0


def scene_mixed():
    """two 12 x 12 sheets, B a gap of 2 H0 above A.  80 vertical links of every kind in turn (160 linked rows: two full
    slices of 64 and a partial one), a hub (vertex 0 of A) with 17 more links into B (with its vertical link, an
    in-cloth link: 19 entries, three batches of 8), a link inside cloth A whose rest state has
    l == L exactly (3-4-5 on the lattice), a duplicate pair, and a pair (143, 287) that the states place on one point."""
    n = 12
    A = sheet(n, n, (0.375, 0.375, 0.5))
    B = sheet(n, n, (0.375, 0.375, 0.5 + STACK_GAP))
    nv = n * n
    g = STACK_GAP
    kinds = [
        (30.0, 0.0, 0.02, 0),                 # seam, damped
        (50.0, 0.5 * g, 0.0, 0),              # spring, stretched
        (50.0, 2.0 * g, 0.03, 0),             # spring, compressed
        (70.0, 2.0 * g, 0.05, TENSION),       # cord, slack
        (70.0, 0.5 * g, 0.05, TENSION),       # cord, taut
        (70.0, g, 0.05, TENSION),             # cord, exactly l == L in the rest state
        (20.0, 0.0, 0.0, TENSION),            # tension-only seam (acts wherever the ends differ)
    ]
    rows = [(v, nv + v) + kinds[v % len(kinds)] for v in range(80)]
    rows += [(0, nv + 1 + q) + kinds[q % len(kinds)] for q in range(17)]          # the hub
    rows += [(0, 3 * n + 4, 60.0, 5 * H0, 0.04, TENSION)]                          # inside A: d = (3, 4, 0) H0, l == L
    rows += [(5, nv + 5, 50.0, 2.0 * g, 0.03, 0), (nv + 5, 5, 50.0, 2.0 * g, 0.03, 0)]   # the pair (5, nv + 5) twice more
    rows += [(nv - 1, 2 * nv - 1, 45.0, g, 0.02, 0)]                               # coincident ends with L > 0
    return [A, B], make_links(rows)


COINCIDENT = (143, 287)

SCENES = {"seam": scene_seam, "mixed": scene_mixed}
_SCENE = {}


def scene(name):
    """(cloths [(X, T)], links, X of all vertices (n, 3) float32)"""
    if name not in _SCENE:
        cloths, links = SCENES[name]()
        _SCENE[name] = (cloths, links, np.concatenate([X for X, _ in cloths]))
    return _SCENE[name]


# ---- states: (x, v) float32 per vertex ----------------------------------------------------------------------------------
def _positions(name, X, perturb, seed):
    x = np.asarray(X, np.float64).copy()
    if perturb:
        x += 0.2 * H0 * np.random.default_rng(seed).normal(size=x.shape)
    x = x.astype(np.float32)
    if name == "mixed":
        x[COINCIDENT[1]] = x[COINCIDENT[0]]
    return x


def state(st, name, X):
    """rest: the lattice positions, v = 0; translation / rotation / random: perturbed positions with a rigid translation,
    a rigid rotation about the scene's centre, random velocities"""
    r = np.random.default_rng(11)
    if st == "rest":
        x = _positions(name, X, False, 0)
        return x, np.zeros_like(x)
    x = _positions(name, X, True, 5)
    if st == "translation":
        v = np.broadcast_to(np.array([0.7, -0.4, 0.25]), x.shape)
    elif st == "rotation":
        om = np.array([3.0, -2.0, 5.0])
        v = np.cross(om, x.astype(np.float64) - x.astype(np.float64).mean(axis=0))
    elif st == "random":
        v = 0.5 * r.normal(size=x.shape)
    else:
        raise KeyError(st)
    return x, np.asarray(v, np.float32).copy()


STATES = ("rest", "translation", "rotation", "random")


# ---- the model in float64 -----------------------------------------------------------------------------------------------
def _l32(d32):
    """the engine's float length and squared length of float differences (the fused multiply-adds formed in double and
    rounded once more: the same float except in rare last bits, which no state of the tests sits on)"""
    d = d32.astype(np.float64)
    p = (d[:, 0] * d[:, 0]).astype(np.float32)
    p = (d[:, 1] * d[:, 1] + p.astype(np.float64)).astype(np.float32)
    p = (d[:, 2] * d[:, 2] + p.astype(np.float64)).astype(np.float32)
    return p, np.sqrt(p)


def acts(links, x32):
    """(n,) bool: the links that act on the float positions x32"""
    x32 = np.asarray(x32, np.float32)
    d32 = x32[links["b"]] - x32[links["a"]]
    l2, l = _l32(d32)
    L = links["rest_length"]
    return ((L == 0) | (l2 >= np.float32(1e-30))) & (((links["flags"] & TENSION) == 0) | (l > L))


def link_forces64(links, x32, v32):
    """(force on a (n, 3) float64, S (n,), l (n,) float64, acts (n,))"""
    x, v = np.asarray(x32, np.float32).astype(np.float64), np.asarray(v32, np.float32).astype(np.float64)
    k, L, c = (links[q].astype(np.float64) for q in ("stiffness", "rest_length", "damping"))
    d, w = x[links["b"]] - x[links["a"]], v[links["b"]] - v[links["a"]]
    l = np.sqrt((d * d).sum(axis=1))
    on = acts(links, x32)
    ls = np.where(l > 0, l, 1.0)
    spring = ((k * (l - L) + c * (w * d).sum(axis=1) / ls) / ls)[:, None] * d
    seam = k[:, None] * d + c[:, None] * w
    f = np.where((L > 0)[:, None], spring, seam) * on[:, None]
    S = (k * (l + L) + c * np.sqrt((w * w).sum(axis=1))) * on
    return f, S, l, on


def vertex_forces64(links, x32, v32, n_verts):
    """(f (n_verts, 3) float64, bound (n_verts,) = R_i 2^-24 sum S, accumulation bound (n_verts,) = n_i 2^-24 sum S)"""
    f, S, _, _ = link_forces64(links, x32, v32)
    F, SS, n = np.zeros((n_verts, 3)), np.zeros(n_verts), np.zeros(n_verts)
    for end, sign in (("a", 1.0), ("b", -1.0)):
        np.add.at(F, links[end], sign * f)
        np.add.at(SS, links[end], S)
        np.add.at(n, links[end], 1.0)
    return F, (R_LINK + n) * U * SS, n * U * SS


def energy64(links, x32):
    """(sum of 1/2 k (l - L)^2 over the links that act, in extended precision; its bound; the lengths (n,) float64).
    The bound, in units of 2^-53 of T = 1/2 k (l + L)^2 per term: the engine forms d (1 per component), |d|^2 (5 roundings,
    2.5 on l), the square root (1), l - L (1), its square (1) and the two products with 1/2 k (2) -- the error of l,
    4.5, enters twice through the square: at most 16 of T; then the n - 1 additions of the sum in link order, each at most
    one rounding of a partial sum: (16 + n) 2^-53 sum T."""
    x = np.asarray(x32, np.float32).astype(np.longdouble)
    k, L = links["stiffness"].astype(np.longdouble), links["rest_length"].astype(np.longdouble)
    d = x[links["b"]] - x[links["a"]]
    l = np.sqrt((d * d).sum(axis=1))
    on = acts(links, x32)
    e = 0.5 * k * (l - L) ** 2 * on
    T = 0.5 * k * (l + L) ** 2 * on
    return float(math.fsum(float(q) for q in e)), float((16 + len(links)) * 2.0 ** -53 * T.sum()), l.astype(np.float64)


def margin(err, bound):
    """the worst |err| / bound over the vertices (0 where the error vanishes)"""
    e = np.abs(np.asarray(err, np.float64))
    e = e.max(axis=1) if e.ndim == 2 else e
    w = np.where(e == 0, 0.0, e / np.maximum(bound, 1e-300))
    return float(w.max()) if len(w) else 0.0


def max_stable_dt(links, mass):
    """the positive root of W dt^2 + 2 G dt = 4, W = max_i (2 / m_i) sum k, G = max_i (2 / m_i) sum c"""
    ks, cs = np.zeros(len(mass)), np.zeros(len(mass))
    for end in ("a", "b"):
        np.add.at(ks, links[end], links["stiffness"].astype(np.float64))
        np.add.at(cs, links[end], links["damping"].astype(np.float64))
    W, G = float((2 * ks / mass).max()), float((2 * cs / mass).max())
    return 4.0 / (G + math.sqrt(G * G + 4 * W)) if W > 0 or G > 0 else math.inf
