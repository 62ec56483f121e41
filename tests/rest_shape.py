"""Rest shape apart from the pose (mpm_set_rest_shape): the poses and rest shapes of tests/test_rest_shape.py (CPU) and
tests/test_rest_shape_gpu.py, built from the meshes of tests/rest_meshes.py, and the small sheets of the dynamics tests.

A case is a pair (rest shape R, pose P) of one mesh: an engine is added at P and given set_rest_shape(R); its twin is added
at R.  The float64 rest state of R is rest_meshes.rest_state(R), made once per case, and it is compared under that
module's bounds unchanged (bound_ratios with ENGINE_FACTOR x ORACLE_C*): this module introduces no tolerance.

Kinds of pose (KINDS).  In the first four the rest shape is the mesh M of rest_meshes itself, kept inside its cube
[0.15, 0.85]^3, and the pose is M moved:
  rigid   rotated by 0.1 rad about a random axis through the cube's centre and shifted by (0.01, -0.02, 0.015)
  scale   scaled by 1.1 about the centre
  shear   x += 0.1 (y - 0.5),  z += 0.05 (x - 0.5)
  noise   every vertex moved by up to 0.05 of its shortest incident edge, at random (a vertex in no face stays)
In the two EXACT kinds the pose is M and the rest shape is derived from it in float arithmetic that does not round:
  double  R = M / 2: the pose is the rest shape scaled by exactly 2.  Every edge of R is exactly half the pose's, so
          Finalize's arithmetic (products, sums, 1 / sqrt, the division by det) scales by powers of two without a
          rounding of its own: Dm^-1(R) = 2 Dm^-1(M) and vol(R) = vol(M) / 4 to the bit -- checked against an untouched
          engine at M, no twin and no bound needed
  shift   R = M - 1/16: every coordinate of M is >= 0.15 > 1/16 and a multiple of its own ulp, as 1/16 is, and the
          difference is smaller in magnitude: it is exact.  The edges of R are then the pose's, bit for bit, and so is the
          whole rest state
Every pose and every rest shape lies inside [0.05, 0.95]^3 (three wall cells of the 64^3 grid are 0.047), is accepted by
mpm_rest_shape_check, and no rest shape's kappa exceeds rest_meshes.KAPPA_MAX (tests/test_rest_shape.py asserts all of
it)."""
import numpy as np

from tests import rest_meshes as rm

BITS = rm.BITS
DX = rm.DX
DOMAIN = (0.05, 0.95)
DENSITIES = (500.0, 2000.0, 7300.0)       # tests/test_rest_state_gpu.py's
KINDS = ("rigid", "scale", "shear", "noise", "double", "shift")
EXACT = ("double", "shift")
SHIFT = 1.0 / 16
THREE = "three"                           # rest_meshes.three_cloths(): slivers as two cloths, and valence

# (mesh, kind) of the twin tests: every mesh of rest_meshes once with a general pose, the valence mesh (1 to 40 faces
# around a vertex) with every kind, the three cloths with two
CASES = (("orientations", "rigid"), ("slivers", "noise"), ("scales", "shear"), ("valence", "scale"), ("valence", "rigid"),
         ("valence", "shear"), ("valence", "noise"), ("valence", "double"), ("valence", "shift"), ("slivers", "double"),
         ("scales", "shift"), ("tails_1", "noise"), ("tails_255", "scale"), ("tails_256", "shear"), ("tails_257", "rigid"),
         (THREE, "noise"), (THREE, "scale"))

_CACHE = {}


def base(name):
    """the mesh of rest_meshes called `name`, or the merged mesh of its three cloths"""
    if name == THREE:
        return rm.three_cloths()[1]
    return rm.meshes()[name][0]


def _shortest_incident_edge(mesh):
    x, idx = mesh.pos.astype(np.float64), mesh.idx
    out = np.full(mesh.nv, np.inf)
    for a, b in ((0, 1), (1, 2), (2, 0)):
        e = np.linalg.norm(x[idx[:, a]] - x[idx[:, b]], axis=1)
        np.minimum.at(out, idx[:, a], e)
        np.minimum.at(out, idx[:, b], e)
    return np.where(np.isfinite(out), out, 0.0)


def moved(mesh, kind, seed=0):
    """the float32 positions of `mesh` moved by a general kind"""
    rng = np.random.default_rng(1000 + seed)
    x = mesh.pos.astype(np.float64)
    c = np.full(3, 0.5)
    if kind == "rigid":
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        Rm = np.eye(3) + np.sin(0.1) * K + (1 - np.cos(0.1)) * K @ K
        y = c + (x - c) @ Rm.T + np.array([0.01, -0.02, 0.015])
    elif kind == "scale":
        y = c + 1.1 * (x - c)
    elif kind == "shear":
        y = x.copy()
        y[:, 0] += 0.1 * (x[:, 1] - 0.5)
        y[:, 2] += 0.05 * (x[:, 0] - 0.5)
    elif kind == "noise":
        y = x + 0.05 * _shortest_incident_edge(mesh)[:, None] * rng.uniform(-1.0, 1.0, x.shape)
    else:
        raise KeyError(kind)
    return y.astype(np.float32)


def case(name, kind):
    """-> dict(rest: Mesh R, pose: Mesh P, ref: rest_state(R), base: the mesh of rest_meshes, parts: None or the three
    cloths as [(rest Mesh, pose Mesh)]); made once"""
    key = (name, kind)
    if key not in _CACHE:
        m = base(name)
        if kind == "double":
            rest, pose = rm.Mesh(f"{name} / 2", m.pos * np.float32(0.5), m.vel, m.idx), m
        elif kind == "shift":
            rest, pose = rm.Mesh(f"{name} - 1/16", m.pos - np.float32(SHIFT), m.vel, m.idx), m
        else:
            rest, pose = m, rm.Mesh(f"{name}, {kind}", moved(m, kind, seed=len(name)), m.vel, m.idx)
        if kind in EXACT or name == THREE:
            ref = rm.rest_state(rest)
        else:
            ref = rm.meshes()[name][1]
        parts = None
        if name == THREE:
            parts, at = [], 0
            for p in rm.three_cloths()[0]:
                sl = slice(at, at + p.nv)
                parts.append((rm.Mesh(p.name, rest.pos[sl], p.vel, p.idx), rm.Mesh(p.name, pose.pos[sl], p.vel, p.idx)))
                at += p.nv
        _CACHE[key] = dict(rest=rest, pose=pose, ref=ref, base=m, parts=parts)
    return _CACHE[key]


# ---- the sheets of the dynamics tests --------------------------------------------------------------------------------
SHEET_RES = 12


def sheet(side=0.2, z=0.5, centre=(0.5, 0.5), jitter=0.0, seed=7):
    """a 12 x 12 sheet: (pos (144, 3) float32, idx (242, 3) int32); jitter in units of the spacing"""
    from drake_amd import scenes
    pos, idx = scenes.cloth_sheet(SHEET_RES, side, z, centre)
    if jitter:
        j = np.stack([scenes.hash_uniform(seed, len(pos), c) for c in range(3)], -1)
        pos = (pos + np.float32(jitter * side / SHEET_RES) * j).astype(np.float32)
    return pos, idx.reshape(-1, 3)


def scaled(pos, s, centre=None):
    """pos scaled by s about its own mean (or `centre`), in float64, rounded once"""
    x = pos.astype(np.float64)
    c = x.mean(axis=0) if centre is None else np.asarray(centre, np.float64)
    return (c + s * (x - c)).astype(np.float32)


def boundary(res=SHEET_RES):
    i, j = np.meshgrid(np.arange(res), np.arange(res), indexing="ij")
    return np.flatnonzero(((i == 0) | (i == res - 1) | (j == 0) | (j == res - 1)).reshape(-1))


def edges(idx):
    e = np.concatenate([idx[:, [0, 1]], idx[:, [1, 2]], idx[:, [2, 0]]])
    return np.unique(np.sort(e, axis=1), axis=0)


def mean_edge(pos, idx):
    e = edges(idx)
    x = np.asarray(pos, np.float64)
    return float(np.linalg.norm(x[e[:, 0]] - x[e[:, 1]], axis=1).mean())


def base_cells(x, bits=BITS):
    """the base cell of every position (mpm_device.h: base_cell), one integer per particle, and its distance (cells) to
    the nearest cell boundary"""
    t = np.asarray(x, np.float32).astype(np.float64) * (1 << bits) - 0.5
    c = np.floor(t).astype(np.int64)
    return (c[:, 0] << 2 * bits) | (c[:, 1] << bits) | c[:, 2], np.minimum(t - np.floor(t), np.ceil(t) - t).min(axis=1)


def spread(idx, pitch=3.2, origin=0.2, z=0.5):
    """The 12 x 12 sheet drawn out to `pitch` cells between neighbours, (144, 3) float32: every vertex then has a base
    cell to itself and so has every face particle (the centroids of a quad's two faces lie pitch / 3 > 1 cells apart).
    A re-sort of this state orders the particles by their cells alone, whatever order they were in: two engines that
    were finalized at different positions hold the same particle order afterwards (one_per_cell asserts the premise)."""
    i, j = np.meshgrid(np.arange(SHEET_RES), np.arange(SHEET_RES), indexing="ij")
    x = np.stack([origin + pitch * DX * i.reshape(-1), origin + pitch * DX * j.reshape(-1), np.full(i.size, z)], 1)
    return x.astype(np.float32)


def one_per_cell(pos, idx, margin=1e-3):
    """True when no two vertices and no two face particles (the float32 mean of the corners, as the tests upload it) share
    a base cell, none closer than `margin` cells to a cell boundary"""
    x = np.asarray(pos, np.float32)
    fc = x[idx].astype(np.float64).mean(axis=1).astype(np.float32)
    (cv, dv), (cf, df) = base_cells(x), base_cells(fc)
    return bool(len(np.unique(cv)) == len(cv) and len(np.unique(cf)) == len(cf) and dv.min() > margin and df.min() > margin)


def arc(pos, radius, centre_x=0.5):
    """a flat sheet at height z rolled about the y axis onto a cylinder of `radius` (arc length along x kept)"""
    x = pos.astype(np.float64)
    th = (x[:, 0] - centre_x) / radius
    return np.stack([centre_x + radius * np.sin(th), x[:, 1], x[:, 2] - radius * (1.0 - np.cos(th))], 1).astype(np.float32)


def octahedron(r=0.06, centre=(0.5, 0.5, 0.5)):
    """a closed mesh wound outwards: (pos (6, 3) float32, idx (8, 3) int32); its signed volume is 4 r^3 / 3"""
    c = np.asarray(centre, np.float64)
    pos = c + r * np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
    idx = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)
    return pos.astype(np.float32), idx


def signed_volume(pos, idx):
    x = np.asarray(pos, np.float64)
    return float(np.einsum("fi,fi->f", x[idx[:, 0]], np.cross(x[idx[:, 1]], x[idx[:, 2]])).sum() / 6.0)
