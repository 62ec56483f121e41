"""Float64 reference of the grid update's rigid bodies (mpm_set_grid_bodies, mpm_bc = MPM_BC_BODIES) and the scenes of
tests/test_grid_bodies.py (CPU) and tests/test_grid_bodies_gpu.py.  No GPU, no engine.

The reference is a function of the node sums (m, mv) -- the engine's own, downloaded after ParticleToGrid --, the wall
rule and the table, taking the caller's float32 poses and dimensions as exact inputs.  Signed distances and gradients
are closed forms written here (the ellipsoid's nearest point: the root of its secular equation by bisection to the last
bit of a double); a mesh body is tests/sdf_mesh_reference.interpolant on its lattice values, which is the header's
definition of that surface.

Every formula takes the number type T: T = float64 is the reference; T = float32 is THE SAME formulas rounded to float
after every operation, and the distance between the two evaluations is the measured float noise the engine is held
to (x NOISE_FLOOR).  The float32 evaluation takes membership and the deciding body from the float64 one: it measures the
noise of the update formulas at nodes where membership is not in question (see `undecided`)."""
import numpy as np

from drake_amd import scenes
from tests import sdf_mesh_reference as smr
from tests import transfer_layouts as tl

F32, F64 = np.float32, np.float64
FIXED, SLIP_APPROACHING, SLIP = 0, 1, 2
HALF_SPACE, SPHERE, BOX, CAPSULE, CYLINDER, ELLIPSOID, MESH = 0, 1, 2, 3, 4, 5, 6   # MESH: this module's tag only
KIND_NAMES = ("half_space", "sphere", "box", "capsule", "cylinder", "ellipsoid", "mesh")
DELTA = 4e-6          # the probe of `undecided`: some 30 ulp of a coordinate below 1
NORMAL_TOL = 1e-3
MAX_UNDECIDED_SHARE = 0.01
MIN_COMPARED = 100
WALL = 3


def rot(axis, angle):
    """Rodrigues, rounded to float32 once: what a caller hands over as R_WB (row major, body -> world)"""
    a = np.asarray(axis, F64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return (np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K).astype(F32)


class Body:
    """one entry of the table; every number is kept as the float32 the engine receives"""

    def __init__(self, kind, body=0, p=(0, 0, 0), R=None, dims=(0, 0, 0), v=(0, 0, 0), w=(0, 0, 0), mode=FIXED, friction=0.3,
                 mesh=None, cell=None, pad=2):
        self.kind, self.body, self.mode = int(kind), int(body), int(mode)
        self.p, self.dims, self.v, self.w = (np.asarray(a, F32) for a in (p, dims, v, w))
        self.R = np.eye(3, dtype=F32) if R is None else np.asarray(R, F32).reshape(3, 3)
        self.friction = F32(friction)
        self.mesh, self.cell, self.pad = mesh, cell, pad    # mesh: (verts, tris) in the body frame
        self.lattice = None                                 # (values (nz, ny, nx), n, lo, cell) once known

    def cpu_lattice(self):
        """the lattice as mpm_sdf_shape_from_mesh lays it out, values by the float64 mesh distance"""
        if self.lattice is None:
            verts, tris = self.mesh
            n, lo = smr.lattice_layout(verts, self.cell, self.pad)
            nodes = smr.lattice_nodes(n, lo, self.cell)
            vals = smr.mesh_sdf(nodes.reshape(-1, 3), verts, tris).reshape(n[2], n[1], n[0]).astype(F32)
            self.lattice = (vals, n, lo, F32(self.cell))
        return self

    def capi(self, shape_id=None):
        from drake_amd import Collider, GridBody, GB_NO_MESH
        c = Collider(0 if self.kind == MESH else self.kind, body=self.body, p_WB=self.p, R_WB=self.R, dims=self.dims,
                     v=self.v, w=self.w)
        return GridBody(c, sdf_shape=GB_NO_MESH if self.kind != MESH else int(shape_id), mode=self.mode,
                        friction=float(self.friction))


# ---- signed distances and gradients, generic in the number type ---------------------------------------------------------
def _norm(a):
    return np.sqrt((a * a).sum(-1))


def _ellipsoid_normal(y, a):
    """body-frame unit gradient at the nearest point of the ellipsoid with semi-axes a to y (N, 3), float64: the root t of
    sum (a_i y_i / (t + a_i^2))^2 = 1 in [-e^2 + e |y_e|, -e^2 + |a y|] (e the smallest semi-axis; D. Eberly, "Distance
    from a Point to an Ellipse, an Ellipsoid, or a Hyperellipsoid"), by bisection until the bracket stops shrinking"""
    y, a = np.asarray(y, F64), np.asarray(a, F64)
    ay = np.abs(y)
    e = int(np.argmin(a))
    t0 = -a[e] ** 2 + a[e] * np.maximum(ay[:, e], 1e-300)
    t1 = -a[e] ** 2 + _norm(a * ay)
    t1 = np.maximum(t1, t0)
    for _ in range(200):
        t = 0.5 * (t0 + t1)
        g = ((a * ay / (t[:, None] + a ** 2)) ** 2).sum(-1) - 1.0
        t0 = np.where(g > 0, t, t0)
        t1 = np.where(g > 0, t1, t)
    t = 0.5 * (t0 + t1)
    n = y / (t[:, None] + a ** 2)     # x_i / a_i^2 with x the nearest point
    return n / _norm(n)[:, None]


def body_sdf(b, x, T=F64, normals=True):
    """phi (N,) and the unit world gradient (N, 3) of body b at world points x, every operation in T"""
    x = np.asarray(x, T)
    R, p, d = b.R.astype(T), b.p.astype(T), b.dims.astype(T)
    xb = (x - p) @ R                      # R^T (x - p)
    N = len(x)
    g = np.zeros((N, 3), T)
    with np.errstate(all="ignore"):
        if b.kind == HALF_SPACE:
            phi = xb[:, 2].copy()
            g[:, 2] = 1
        elif b.kind == SPHERE:
            ln = _norm(xb)
            phi = ln - d[0]
            g = xb / ln[:, None]
        elif b.kind == BOX:
            q = np.abs(xb) - d
            sg = np.where(xb < 0, T(-1), T(1))
            m = q.max(1)
            ax = np.argmax(q, 1)          # (the first of equal maxima: x, then y, then z, as the engine's tie rule)
            inside = m <= 0
            o = np.maximum(q, 0)
            lo = _norm(o)
            phi = np.where(inside, m, lo)
            g_in = np.zeros((N, 3), T)
            g_in[np.arange(N), ax] = sg[np.arange(N), ax]
            g = np.where(inside[:, None], g_in, sg * o / lo[:, None])
        elif b.kind == CAPSULE:
            r = xb.copy()
            r[:, 2] = xb[:, 2] - np.clip(xb[:, 2], -d[1], d[1])
            ln = _norm(r)
            phi = ln - d[0]
            g = r / ln[:, None]
        elif b.kind == CYLINDER:
            # (without the boundary band of four float epsilons: its nodes are undecided by construction, DELTA is wider)
            r = np.sqrt(xb[:, 0] ** 2 + xb[:, 1] ** 2)
            az = np.abs(xb[:, 2])
            sz = np.where(xb[:, 2] < 0, T(-1), T(1))
            u = np.stack([xb[:, 0] / r, xb[:, 1] / r], -1)
            dr, dz = r - d[0], az - d[1]
            inside = (dr <= 0) & (dz <= 0)
            cap = inside & (-dz < -dr)    # the barrel wins a tie
            orr, oz = np.maximum(dr, 0), np.maximum(dz, 0)
            lo = np.sqrt(orr ** 2 + oz ** 2)
            phi = np.where(inside, np.where(cap, dz, dr), lo)
            gr = np.where(inside, np.where(cap, T(0), T(1)), orr / lo)
            gz = np.where(inside, np.where(cap, sz, T(0)), sz * oz / lo)
            g = np.stack([gr * u[:, 0], gr * u[:, 1], gz], -1)
        elif b.kind == ELLIPSOID:
            # membership by the implicit function (the pair generator's predicate); the gradient from the exact nearest
            # point, solved in double from the T-rounded inputs (the engine's solve is FP64 too) and rounded to T
            phi = ((xb / d) ** 2).sum(-1) - T(1)
            if normals:
                g = _ellipsoid_normal(xb.astype(F64), d.astype(F64)).astype(T)
        else:
            vals, n, lo, cell = b.lattice
            if T is F64:
                phi, g, _ = smr.interpolant(vals, n, lo, cell, xb)
            else:
                phi, g = _interpolant32(vals, n, lo, cell, xb)
    return phi.astype(T), (g.astype(T) @ R.T).astype(T)


def _interpolant32(values, n, lo, cell, xb):
    """sdf_mesh_reference.interpolant with every operation in float32 (the header's formulas, mpm_sdf_collider_t)"""
    T = F32
    xb = np.asarray(xb, T)
    lo = np.asarray(lo, T)
    n = np.asarray(n)
    hi = (lo + (n - 1).astype(T) * T(cell)).astype(T)
    q = np.clip(xb, lo, hi)
    t = ((q - lo) * (T(1) / T(cell))).astype(T)
    i = np.minimum(np.floor(t).astype(np.int64), n - 2)
    f = np.minimum(t - i.astype(T), T(1)).astype(T)
    V = np.asarray(values, T)
    c = {(dx, dy, dz): V[i[:, 2] + dz, i[:, 1] + dy, i[:, 0] + dx] for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)}
    fx, fy, fz = f[:, 0], f[:, 1], f[:, 2]
    a = {(dy, dz): c[0, dy, dz] + fx * (c[1, dy, dz] - c[0, dy, dz]) for dy in (0, 1) for dz in (0, 1)}
    b0, b1 = a[0, 0] + fy * (a[1, 0] - a[0, 0]), a[0, 1] + fy * (a[1, 1] - a[0, 1])
    tri = b0 + fz * (b1 - b0)
    d = xb - q
    out = _norm(d)
    ex = {(dy, dz): c[1, dy, dz] - c[0, dy, dz] for dy in (0, 1) for dz in (0, 1)}
    ex0, ex1 = ex[0, 0] + fy * (ex[1, 0] - ex[0, 0]), ex[0, 1] + fy * (ex[1, 1] - ex[0, 1])
    gx = ex0 + fz * (ex1 - ex0)
    ey0, ey1 = a[1, 0] - a[0, 0], a[1, 1] - a[0, 1]
    gy = ey0 + fz * (ey1 - ey0)
    gz = b1 - b0
    g = np.where((out > 0)[:, None], d, np.stack([gx, gy, gz], 1)).astype(T)
    nn = (g * g).sum(-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        g = np.where((nn > T(1e-30))[:, None], g / np.sqrt(nn)[:, None], np.array([0, 0, 1], T))
    return (tri + out).astype(T), g.astype(T)


def rigid_velocity(b, x, T=F64):
    """v_c(x) = v + w x (x - p_WB)"""
    r = np.asarray(x, T) - b.p.astype(T)
    w, v = b.w.astype(T), b.v.astype(T)
    return np.stack([v[0] + (w[1] * r[:, 2] - w[2] * r[:, 1]), v[1] + (w[2] * r[:, 0] - w[0] * r[:, 2]),
                     v[2] + (w[0] * r[:, 1] - w[1] * r[:, 0])], -1).astype(T)


# ---- the update -----------------------------------------------------------------------------------------------------------
def node_positions(bits, idx=None):
    """x = (idx + 0.5) dx of the cells `idx` (all cells when None), exact in float32 and float64"""
    xyz = tl.key_coords(bits)
    if idx is not None:
        xyz = xyz[idx]
    return (xyz.astype(F64) + 0.5) / float(1 << bits)


def walls(m, mv, bits, T=F64, wall=WALL):
    """v = mv / m and the domain walls (transfer_layouts.grid64 / grid32)"""
    return (tl.grid64 if T is F64 else tl.grid32)(m, mv, bits, wall).astype(T)


def apply_mode(b, v_in, vc, n, T=F64):
    """the three modes of the grid update for one body at nodes with velocity v_in, body velocity vc and unit normal n"""
    v_in, vc, n = (np.asarray(a, T) for a in (v_in, vc, n))
    dv = (vc - v_in).astype(T)
    dn = (n * dv).sum(-1).astype(T)
    if b.mode == FIXED:
        return vc.copy()
    fr = T(b.friction)
    frac = (dn.astype(F64) * (1.0 - F64(b.friction))).astype(T)     # (a double product in the reference, :783-786)
    out = (v_in + (dv * fr + n * frac[:, None])).astype(T)
    if b.mode == SLIP_APPROACHING:
        out = np.where((dn > 0)[:, None], out, v_in)
    return out.astype(T)


def reference(m, mv, bits, bodies, n_acc, T=F64, decider=None, wall=WALL):
    """The grid update with rigid bodies.  m (n_cells,), mv (n_cells, 3): the node sums after ParticleToGrid.
    -> dict: on (indices of the nodes with mass), x, v_in (after the walls), v (written; v* is the same vector),
    decider (index into `bodies`, -1: none), vc (the deciding body's velocity at the node, 0 where none),
    imp (n_acc, 6): per accumulator (tau, f) sums in float64, absl (n_acc,): sum of |l| of its nodes.
    `decider`: take membership from another evaluation (the float32 yardstick takes the float64 one's)."""
    m = np.asarray(m)
    on = np.nonzero(m > 0)[0]
    x = node_positions(bits, on)
    v_in = walls(m, mv, bits, T, wall)[on]
    v = v_in.copy()
    vc_all = np.zeros_like(v)
    if decider is None:
        decider = np.full(len(on), -1)
        for k, b in enumerate(bodies):
            free = decider < 0
            phi, _ = body_sdf(b, x[free], F64, normals=False)
            idx = np.nonzero(free)[0][phi < 0]
            decider[idx] = k
    for k, b in enumerate(bodies):
        sel = np.nonzero(decider == k)[0]
        if not len(sel):
            continue
        _, n = body_sdf(b, x[sel], T)
        vc = rigid_velocity(b, x[sel], T)
        vc_all[sel] = vc
        v[sel] = apply_mode(b, v_in[sel], vc, n, T)
    imp, absl = np.zeros((n_acc, 6)), np.zeros(n_acc)
    mass = np.asarray(m, T)[on].astype(F64)
    for k, b in enumerate(bodies):
        sel = np.nonzero(decider == k)[0]
        if b.body >= n_acc or not len(sel):
            continue
        # (the products of the reaction are formed in double by the engine, from its float velocities: here from T's)
        l = -mass[sel, None] * (v[sel].astype(F64) - v_in[sel].astype(F64))
        r = x[sel] - b.p.astype(F64)
        imp[b.body, :3] += np.cross(r, l).sum(0)
        imp[b.body, 3:] += l.sum(0)
        absl[b.body] += _norm(l).sum()
    return dict(on=on, x=x, v_in=v_in, v=v, decider=decider, vc=vc_all, imp=imp, absl=absl)


def undecided(bodies, x, decider):
    """Nodes where float and double may disagree about membership or the normal: for any body up to and including the
    deciding one (every body when none decides) phi < 0 differs among the seven points x, x +- DELTA e_a, or the deciding
    body's normal differs by more than NORMAL_TOL in a component among them."""
    x = np.asarray(x, F64)
    probes = [np.zeros(3)] + [s * DELTA * np.eye(3)[a] for a in range(3) for s in (1, -1)]
    und = np.zeros(len(x), bool)
    last = np.where(decider < 0, len(bodies) - 1, decider)
    for k, b in enumerate(bodies):
        sel = np.nonzero(last >= k)[0]
        if not len(sel):
            continue
        mine = decider[sel] == k
        inside0, n0 = None, None
        for q in probes:
            phi, n = body_sdf(b, x[sel] + q, F64, normals=False)
            ins = phi < 0
            if inside0 is None:
                inside0 = ins
            und[sel] |= ins != inside0
        if mine.any():
            s2 = sel[mine]
            for q in probes:
                _, n = body_sdf(b, x[s2] + q, F64)
                if n0 is None:
                    n0 = n
                with np.errstate(invalid="ignore"):
                    und[s2] |= ~(np.abs(n - n0).max(-1) <= NORMAL_TOL)
    return und


def check_scene_conditions(bodies, x, decider, und):
    """the conditions of the comparison: -> (share of undecided among the nodes inside some body, {(kind, mode): compared})"""
    inside = decider >= 0
    share = float((und & inside).sum()) / max(int(inside.sum()), 1)
    counts = {}
    for k, b in enumerate(bodies):
        key = (KIND_NAMES[b.kind], b.mode)
        counts[key] = counts.get(key, 0) + int(((decider == k) & ~und).sum())
    return share, counts


# ---- scenes -----------------------------------------------------------------------------------------------------------------
BITS = 7


def slab(bits=BITS, center=(0.5, 0.5, 0.5), side=0.3, thickness=0.2, seed=11, v0=(0.0, 0.0, -0.5), vel_amp=0.3, pitch=0.9):
    """A block of cloth: horizontal sheets `pitch` cells apart in every direction, so that every grid node inside the block
    carries mass (a cloth only loads a shell of nodes; the bodies need several layers).  -> [(pos, vel, idx)]"""
    dx = 1.0 / (1 << bits)
    res = int(round(side / (pitch * dx)))
    layers = max(int(round(thickness / (pitch * dx))), 1)
    out = []
    for k in range(layers):
        z = center[2] - 0.5 * thickness + (k + 0.5) * thickness / layers
        pos, idx = scenes.cloth_sheet(res, side, z, center[:2])
        n = len(pos)
        j = np.stack([scenes.hash_uniform(seed, n, 6 * k + c) for c in range(3)], -1)
        u = np.stack([scenes.hash_uniform(seed, n, 6 * k + 3 + c) for c in range(3)], -1)
        pos = (pos + F32(0.05 * side / res) * j).astype(F32)
        vel = (np.asarray(v0, F32) + F32(vel_amp) * u).astype(F32)
        out.append((pos, vel, idx))
    return out


def massive_nodes(sheets, bits):
    """the cells ParticleToGrid gives mass to, predicted without an engine: the 27-node stencils of every vertex and of
    every face's centroid"""
    pts = []
    for pos, _, idx in sheets:
        pts.append(pos.astype(F64))
        pts.append(pos[idx.reshape(-1, 3)].astype(F64).mean(1))
    base, _ = tl.base_cells(np.concatenate(pts), bits)
    base = np.unique(base, axis=0)
    keys = [tl.cell_key(base[:, 0] + o[0], base[:, 1] + o[1], base[:, 2] + o[2]) for o in tl.OFFSETS]
    return np.unique(np.concatenate(keys))


_V, _W = (0.1, -0.05, 0.2), (1.0, -2.0, 1.5)
_C = (0.5, 0.5, 0.5)


def _kind_body(kind, mode):
    """one body per kind, posed with a rotation that is not axis-aligned, v and w non-zero"""
    common = dict(body=0, p=_C, v=_V, w=_W, mode=mode, friction=0.3)
    if kind == HALF_SPACE:
        return Body(HALF_SPACE, R=rot((1, 0.4, 0.1), 0.2), **common)
    if kind == SPHERE:
        return Body(SPHERE, R=rot((0.3, 1, 0.2), 0.9), dims=(0.06, 0, 0), **common)
    if kind == BOX:
        return Body(BOX, R=rot((1, 2, 0.5), 0.7), dims=(0.11, 0.07, 0.05), **common)
    if kind == CAPSULE:
        return Body(CAPSULE, R=rot((0.2, 1, 1), 2.1), dims=(0.04, 0.09, 0), **common)
    if kind == CYLINDER:
        return Body(CYLINDER, R=rot((1, 0.3, 0.2), 1.1), dims=(0.07, 0.05, 0), **common)
    if kind == ELLIPSOID:
        return Body(ELLIPSOID, R=rot((0.5, -1, 0.7), 0.8), dims=(0.10, 0.06, 0.045), **common)
    return Body(MESH, R=rot((1, -0.6, 0.3), 0.6), mesh=smr.icosphere(0.07, 2), cell=0.01, pad=2, **common)


def kind_scene(kind):
    """-> (sheets, {mode: [body]}): one engine state, the three modes of one body of `kind`"""
    return slab(), {mode: [_kind_body(kind, mode)] for mode in (FIXED, SLIP_APPROACHING, SLIP)}


def overlap_scene():
    """Five bodies that overlap, in an order that matters: a sphere inside a box, a capsule through both, a cylinder
    next to them and a tilted half-space under everything; a different accumulator each, one out of range."""
    bodies = [
        Body(SPHERE, body=0, p=(0.5, 0.5, 0.52), R=rot((0.3, 1, 0.2), 0.9), dims=(0.06, 0, 0), v=_V, w=_W, mode=SLIP, friction=0.3),
        Body(BOX, body=1, p=(0.5, 0.5, 0.5), R=rot((1, 2, 0.5), 0.7), dims=(0.11, 0.07, 0.05), v=(0, 0.1, 0), w=(0, 0, 2.0), mode=FIXED),
        Body(CAPSULE, body=2, p=(0.47, 0.52, 0.5), R=rot((0.2, 1, 1), 2.1), dims=(0.04, 0.09, 0), v=(0.05, 0, 0.1), w=(1, 0, 0),
             mode=SLIP_APPROACHING, friction=0.6),
        Body(CYLINDER, body=7, p=(0.58, 0.45, 0.5), R=rot((1, 0.3, 0.2), 1.1), dims=(0.07, 0.05, 0), v=(0, 0, 0.3), w=(0.5, 0.5, -1),
             mode=SLIP, friction=0.0),
        Body(HALF_SPACE, body=3, p=(0.5, 0.5, 0.44), R=rot((1, 0.4, 0.1), 0.2), v=(0, 0, 0.05), w=(0, 0, 0), mode=SLIP, friction=1.0),
    ]
    return slab(seed=13), {"overlap": bodies}


SCENES = {KIND_NAMES[k]: (lambda k=k: kind_scene(k)) for k in range(7)}
SCENES["overlap"] = overlap_scene
N_ACC = 4    # accumulators of every scene (the overlap scene's cylinder, body 7, is out of range on purpose)
