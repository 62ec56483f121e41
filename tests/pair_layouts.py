"""Particle layouts that reach every branch of the device-side contact front end (k_ct_gen_count_scan, k_ct_gen_write and
k_ct_watch of drake_amd/csrc/mpm_contact_dev.h, with sdf_closed / collider_inside / collider_near under them), float64
restatements of the signed distances, and rounding bounds.  CPU only: nothing here imports the engine.

Layouts
-------
A layout is a rest mesh of T disconnected triangles plus E vertices that belong to no face (np = 4 T + E particles, any
number), the state to upload in the engine's original order (all faces, then all vertices) and a list of colliders (Col:
float32 pose, dims and spatial velocity).  The generator reads an uploaded face position as it is, so outside the `watch`
layout every particle with mass -- a face or a triangle's corner -- is simply a point.  A vertex in no face is a particle
without mass: the generator counts only particles with mass (q.w > 0, the test that keeps a partitioned domain's ghost
copies out), so it makes no pair wherever it is; the layouts put some inside colliders and expect none.  They come first
among the vertices, so that the last particle has mass.  Everything is seeded.  `claims` lists (text, check) of what a layout is built to
reach; tests/test_pair_layouts.py evaluates every check with the restatements below.

    features     kinds 0-5 under generic rotated poses with v, w != 0; particles aimed at every feature of every kind,
                 inside and outside at depths DEPTHS x dx; all decided, gradient ties at least TIE_BAND away
    conventions  identity pose, p_WB = 0 (body coordinates are the world's, exactly): the sphere's centre, a point on the
                 capsule's axis segment, the box's interior ties and a coordinate exactly 0, the cylinder's axis and ties
    shell        kinds 0-4: 256 points each within +-4 ulp per coordinate of the surface (membership undecidable by design)
    blocks       np in BLOCK_NP, four small spheres about each particle at the scan's structural slots (24 colliders for six
                 slots), 1, 2 or all 4 of them containing it (the others miss it by a decided margin); everything else far
                 from every collider
    tables       16 and 17 analytic colliders that all contain one particle, with and without an ellipsoid among them
    empty        colliders that contain nothing
    watch        ~2000 particles far from the colliders; the states of the watch tests are made from it by moving one vertex
                 or one triangle (watch_state)

Restatements (float64, numpy, from the float32 pose, dims and point)
---------------------------------------------------------------------
world_sdf64   phi and the world gradient R gb of kinds 0-5 with the conventions of sdf_closed / sdf_ellipsoid: body
              coordinates xb = R^T (x - p); sphere and capsule +z_B at length 0; box inside: the first maximal axis,
              Sign(0) = +1; the cylinder of Drake's (r, z) cross-section box; the ellipsoid by Eberly's bisection
mesh_sdf64    tests/sdf_mesh_reference.interpolant on a downloaded lattice
rigid_v64     v + w x (x - p_WB)

Bounds (u = 2^-24, the unit roundoff of float32; |.| the Euclidean length unless indexed)
------------------------------------------------------------------------------------------
Body coordinates.  d = fl(x - p) carries u |d_i| per component; xb_k = R_0k d_0 + R_1k d_1 + R_2k d_2 is three products and
two sums (or one product and two fused multiply-adds: fewer roundings), at most 3 u sum_i |R_ik| |d_i| more; the columns
of R are unit vectors, so per coordinate  e_k = 4 u |d|  and as a vector  e = 4 sqrt(3) u |d|.  phi is 1-Lipschitz in xb.
    phi   kind 0   e_k                                                 (one coordinate, nothing else)
          kind 1   e + 3 u len + u |phi|                               (three squares and two sums under a root: 3 u; len - r)
          kind 2   e + u |q| + 3 u |phi|                               (q = |xb| - h; outside the root of the squares of o)
          kind 3   e + u (|z| + h) + 3 u len + u |phi|                 (z - clamp(z); then as the sphere)
          kind 4   e + 3 u r + u (r + R) + u (|z| + h) + 3 u |phi|     (r; r - R; |z| - h; the root or the weighted sum)
                   + 2 sqrt(2) CYL_TOL max(1, R, h) within twice the error of r or |z| of a threshold of the boundary class
                   (float and double may classify a coordinate differently there; the branches differ by at most the band)
          kind 5   membership (the implicit function in float32): e + 4 u max a_i   (g = sum (xb_i / a_i)^2 to 4 u near 1,
                   |grad g| >= 2 / max a_i on the surface); the distance itself is solved in float64 from x - p in
                   float64 and rounded once: 2 u |phi| + 2^-30 max a_i
          mesh     e + 8 u (max |corner value| + extent of the lattice box)      (clamp, scale, three nested lerps)
    grad  (largest component of the world gradient's error)  gb's error as a vector, plus 6 u for R gb (three products
          and two sums over terms that add up to at most sqrt(3)):
          kind 0, box inside, cylinder cap inside: 6 u     kinds 1, 3: (e + u (|z| + h)) / len + 4 u + 6 u
          box outside: (e + u |q|) / phi + 4 u + 6 u
          cylinder: the radial unit vector e / r + 3 u where it is used, outside also (e + u (2 r + R + |z| + h)) / phi + 4 u
          kind 5: 8 u     mesh: see mesh_bounds (the interpolant's own change over the coordinate error)
          Not covered, and excluded from gradient checks (grad_ok): the box's inside within 2 (e_k + u |q|) of a tie of its
          two largest q, the cylinder's inside within the same of its cap/barrel tie, of its axis and of the boundary
          class, the ellipsoid's inside within 1e-3 min a_i of the plane of its shortest axis.
    rigid_v  per component 4 u (max |v_i| + 2 max |w_i| max |r_i|)    (r = x - p; two products, a difference, a sum)
These are bounds of the arithmetic, not fits: tests/test_pair_layouts.py evaluates a float32 numpy restatement of the device
code both with separate multiplies and adds and with the fused order the device compiles to (fma(R6, d2, fma(R0, d0,
R3 d1)) and the like, the FMA emulated through float64) on every layout and requires it inside the bounds; the measured
worst ratios per layout, kind and field go to tests.helpers.MARGINS.

Classification of a (particle, collider): decided in when phi64 < -DECIDE x bound, decided out when phi64 > +DECIDE x
bound, undecidable otherwise (DECIDE = 8).
"""
import numpy as np

from tests import sdf_mesh_reference as meshref

F = np.float32
D = np.float64
U32 = 2.0 ** -24
CYL_TOL = 4 * np.finfo(np.float32).eps     # the device's float-sized stand-in for Drake's 1e-14 (mpm_contact_dev.h)
DECIDE = 8.0
DEPTHS = (0.5, 1e-2, 1e-4)                 # x dx
TIE_BAND = 0.1                             # x dx: how far `features` stays from every gradient tie
WATCH_MARGIN = 1e-3                        # x dx (k_ct_watch)
BLOCK_NP = (4095, 4096, 4097, 8192, 8193)
POISON_BODY = 0                            # the body of the half-space that poisons the pair buffers; test bodies are 1 ..
KIND_NAMES = ("half-space", "sphere", "box", "capsule", "cylinder", "ellipsoid")


def rot(axis, angle):
    axis = np.asarray(axis, D) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return (np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K).astype(F)


class Col:
    """a collider as the engine gets it: everything float32"""

    def __init__(self, kind, body, p=(0, 0, 0), R=None, dims=(0, 0, 0), v=(0, 0, 0), w=(0, 0, 0)):
        self.kind, self.body = int(kind), int(body)
        self.p = np.asarray(p, F)
        self.R = np.eye(3, dtype=F) if R is None else np.asarray(R, F).reshape(3, 3)
        self.dims, self.v, self.w = np.asarray(dims, F), np.asarray(v, F), np.asarray(w, F)

    def world(self, xb):
        """body-frame points (float64) -> world (float64)"""
        return np.asarray(xb, D) @ self.R.astype(D).T + self.p.astype(D)


# ---- float64 restatements ------------------------------------------------------------------------------------------

def sdf_cylinder(xb, R, h):
    """Drake's cylinder: the (r, z) box [-R, R] x [-h, h], coordinates classified inside / boundary / outside."""
    xb = np.asarray(xb, np.float64)
    r = np.hypot(xb[:, 0], xb[:, 1])
    z = xb[:, 2]
    az = np.abs(z)
    sz = np.where(z < 0, -1.0, 1.0)
    tr, tz = CYL_TOL * max(1.0, R), CYL_TOL * max(1.0, h)
    axis = r < tr
    with np.errstate(invalid="ignore", divide="ignore"):
        ux = np.where(axis, 1.0, xb[:, 0] / r)
        uy = np.where(axis, 0.0, xb[:, 1] / r)
    out_r, out_z = r > R + tr, az > h + tz
    bnd_r, bnd_z = ~out_r & (r >= R - tr), ~out_z & (az >= h - tz)
    outside = out_r | out_z
    boundary = ~outside & (bnd_r | bnd_z)
    cap = ~outside & ~boundary & (h - az < R - r)
    dr = np.where(out_r | bnd_r, r - R, 0.0)
    dz = np.where(out_z | bnd_z, sz * (az - h), 0.0)
    lo = np.hypot(dr, dz)
    w = np.where(bnd_r & bnd_z, np.sqrt(0.5), 1.0)
    phi = np.where(outside, lo, np.where(boundary, np.where(bnd_r, w * (r - R), 0) + np.where(bnd_z, w * (az - h), 0),
                                         np.where(cap, az - h, r - R)))
    with np.errstate(invalid="ignore", divide="ignore"):
        gr = np.where(outside, dr / lo, np.where(boundary, np.where(bnd_r, w, 0.0), np.where(cap, 0.0, 1.0)))
        gz = np.where(outside, dz / lo, np.where(boundary, np.where(bnd_z, w * sz, 0.0), np.where(cap, sz, 0.0)))
    return phi, np.stack([gr * ux, gr * uy, gz], 1)


def sdf_ellipsoid(xb, radii, iters=200):
    """Eberly: axes sorted descending, the query in the first octant, the secular equation's root by bisection
    (vectorised; no coordinate may be exactly zero)."""
    xb = np.asarray(xb, np.float64)
    a = np.asarray(radii, np.float64)
    order = np.argsort(-a, kind="stable")
    e = a[order]
    y = np.abs(xb[:, order])
    z = y / e
    g = (z * z).sum(1) - 1
    r = (e / e[2]) ** 2
    n = r * z
    s0 = z[:, 2] - 1
    s1 = np.where(g < 0, 0.0, np.sqrt(n[:, 0] ** 2 + n[:, 1] ** 2 + z[:, 2] ** 2) - 1)
    for _ in range(iters):
        s = 0.5 * (s0 + s1)
        gs = (n[:, 0] / (s + r[0])) ** 2 + (n[:, 1] / (s + r[1])) ** 2 + (z[:, 2] / (s + 1)) ** 2 - 1
        s0 = np.where(gs > 0, s, s0)
        s1 = np.where(gs < 0, s, s1)
    s = 0.5 * (s0 + s1)
    x = r * y / (s[:, None] + r)
    x = np.where((g == 0)[:, None], y, x)
    dist = np.linalg.norm(x - y, axis=1)
    N = np.empty_like(x)
    N[:, order] = x
    N = np.sign(xb) * N
    grad = N / (a * a)
    grad /= np.linalg.norm(grad, axis=1)[:, None]
    return np.where(g < 0, -dist, dist), grad


def _unit_or_z(r, ln):
    with np.errstate(invalid="ignore", divide="ignore"):
        g = r / ln[:, None]
    return np.where((ln > 0)[:, None], g, np.array([0.0, 0.0, 1.0]))


def sdf_body64(kind, xb, dims):
    """phi and the body-frame unit gradient of kinds 0-5 at body-frame points xb (n, 3), float64, sdf_closed's conventions"""
    xb = np.asarray(xb, D)
    dims = np.asarray(dims, D)
    n = len(xb)
    if kind == 0:
        return xb[:, 2].copy(), np.tile([0.0, 0.0, 1.0], (n, 1))
    if kind == 1:
        ln = np.sqrt((xb * xb).sum(1))
        return ln - dims[0], _unit_or_z(xb, ln)
    if kind == 2:
        q = np.abs(xb) - dims
        sg = np.where(xb < 0, -1.0, 1.0)
        m = q.max(1)
        a = np.where((q[:, 0] >= q[:, 1]) & (q[:, 0] >= q[:, 2]), 0, np.where(q[:, 1] >= q[:, 2], 1, 2))
        gi = np.zeros((n, 3))
        gi[np.arange(n), a] = sg[np.arange(n), a]
        o = np.maximum(q, 0)
        lo = np.sqrt((o * o).sum(1))
        with np.errstate(invalid="ignore", divide="ignore"):
            go = sg * o / lo[:, None]
        inside = m <= 0
        return np.where(inside, m, lo), np.where(inside[:, None], gi, go)
    if kind == 3:
        zc = np.clip(xb[:, 2], -dims[1], dims[1])
        r = xb.copy()
        r[:, 2] -= zc
        ln = np.sqrt((r * r).sum(1))
        return ln - dims[0], _unit_or_z(r, ln)
    if kind == 4:
        return sdf_cylinder(xb, float(dims[0]), float(dims[1]))
    return sdf_ellipsoid(xb, dims)


def body64(c, x):
    d = np.asarray(x, D) - c.p.astype(D)
    return d @ c.R.astype(D), d


def world_sdf64(c, x):
    xb, _ = body64(c, x)
    phi, gb = sdf_body64(c.kind, xb, c.dims)
    return phi, gb @ c.R.astype(D).T


def rigid_v64(c, x):
    return c.v.astype(D) + np.cross(c.w.astype(D), np.asarray(x, D) - c.p.astype(D))


def mesh_sdf64(lattice, col_p, col_R, x):
    """(phi, world gradient, lattice coordinate t): the documented interpolant of a downloaded lattice
    (values, n, lo, cell) under the float32 pose (col_p, col_R)"""
    values, n, lo, cell = lattice
    R = np.asarray(col_R, F).astype(D).reshape(3, 3)
    xb = (np.asarray(x, D) - np.asarray(col_p, F).astype(D)) @ R
    phi, gb, t = meshref.interpolant(values, n, lo, cell, xb)
    return phi, gb @ R.T, t


# ---- bounds ----------------------------------------------------------------------------------------------------------

def coord_error(c_p, x):
    """(e_k, e): the error of a body coordinate and of the body-frame point (module docstring)"""
    d = np.linalg.norm(np.asarray(x, D) - np.asarray(c_p, F).astype(D), axis=1)
    return 4 * U32 * d, 4 * np.sqrt(3.0) * U32 * d


def bounds(c, x):
    """dict(phi, grad, rv, grad_ok, val): per-point bounds of the module docstring for collider c at world points x.
    phi: the bound that classifies (and, but for the ellipsoid, bounds dist); val: the bound on dist"""
    u = U32
    xb, d = body64(c, x)
    ek, e = coord_error(c.p, x)
    phi, _ = sdf_body64(c.kind, xb, c.dims)
    aphi = np.abs(phi)
    dims = c.dims.astype(D)
    n = len(xb)
    ok = np.ones(n, bool)
    rot6 = 6 * u
    if c.kind == 0:
        bphi, bg = ek, np.full(n, rot6)
    elif c.kind == 1:
        ln = np.linalg.norm(xb, axis=1)
        bphi = e + 3 * u * ln + u * aphi
        with np.errstate(divide="ignore", invalid="ignore"):
            bg = e / ln + 4 * u + rot6
        ok = ln > 0
    elif c.kind == 2:
        q = np.abs(xb) - dims
        qn = np.linalg.norm(q, axis=1)
        bphi = e + u * qn + 3 * u * aphi
        inside = q.max(1) <= 0
        with np.errstate(divide="ignore", invalid="ignore"):
            bg = np.where(inside, rot6, (e + u * qn) / aphi + 4 * u + rot6)
        qs = np.sort(q, axis=1)
        ok = ~(inside & (qs[:, 2] - qs[:, 1] <= 2 * (ek + u * qn)))
    elif c.kind == 3:
        z, h = xb[:, 2], dims[1]
        r = xb.copy()
        r[:, 2] -= np.clip(z, -h, h)
        ln = np.linalg.norm(r, axis=1)
        own = u * (np.abs(z) + h)
        bphi = e + own + 3 * u * ln + u * aphi
        with np.errstate(divide="ignore", invalid="ignore"):
            bg = (e + own) / ln + 4 * u + rot6
        ok = ln > 0
    elif c.kind == 4:
        R, h = dims[0], dims[1]
        r, az = np.hypot(xb[:, 0], xb[:, 1]), np.abs(xb[:, 2])
        tol = CYL_TOL * max(1.0, R, h)
        own = 3 * u * r + u * (r + R) + u * (az + h)
        near = np.zeros(n, bool)
        for val, edge in ((r, R), (az, h)):
            for s in (-1.0, 1.0):
                near |= np.abs(val - (edge + s * CYL_TOL * max(1.0, edge))) <= 2 * (e + own)
        bphi = e + own + 3 * u * aphi + np.where(near, 2 * np.sqrt(2.0) * tol, 0.0)
        near |= r <= tol + 2 * (e + own)       # (the axis: the gradient's radial direction only)
        outside = (r > R) | (az > h)
        cap = ~outside & (h - az < R - r)
        with np.errstate(divide="ignore", invalid="ignore"):
            radial = e / r + 3 * u
            bg = np.where(outside, (e + own) / aphi + 4 * u + radial, np.where(cap, 0.0, radial)) + rot6
        tie = ~outside & (np.abs((h - az) - (R - r)) <= 2 * (ek + own))
        ok = ~(near | tie)
    else:
        amax, amin = dims.max(), dims.min()
        bphi = e + 4 * u * amax
        bg = np.full(n, 8 * u)
        g = ((xb / dims) ** 2).sum(1)
        ok = ~((g < 1) & (np.abs(xb[:, int(np.argmin(dims))]) < 1e-3 * amin))
    val = 2 * u * aphi + 2.0 ** -30 * dims.max() if c.kind == 5 else bphi
    r_ = np.abs(d).max(1)
    brv = 4 * u * (np.abs(c.v.astype(D)).max() + 2 * np.abs(c.w.astype(D)).max() * r_)
    return dict(phi=bphi, val=val, grad=np.where(ok, bg, np.inf), rv=np.full((n,), 1.0) * brv, grad_ok=ok)


def mesh_bounds(lattice, col_p, col_R, x):
    """dict(phi, grad, grad_ok) for a mesh collider: phi as in the module docstring; grad: the interpolant's own change
    when the body-frame point moves by the coordinate error along any axis (its gradient is piecewise smooth: points
    within 1e-3 of a cell face or 1e-5 of the lattice box's surface are excluded), plus the roundings of the differences
    of corner values against the gradient's length (32 u max |corner| / cell) and 6 u for R gb"""
    values, n, lo, cell = lattice
    ek, e = coord_error(col_p, x)
    lo64 = np.asarray(lo, D)
    hi64 = lo64 + (np.asarray(n) - 1) * D(cell)
    ext = float((hi64 - lo64).max())
    cmax = float(np.abs(values).max())
    bphi = e + 8 * U32 * (cmax + ext)
    R = np.asarray(col_R, F).astype(D).reshape(3, 3)
    xb = (np.asarray(x, D) - np.asarray(col_p, F).astype(D)) @ R
    _, g0, t = meshref.interpolant(values, n, lo, cell, xb)
    bg = np.zeros(len(xb))
    for a in range(3):
        for s in (-1.0, 1.0):
            y = xb.copy()
            y[:, a] += s * ek
            bg = np.maximum(bg, np.abs(meshref.interpolant(values, n, lo, cell, y)[1] - g0).max(1))
    frac = np.abs(t - np.round(t)).min(1)
    gap = np.linalg.norm(np.clip(xb, lo64, hi64) - xb, axis=1)
    depth = np.minimum(xb - lo64, hi64 - xb).min(1)
    ok = (gap > 1e-5) | ((depth > 1e-5) & (frac > 1e-3))
    return dict(phi=bphi, val=bphi, grad=np.where(ok, 2 * bg + 32 * U32 * cmax / float(cell) + 6 * U32, np.inf), grad_ok=ok)


def classify(phi64, bound):
    """(decided in, decided out)"""
    return phi64 < -DECIDE * bound, phi64 > DECIDE * bound


def evaluate(lay):
    """per collider of the layout: dict(phi, grad, rv, b (bounds), din, dout) at every particle (original order)"""
    out = []
    for c in lay["cols"]:
        phi, grad = world_sdf64(c, lay["pos"])
        b = bounds(c, lay["pos"])
        din, dout = classify(phi, b["phi"])
        # (a particle without mass makes no pair, wherever it is)
        din, dout = din & ~lay["massless"], dout | lay["massless"]
        out.append(dict(phi=phi, grad=grad, rv=rigid_v64(c, lay["pos"]), b=b, din=din, dout=dout))
    return out


def margin(err, bound):
    """the worst ratio err / bound over the entries with a finite bound (0 when there is none)"""
    err, bound = np.broadcast_arrays(np.asarray(err, D), np.asarray(bound, D))
    m = np.isfinite(bound)
    if not m.any():
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err[m] == 0, 0.0, err[m] / bound[m])
    return float(r.max())


# ---- the float32 restatement of the device code, in both contraction orders ---------------------------------------------

class Ops32:
    """float32 arithmetic on numpy arrays; `fused`: sums of products the way the device contracts them"""

    def __init__(self, fused):
        self.fused = fused

    @staticmethod
    def fma(a, b, c):
        return (np.asarray(a, F).astype(D) * np.asarray(b, F).astype(D) + np.asarray(c, F).astype(D)).astype(F)

    def dot(self, a, b):
        """a0 b0 + a1 b1 (+ a2 b2) in the device's order"""
        a = [np.asarray(t, F) for t in a]
        b = [np.asarray(t, F) for t in b]
        if not self.fused:
            s = a[0] * b[0] + a[1] * b[1]
            return s + a[2] * b[2] if len(a) == 3 else s
        s = self.fma(a[0], b[0], a[1] * b[1])
        return self.fma(a[2], b[2], s) if len(a) == 3 else s


def body32(c, x, ops):
    x = np.asarray(x, F)
    d = x - c.p
    R = c.R.reshape(-1)
    return np.stack([ops.dot((R[k], R[3 + k], R[6 + k]), (d[:, 0], d[:, 1], d[:, 2])) for k in range(3)], 1), d


def sdf_body32(kind, xb, dims, ops):
    """sdf_closed (kinds 0-4) in float32"""
    dims = np.asarray(dims, F)
    n = len(xb)
    x, y, z = xb[:, 0], xb[:, 1], xb[:, 2]
    zero, one = np.zeros(n, F), np.ones(n, F)
    with np.errstate(invalid="ignore", divide="ignore"):
        if kind == 0:
            return z.copy(), np.stack([zero, zero, one], 1)
        if kind in (1, 3):
            r2 = z - np.clip(z, -dims[1], dims[1]) if kind == 3 else z
            ln = np.sqrt(ops.dot((x, y, r2), (x, y, r2)))
            g = np.stack([x / ln, y / ln, r2 / ln], 1)
            return ln - dims[0], np.where((ln > 0)[:, None], g, np.array([0, 0, 1], F)).astype(F)
        if kind == 2:
            q = np.abs(xb) - dims
            sg = np.where(xb < 0, F(-1), F(1))
            m = q.max(1)
            a = np.where((q[:, 0] >= q[:, 1]) & (q[:, 0] >= q[:, 2]), 0, np.where(q[:, 1] >= q[:, 2], 1, 2))
            gi = np.zeros((n, 3), F)
            gi[np.arange(n), a] = sg[np.arange(n), a]
            o = np.maximum(q, F(0))
            lo = np.sqrt(ops.dot((o[:, 0], o[:, 1], o[:, 2]), (o[:, 0], o[:, 1], o[:, 2])))
            go = sg * o / lo[:, None]
            inside = m <= 0
            return np.where(inside, m, lo).astype(F), np.where(inside[:, None], gi, go).astype(F)
        R, h = dims[0], dims[1]
        r, az = np.sqrt(ops.dot((x, y), (x, y))), np.abs(z)
        tr, tz = F(CYL_TOL) * max(F(1), R), F(CYL_TOL) * max(F(1), h)
        sz = np.where(z < 0, F(-1), F(1))
        axis = r < tr
        ux, uy = np.where(axis, one, x / r), np.where(axis, zero, y / r)
        out_r, out_z = r > R + tr, az > h + tz
        bnd_r, bnd_z = ~out_r & (r >= R - tr), ~out_z & (az >= h - tz)
        outside = out_r | out_z
        boundary = ~outside & (bnd_r | bnd_z)
        cap = ~outside & ~boundary & (h - az < R - r)
        dr = np.where(out_r | bnd_r, r - R, zero)
        dz = np.where(out_z | bnd_z, sz * (az - h), zero)
        lo = np.sqrt(ops.dot((dr, dz), (dr, dz)))
        w = np.where(bnd_r & bnd_z, F(0.70710678), F(1))
        pb = np.where(bnd_r, w * (r - R), zero) + np.where(bnd_z, w * (az - h), zero)
        phi = np.where(outside, lo, np.where(boundary, pb, np.where(cap, az - h, r - R))).astype(F)
        gr = np.where(outside, dr / lo, np.where(boundary, np.where(bnd_r, w, zero), np.where(cap, zero, one))).astype(F)
        gz = np.where(outside, dz / lo, np.where(boundary, np.where(bnd_z, w * sz, zero), np.where(cap, sz, zero))).astype(F)
        return phi, np.stack([gr * ux, gr * uy, gz], 1).astype(F)


def restate32(c, x, fused):
    """the device's float32 evaluation of collider c at world points x: dict(phi, grad, rv, inside).  The ellipsoid's
    distance is a float64 solve on the device: its phi / grad are None here and `inside` is the implicit function's."""
    ops = Ops32(fused)
    xb, d = body32(c, x, ops)
    if c.kind == 5:
        t = xb / (F(1) * c.dims)
        inside = ops.dot((t[:, 0], t[:, 1], t[:, 2]), (t[:, 0], t[:, 1], t[:, 2])) < F(1)
        phi = grad = None
    else:
        phi, gb = sdf_body32(c.kind, xb, c.dims, ops)
        R = c.R.reshape(-1)
        grad = np.stack([ops.dot((R[3 * i], R[3 * i + 1], R[3 * i + 2]), (gb[:, 0], gb[:, 1], gb[:, 2])) for i in range(3)], 1)
        inside = phi < 0
    v, w = c.v, c.w
    if fused:
        rv = np.stack([Ops32.fma(-w[(k + 2) % 3], d[:, (k + 1) % 3], Ops32.fma(w[(k + 1) % 3], d[:, (k + 2) % 3], v[k]))
                       for k in range(3)], 1)
    else:
        rv = np.stack([v[k] + w[(k + 1) % 3] * d[:, (k + 2) % 3] - w[(k + 2) % 3] * d[:, (k + 1) % 3] for k in range(3)], 1)
    return dict(phi=phi, grad=grad, rv=rv.astype(F), inside=inside)


# ---- builders ---------------------------------------------------------------------------------------------------------

def rest_mesh(bits, T, E):
    """T disconnected right triangles with legs of one cell and E vertices in no face, on a lattice inside [0.2, 0.8]^3:
    (rest vertex positions (E + 3 T, 3) float32 -- the vertices in no face FIRST, so that the last particle is a
    triangle's corner --, indices (T, 3) int32)"""
    dx = 1.0 / (1 << bits)
    K = T + E
    M = int(np.ceil(K ** (1.0 / 3.0) - 1e-9))
    sp = 0.6 / M
    assert sp >= 2.5 * dx or K < 64, (K, sp / dx)
    k = np.arange(K)
    base = 0.2 + sp * (np.stack([k % M, (k // M) % M, k // (M * M)], 1) + 0.25)
    tri = base[:T, None, :] + dx * np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], D)[None]
    verts = np.concatenate([base[T:], tri.reshape(-1, 3)]).astype(F)
    return verts, E + np.arange(3 * T, dtype=np.int32).reshape(T, 3)


def default_state(verts, idx):
    """every particle where the rest mesh has it (faces at the float32 centroid), original order"""
    cen = ((verts[idx[:, 0]] + verts[idx[:, 1]]) + verts[idx[:, 2]]) / F(3)
    return np.concatenate([cen, verts]).astype(F)


def distinct_velocities(n, seed):
    """(n, 3) float32, every row different from every other"""
    rng = np.random.default_rng(seed)
    v = (rng.uniform(-0.5, 0.5, (n, 3)) + (np.arange(n)[:, None] + 1) * np.array([1e-4, -5e-5, 2.5e-5])).astype(F)
    assert len(np.unique(v, axis=0)) == n
    return v


FILLER = (0.5, 0.5, 0.92)      # where the particles go that a layout of aimed points has no use for


def _finish(name, bits, T, pos, cols, claims, seed, E=None, **extra):
    """the layout dict from the state in original order: T faces, E vertices in no face, 3 T corners"""
    pos = np.asarray(pos, F)
    n = len(pos)
    E = n - 4 * T if E is None else E
    assert T >= 1 and E >= 0 and n == 4 * T + E, (name, n, T, E)
    verts, idx = rest_mesh(bits, T, E)
    assert pos.min() >= 0.0 and pos.max() < 1.0, name
    massless = np.zeros(n, bool)
    massless[T:T + E] = True
    lay = dict(name=name, bits=bits, dx=1.0 / (1 << bits), T=T, E=E, n=n, rest=verts, idx=idx, pos=pos, massless=massless,
               vel=distinct_velocities(n, seed), cols=list(cols), claims=list(claims),
               n_bodies=1 + max([c.body for c in cols], default=0))
    lay.update(extra)
    return lay


def _from_points(name, bits, pts, cols, claims, seed, massless_at=(), per_point=None, **extra):
    """a layout whose particles with mass are the points `pts` (m, 3) -- faces first, then corners; 4 T >= m, the rest at
    FILLER --, plus one vertex in no face at each of `massless_at`: it has no mass and makes no pair wherever it is
    (k_ct_gen_count_scan counts only particles with mass: the ghost copies of a partitioned domain have none).
    lay["where"][k]: the particle of point k; per_point arrays become per-particle ones (-1 elsewhere)."""
    pts = np.asarray(pts, D)
    m, E = len(pts), len(massless_at)
    T = max(1, -(-m // 4))
    n = 4 * T + E
    pos = np.tile(np.asarray(FILLER, D), (n, 1)) + 1e-3 * np.arange(n)[:, None] * np.array([1.0, -0.7, 0.3]) / n
    where = np.concatenate([np.arange(T), T + E + np.arange(3 * T)])[:m]
    pos[where] = pts
    if E:
        pos[T:T + E] = np.asarray(massless_at, D)
    for k, v in (per_point or {}).items():
        a = np.full(n, -1, np.asarray(v).dtype)
        a[where] = v
        extra[k] = a
    return _finish(name, bits, T, pos, cols, claims, seed, E=E, where=where, **extra)


def _split(n):
    """np = 4 T + E with at least four vertices in no face"""
    E = 4 + n % 4
    return (n - E) // 4, E


# ---- features -------------------------------------------------------------------------------------------------------------

def _unit(v):
    v = np.asarray(v, D)
    return v / np.linalg.norm(v)


def _feature_points(kind, dims):
    """[(feature, surface point S, outward unit normal N, sides)] in the body frame; sides: which of inside (-1) and
    outside (+1) the feature is aimed at from"""
    both, out = (-1, 1), (1,)
    a = np.asarray(dims, D)
    pts = []
    if kind == 0:
        for k, (x, y) in enumerate(((0.0, 0.0), (0.07, -0.03), (-0.05, 0.06), (0.02, 0.09))):
            pts.append((f"plane {k}", (x, y, 0.0), (0, 0, 1), both))
    elif kind == 1:
        for k, dr in enumerate(((1, 0, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (1, 2, 3), (-2, 1, -0.5), (0.3, -1, 2))):
            n = _unit(dr)
            pts.append((f"sphere dir {k}", a[0] * n, n, both))
    elif kind == 2:
        frac = np.array([0.31, -0.23, 0.17])          # generic interior coordinates, as fractions of the half extents
        for ax in range(3):
            for s in (-1, 1):
                S = frac * a
                S[ax] = s * a[ax]
                n = np.zeros(3)
                n[ax] = s
                pts.append((f"face {'xyz'[ax]}{'-+'[s > 0]} (inside: nearest that face)", S, n, both))
        for ax in range(3):                           # the edge along axis ax
            for s1 in (-1, 1):
                for s2 in (-1, 1):
                    b, c = (ax + 1) % 3, (ax + 2) % 3
                    S, n = frac * a, np.zeros(3)
                    S[b], S[c] = s1 * a[b], s2 * a[c]
                    n[b], n[c] = s1, s2 * 0.8
                    pts.append((f"edge along {'xyz'[ax]} {s1:+d}{s2:+d}", S, _unit(n), out))
        for s in [(i, j, k) for i in (-1, 1) for j in (-1, 1) for k in (-1, 1)]:
            pts.append((f"corner {s}", np.array(s) * a, _unit(np.array(s) * (1.0, 0.8, 0.6)), out))
    elif kind == 3:
        r, h = a[0], a[1]
        for k, (th, z) in enumerate(((0.3, 0.0), (2.0, 0.6 * h), (4.1, -0.8 * h))):
            n = np.array([np.cos(th), np.sin(th), 0.0])
            pts.append((f"barrel {k}", r * n + (0, 0, z), n, both))
        for s in (-1, 1):
            for k, dr in enumerate(((0, 0, 1), (1, 1, 1), (-1, 0.5, 0.3))):
                n = _unit(np.array(dr) * (1, 1, s))
                pts.append((f"cap {'-+'[s > 0]} {k}", np.array([0, 0, s * h]) + r * n, n, both))
            eps = 1e-3 * h
            n = np.array([np.cos(1.1), np.sin(1.1), 0.0])
            pts.append((f"junction {'-+'[s > 0]} barrel side", r * n + (0, 0, s * (h - eps)), n, both))
            n = _unit([np.cos(2.7), np.sin(2.7), s * eps / r])
            pts.append((f"junction {'-+'[s > 0]} cap side", np.array([0, 0, s * h]) + r * n, n, both))
    elif kind == 4:
        R, h = a[0], a[1]
        for k, (th, z) in enumerate(((0.4, 0.0), (2.2, 0.45 * h), (4.4, -0.3 * h))):
            n = np.array([np.cos(th), np.sin(th), 0.0])
            pts.append((f"barrel {k} (inside: nearer the barrel)", R * n + (0, 0, z), n, both))
        for s in (-1, 1):
            for k, (th, rho) in enumerate(((0.9, 0.1 * R), (3.0, 0.5 * R), (5.0, 0.25 * R))):
                pts.append((f"cap {'-+'[s > 0]} {k} (inside: nearer the cap)", (rho * np.cos(th), rho * np.sin(th), s * h),
                            (0, 0, s), both))
            for k, th in enumerate((0.2, 2.9)):
                pts.append((f"rim {'-+'[s > 0]} {k}", (R * np.cos(th), R * np.sin(th), s * h),
                            _unit((np.cos(th), np.sin(th), 0.7 * s)), out))
    else:
        def surf(th, ph):
            S = a * (np.cos(th) * np.sin(ph), np.sin(th) * np.sin(ph), np.cos(ph))
            return S, _unit(S / (a * a))
        ends = {"x+": (0.05, np.pi / 2 - 0.05), "x-": (np.pi + 0.05, np.pi / 2 + 0.05), "y+": (np.pi / 2 - 0.05, np.pi / 2 - 0.05),
                "y-": (1.5 * np.pi + 0.05, np.pi / 2 + 0.05), "z+": (0.7, 0.05), "z-": (3.9, np.pi - 0.05)}
        for k, (th, ph) in ends.items():
            pts.append((f"axis end {k}", *surf(th, ph), both))
        for k in range(8):
            th = (k % 4) * np.pi / 2 + 0.6
            ph = 0.9 if k < 4 else np.pi - 1.1
            pts.append((f"octant {k}", *surf(th, ph), both))
    return [(f, np.asarray(S, D), np.asarray(N, D), sides) for f, S, N, sides in pts]


FEATURE_COLS = (
    dict(kind=0, p=(0.5, 0.5, 0.22), R=rot((1, 0.4, 0.1), 0.12), dims=(0, 0, 0), v=(0.1, 0.0, 0.3), w=(0.2, -0.1, 0.4)),
    dict(kind=1, p=(0.3, 0.3, 0.6), R=rot((1, 2, 3), 0.9), dims=(0.06, 0, 0), v=(0.1, 0.2, -0.1), w=(0.0, 1.0, 2.0)),
    dict(kind=2, p=(0.7, 0.3, 0.6), R=rot((2, -1, 1), 1.3), dims=(0.07, 0.05, 0.04), v=(-0.2, 0.1, 0.0), w=(0.5, 0.3, -1.0)),
    dict(kind=3, p=(0.3, 0.7, 0.6), R=rot((0.3, 1, -0.5), 2.1), dims=(0.04, 0.06, 0), v=(0.0, -0.1, 0.2), w=(1.5, 0.0, 0.7)),
    dict(kind=4, p=(0.7, 0.7, 0.6), R=rot((1, 1, 0.2), 0.8), dims=(0.06, 0.08, 0), v=(0.3, 0.0, -0.2), w=(-0.4, 2.0, 0.1)),
    dict(kind=5, p=(0.5, 0.5, 0.75), R=rot((0.2, 0.5, 1), 2.5), dims=(0.09, 0.06, 0.05), v=(0.0, 0.1, -0.2), w=(1.0, 0.2, 0.5)),
)


def features(bits=6):
    dx = 1.0 / (1 << bits)
    cols = [Col(body=1 + j, **c) for j, c in enumerate(FEATURE_COLS)]
    pos, aim = [], []
    for j, c in enumerate(cols):
        for feat, S, N, sides in _feature_points(c.kind, c.dims):
            for side in sides:
                for depth in DEPTHS:
                    pos.append(c.world((S + side * depth * dx * N)[None])[0])
                    aim.append(dict(col=j, feature=feat, side=side, depth=depth * dx))
    pos = np.array(pos)
    ai_p = np.array([a["col"] for a in aim])
    side_p = np.array([a["side"] for a in aim])
    depth_p = np.array([a["depth"] for a in aim])

    def aimed(lay):
        """every particle is decided on the side of its own collider it was aimed from, at about its depth"""
        ev = evaluate(lay)
        ai, side, depth = lay["aim_col"], lay["aim_side"], lay["aim_depth"]
        good = True
        for j in range(len(cols)):
            m = ai == j
            phi = ev[j]["phi"][m]
            good &= bool(np.all(np.where(side[m] < 0, ev[j]["din"][m], ev[j]["dout"][m])))
            good &= bool(np.all((np.abs(phi) > 0.5 * depth[m]) & (np.abs(phi) < 1.5 * depth[m])))
        return good

    def per_kind(lay):
        need = {0: ["plane"], 1: ["sphere dir"], 2: ["face", "edge along", "corner"], 3: ["barrel", "cap -", "cap +", "junction"],
                4: ["barrel", "cap -", "cap +", "rim"], 5: ["axis end", "octant"]}
        feats = {j: {a["feature"] for a in aim if a["col"] == j} for j in range(6)}
        n_box = {k: sum(f.startswith(k) for f in feats[2]) for k in ("face", "edge along", "corner")}
        return all(any(f.startswith(k) for f in feats[j]) for j in need for k in need[j]) and \
            n_box == {"face": 6, "edge along": 12, "corner": 8}

    def box_regions(lay):
        """box: outside points with exactly 1, 2 and 3 positive q; inside points nearest each of the six faces"""
        c = cols[2]
        m = lay["aim_col"] == 2
        xb, _ = body64(c, lay["pos"][m])
        q = np.abs(xb) - c.dims.astype(D)
        npos = (q > 0).sum(1)
        inside = npos == 0
        faces = {(int(np.argmax(qq)), bool(x[np.argmax(qq)] > 0)) for qq, x in zip(q[inside], xb[inside])}
        return {1, 2, 3} <= set(npos.tolist()) and len(faces) == 6

    def ties_away(lay):
        ai = lay["aim_col"]
        return all(bool(np.all(ev["b"]["grad_ok"][ai == j])) for j, ev in enumerate(evaluate(lay))) and \
            _tie_distance(lay, ai) >= TIE_BAND * dx

    claims = [("every aimed particle is decided, on its side, at its depth", aimed),
              ("every feature of every kind is aimed at", per_kind),
              ("the box's 1, 2 and 3 positive q and its six interior face regions", box_regions),
              ("gradient ties are TIE_BAND dx away", ties_away),
              ("velocities and angular velocities of the colliders are non-zero",
               lambda lay: all(np.any(c.v != 0) and np.any(c.w != 0) for c in lay["cols"]))]
    claims.append(("particles without mass sit inside the sphere, the box and the capsule",
                   lambda lay: all(bool(np.all(world_sdf64(lay["cols"][j], lay["pos"][lay["massless"]])[0][j - 1] < -0.01))
                                   for j in (1, 2, 3))))
    return _from_points("features", bits, pos, cols, claims, seed=11, massless_at=[cols[j].p for j in (1, 2, 3)],
                        per_point=dict(aim_col=ai_p, aim_side=side_p, aim_depth=depth_p), aim=aim)


def _tie_distance(lay, ai):
    """the least distance of an aimed inside particle from a tie of its own collider's gradient (box: the two largest q;
    cylinder: cap against barrel, and the axis)"""
    best = np.inf
    for j, c in enumerate(lay["cols"]):
        xb, _ = body64(c, lay["pos"][ai == j])
        dims = c.dims.astype(D)
        if c.kind == 2:
            q = np.sort(np.abs(xb) - dims, axis=1)
            inside = q[:, 2] <= 0
            if inside.any():
                best = min(best, float((q[inside, 2] - q[inside, 1]).min()))
        elif c.kind == 4:
            r, az = np.hypot(xb[:, 0], xb[:, 1]), np.abs(xb[:, 2])
            inside = (r < dims[0]) & (az < dims[1])
            if inside.any():
                best = min(best, float(np.abs((dims[1] - az) - (dims[0] - r))[inside].min()))
                barrel = inside & (dims[1] - az >= dims[0] - r)
                if barrel.any():
                    best = min(best, float(r[barrel].min()))
    return best


# ---- conventions ----------------------------------------------------------------------------------------------------------

def conventions(bits=6):
    """identity pose, p_WB = 0: `exact` lists (particle, collider, phi, body-frame = world gradient), all exactly
    representable and exactly computed (sums, differences and comparisons of dyadic numbers, or no arithmetic at all)"""
    cols = [Col(1, 1, dims=(0.5, 0, 0)),                    # sphere
            Col(3, 2, dims=(0.25, 0.5, 0)),                 # capsule
            Col(2, 3, dims=(0.5, 0.5, 0.5)),                # cube
            Col(2, 4, dims=(0.125, 0.5, 0.5)),              # thin box: a coordinate exactly 0 decides with Sign(0) = +1
            Col(4, 5, dims=(0.5, 0.5, 0)),                  # cylinder whose barrel and caps tie
            Col(4, 6, dims=(0.5, 0.25, 0))]                 # squat cylinder: the caps are nearer
    cols.append(Col(1, 7, dims=(2.0, 0, 0)))                # a container: every point is deep inside, after all the others
    P = [(0.0, 0.0, 0.0), (0.0, 0.0, 0.25), (0.375, 0.375, 0.25), (0.125, 0.375, 0.375), (0.25, 0.25, 0.25),
         (0.0, 0.25, 0.25), (0.125, 0.0, 0.125), (0.0, 0.375, 0.375),
         (0.5, 0.0, 0.0), (0.0, 0.0, 0.75), (0.125, 0.25, 0.25)]      # exactly on surfaces
    # (point, collider): phi is exactly 0 there in any arithmetic -- a pair needs phi < 0, so there is none; the container,
    # which comes later, has one
    on_surface = [(8, 0), (8, 2), (8, 4), (8, 5), (9, 1), (10, 3)]
    exact = [(0, 0, -0.5, (0, 0, 1)),            # the sphere's centre: len == 0, +z_B
             (1, 1, -0.25, (0, 0, 1)),           # on the capsule's axis segment
             (0, 1, -0.25, (0, 0, 1)),           # ... and its middle
             (2, 2, -0.125, (1, 0, 0)),          # q0 == q1 > q2: the first maximal axis
             (3, 2, -0.125, (0, 1, 0)),          # q1 == q2 > q0
             (4, 2, -0.25, (1, 0, 0)),           # q0 == q1 == q2
             (0, 2, -0.5, (1, 0, 0)),            # the cube's centre: all equal, every sign that of 0: +1
             (5, 3, -0.125, (1, 0, 0)),          # x == 0 exactly on the axis that decides: sg = +1
             (0, 4, -0.5, (1, 0, 0)),            # cylinder, the centre: on the axis, the tie goes to the barrel, +x_B
             (6, 4, -0.375, (1, 0, 0)),          # barrel and cap equally deep: the barrel
             (7, 4, -0.125, (0, 1, 0)),
             (0, 5, -0.25, (0, 0, 1)),           # squat: the cap, Sign(0) = +1
             (1, 4, -0.25, (0, 0, 1))]           # on the axis off centre: the cap is 0.25 away, the barrel 0.5
    pos = np.array(P, D)
    # np = 4 T + E with T = 1: eight points
    claims = [("every point and every dimension is exactly representable",
               lambda lay: bool(np.all(lay["pos"][lay["where"]].astype(D) == pos)) and
               all(bool(np.all(np.asarray(c.dims, D) * 8 == np.round(np.asarray(c.dims, D) * 8))) for c in lay["cols"])),
              ("the float64 restatement gives the stated answers exactly", _conventions_hold),
              ("poses are the identity at the origin",
               lambda lay: all(not c.p.any() and np.array_equal(c.R, np.eye(3, dtype=F)) for c in lay["cols"]))]
    # (a particle without mass in the middle of everything)
    claims.append(("the points on surfaces have phi64 == 0 there, and the container holds every point",
                   lambda lay: all(world_sdf64(lay["cols"][j], lay["pos"][lay["where"][k]][None])[0][0] == 0.0 for k, j in on_surface) and
                   bool(np.all(evaluate(lay)[-1]["din"][lay["where"]]))))
    return _from_points("conventions", bits, pos, cols, claims, seed=12, massless_at=[(0.125, 0.125, 0.125)], exact=exact,
                        on_surface=on_surface)


def _conventions_hold(lay):
    for k, j, phi, g in lay["exact"]:
        k = lay["where"][k]
        p64, g64 = world_sdf64(lay["cols"][j], lay["pos"][k:k + 1])
        if p64[0] != phi or not np.array_equal(g64[0], np.array(g, D)):
            return False
    return True


# extra query points of the conventions (negative coordinates cannot be particles: they lie outside the grid):
# (collider index of conventions(), point, phi, gradient)
CONVENTION_QUERIES = [(4, (0.0, -0.25, -0.25), -0.25, (0, -1, 0)), (5, (0.0, 0.0, -0.125), -0.125, (0, 0, -1)),
                      (2, (-0.375, -0.375, 0.25), -0.125, (-1, 0, 0)), (2, (0.125, -0.375, -0.375), -0.125, (0, -1, 0)),
                      (3, (-0.0, 0.25, 0.25), -0.125, (1, 0, 0)), (1, (0.0, 0.0, -0.5), -0.25, (0, 0, 1)),
                      (1, (0.0, 0.0, 0.5), -0.25, (0, 0, 1))]


# ---- shell ------------------------------------------------------------------------------------------------------------------

SHELL_N = 256
SHELL_BAND = 5 * np.sqrt(3.0) * 2.0 ** -24      # |phi64| of a shell point: 4 ulp per coordinate plus its rounding, x < 1


def nudge(x32, rng, ulps=4):
    """every coordinate moved by a whole number of float32 steps in [-ulps, ulps]"""
    k = rng.integers(-ulps, ulps + 1, x32.shape)
    bits = np.asarray(x32, F).view(np.int32) + k.astype(np.int32)      # (positive floats: consecutive integers)
    return bits.view(F)


def _surface_points(kind, dims, rng, n):
    a = np.asarray(dims, D)
    if kind == 0:
        return np.concatenate([rng.uniform(-0.1, 0.1, (n, 2)), np.zeros((n, 1))], 1)
    if kind == 1:
        v = rng.normal(size=(n, 3))
        return a[0] * v / np.linalg.norm(v, axis=1)[:, None]
    if kind == 2:
        S = rng.uniform(-1, 1, (n, 3)) * a
        ax, s = rng.integers(0, 3, n), rng.choice([-1.0, 1.0], n)
        S[np.arange(n), ax] = s * a[ax]
        # a share on edges and corners
        m = rng.random(n) < 0.3
        ax2 = (ax + 1) % 3
        S[m, ax2[m]] = rng.choice([-1.0, 1.0], m.sum()) * a[ax2[m]]
        return S
    if kind == 3:
        v = rng.normal(size=(n, 3))
        v /= np.linalg.norm(v, axis=1)[:, None]
        z = rng.uniform(-a[1], a[1], n)
        cap = rng.random(n) < 0.5
        barrel = np.stack([a[0] * np.cos(z * 50), a[0] * np.sin(z * 50), z], 1)
        caps = a[0] * v + np.stack([np.zeros(n), np.zeros(n), np.sign(v[:, 2]) * a[1]], 1)
        return np.where(cap[:, None], caps, barrel)
    th = rng.uniform(0, 2 * np.pi, n)
    z = rng.uniform(-a[1], a[1], n)
    rho = a[0] * np.sqrt(rng.random(n))
    s = rng.choice([-1.0, 1.0], n)
    which = rng.integers(0, 3, n)      # barrel, cap, rim
    r = np.where(which == 1, rho, a[0])
    zz = np.where(which == 0, z, s * a[1])
    return np.stack([r * np.cos(th), r * np.sin(th), zz], 1)


def shell(bits=6):
    cols = [Col(body=1 + j, **c) for j, c in enumerate(FEATURE_COLS[:5])]
    # (the half-space's plane through the middle of the domain: its points near p)
    cols[0] = Col(0, 1, p=(0.5, 0.5, 0.45), R=rot((1, 0.4, 0.1), 0.7), v=(0.1, 0, 0.3), w=(0.2, -0.1, 0.4))
    rng = np.random.default_rng(13)
    pos, own = [], []
    for j, c in enumerate(cols):
        # 16 x as many candidates; first those whose float32 phi is exactly 0 in the fused or in the separate order (at most
        # 32 of each: where `phi < 0` and `phi <= 0` part), then the others as they come
        x = nudge(c.world(_surface_points(c.kind, c.dims, rng, 16 * SHELL_N)).astype(F), rng)
        zero = [np.nonzero(restate32(c, x, fused)["phi"] == 0)[0][:32] for fused in (True, False)]
        first = np.unique(np.concatenate(zero))
        rest = np.setdiff1d(np.arange(len(x)), first)
        pos.append(x[np.concatenate([first, rest])[:SHELL_N]])
        own += [j] * SHELL_N
    # a container after the shells' colliders: every shell point has a decided pair behind its undecidable one, so a
    # count and a write kernel that disagree about the latter show in the rows
    container = Col(1, 1 + len(cols), p=(0.5, 0.5, 0.5), dims=(0.8, 0, 0), v=(0, 0.1, 0), w=(0.2, 0, 0.1))
    own_p = np.array(own)

    def on_shell(lay):
        own = lay["own"]
        return all(bool(np.all(np.abs(world_sdf64(c, lay["pos"][own == j])[0]) <= SHELL_BAND)) for j, c in enumerate(cols))

    def undecidable(lay):
        """three quarters of every shell are undecidable, and both signs occur on it"""
        ev = evaluate(lay)
        own = lay["own"]
        ok = True
        for j in range(len(cols)):
            m = own == j
            und = ~(ev[j]["din"][m] | ev[j]["dout"][m])
            ok &= und.mean() > 0.75 and (ev[j]["phi"][m] < 0).any() and (ev[j]["phi"][m] > 0).any()
        return ok

    def exact_zeros(lay):
        """sphere, box, capsule and cylinder have shell points whose float32 phi is exactly 0"""
        own = lay["own"]
        return all(any(np.any(restate32(c, lay["pos"][own == j], fused)["phi"] == 0) for fused in (True, False))
                   for j, c in enumerate(cols) if c.kind != 0)

    claims = [("every point is within SHELL_BAND of its own surface", on_shell),
              ("membership is undecidable on the shells, both signs occur", undecidable),
              ("float32 distances of exactly 0 occur", exact_zeros),
              ("the container holds every shell point", lambda lay: bool(np.all(evaluate(lay)[-1]["din"][lay["own"] >= 0])))]
    return _from_points("shell", bits, np.concatenate(pos), cols + [container], claims, seed=13, massless_at=[cols[1].p],
                        per_point=dict(own=own_p))


def mesh_shell_points(lattice, p, R, rng, n=SHELL_N, r_lo=0.2, r_hi=3.0):
    """n world points (float32) within +-4 ulp per coordinate of the zero set of a mesh collider's interpolant: bisection
    along rays from the body origin between r_lo and r_hi times the lattice cell ... times the mesh's extent"""
    values, nn, lo, cell = lattice
    lo64 = np.asarray(lo, D)
    hi64 = lo64 + (np.asarray(nn) - 1) * D(cell)
    ext = float(np.minimum(-lo64, hi64).min())
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    a, b = np.full(n, 0.0), np.full(n, ext)
    for _ in range(60):
        m = 0.5 * (a + b)
        phi = meshref.interpolant(values, nn, lo, cell, v * m[:, None])[0]
        a, b = np.where(phi < 0, m, a), np.where(phi < 0, b, m)
    R64 = np.asarray(R, F).astype(D).reshape(3, 3)
    x = ((v * (0.5 * (a + b))[:, None]) @ R64.T + np.asarray(p, F).astype(D)).astype(F)
    return nudge(x, rng)


# ---- blocks ---------------------------------------------------------------------------------------------------------------

def block_slots(n):
    return sorted({s for s in (0, 4094, 4095, 4096, 4097, n - 1) if 0 <= s < n})


def blocks(n, bits=6):
    """np = n particles where the rest mesh has them and no collider yet: block_colliders() places them once the slot
    order is known"""
    T, E = _split(n)
    verts, idx = rest_mesh(bits, T, E)
    pos = default_state(verts, idx)
    claims = [("np is the requested number", lambda lay: lay["n"] == n and 4 * lay["T"] + lay["E"] == n),
              ("particles are at least 0.4 dx apart",
               lambda lay: _min_distance(lay["pos"]) >= 0.4 * lay["dx"])]
    return _finish(f"blocks {n}", bits, T, pos, [], claims, seed=14 + n)


def _min_distance(pos):
    from_sorted = np.asarray(pos, D)
    best = np.inf
    for k in range(0, len(from_sorted), 1024):
        d = np.linalg.norm(from_sorted[k:k + 1024, None, :] - from_sorted[None, :, :], axis=2)
        d[np.arange(d.shape[0]), k + np.arange(d.shape[0])] = np.inf
        best = min(best, float(d.min()))
    return best


def block_colliders(lay, particles, variant):
    """four spheres of radius 0.2 dx about each of `particles` (original ids): those with centres 0.1 dx from the
    particle contain it, those 0.3 dx away miss it; particle k is inside (1, 2, 4)[(k + variant) % 3] of its four, and
    which of the four changes with k.  Bodies 1 ..; -> (colliders, {particle: number of spheres that contain it})"""
    dx = lay["dx"]
    cols, want = [], {}
    dirs = np.array([(1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, -1, -1)], D)
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    for k, pid in enumerate(particles):
        m = (1, 2, 4)[(k + variant) % 3]
        inside = [(q + k) % 4 < m for q in range(4)]
        want[int(pid)] = m
        for q in range(4):
            c = lay["pos"][pid].astype(D) + dirs[q] * dx * (0.1 if inside[q] else 0.3)
            cols.append(Col(1, 1 + len(cols), p=c, dims=(0.2 * dx, 0, 0), v=(0.1 * q, 0.05, -0.1 * k), w=(0.3, 0.2 * k, 1.0)))
    return cols, want


def blocks_claims_hold(lay, cols, want):
    """every listed particle is decided in exactly `want` spheres, every other pair is decided out"""
    tmp = dict(lay, cols=cols)
    n_in = np.zeros(lay["n"], int)
    for ev in evaluate(tmp):
        if not np.all(ev["din"] | ev["dout"]):
            return False
        n_in += ev["din"]
    expect = np.zeros(lay["n"], int)
    for pid, m in want.items():
        expect[pid] = 0 if lay["massless"][pid] else m
    return bool(np.array_equal(n_in, expect))


# ---- tables ---------------------------------------------------------------------------------------------------------------

TABLE_CENTRE = np.array([0.5, 0.5, 0.5])


def table_colliders(ellipsoid):
    """17 analytic colliders of kinds 0-4 (kind 5 in place of collider 5 with `ellipsoid`) that all contain TABLE_CENTRE by at
    least 0.01; bodies 1 .. 17"""
    rng = np.random.default_rng(15)
    cols = []
    for j in range(17):
        kind = j % 5
        R = rot(rng.normal(size=3), rng.uniform(0.2, 2.8))
        off = rng.uniform(-0.012, 0.012, 3)
        v, w = rng.uniform(-0.3, 0.3, 3), rng.uniform(-2, 2, 3)
        r3 = rng.random(3)           # (drawn whatever the kind: the other colliders are the same with and without the ellipsoid)
        if j == 5 and ellipsoid:
            kind, dims = 5, (0.06, 0.04, 0.035)
        elif kind == 0:
            dims, off = (0, 0, 0), R.astype(D) @ np.array([0.01, -0.02, 0.02 + 0.01 * r3[0]])
        elif kind == 1:
            dims = (0.035 + 0.02 * r3[0], 0, 0)
        elif kind == 2:
            dims = tuple(0.03 + 0.03 * r3)
        elif kind == 3:
            dims = (0.03 + 0.01 * r3[0], 0.05, 0)
        else:
            dims = (0.035 + 0.01 * r3[0], 0.04 + 0.02 * r3[1], 0)
        cols.append(Col(kind, 1 + j, p=TABLE_CENTRE + off, R=R, dims=dims, v=v, w=w))
    return cols


def tables(ellipsoid, bits=6):
    """point 0 at TABLE_CENTRE, 399 more in a cloud of +-0.09 about it, two particles without mass next to point 0"""
    rng = np.random.default_rng(16)
    pos = np.concatenate([TABLE_CENTRE[None], TABLE_CENTRE + rng.uniform(-0.09, 0.09, (399, 3))]).astype(F)
    cols = table_colliders(ellipsoid)

    def centre_in_all(lay):
        k = lay["where"][0]
        return all(bool(ev["din"][k]) and ev["phi"][k] < -0.01 for ev in evaluate(lay)) and \
            all(bool(np.all(ev["phi"][lay["massless"]] < -0.01)) for ev in evaluate(lay))

    def varied(lay):
        ev = evaluate(lay)
        n_in = sum(e["din"].astype(int) for e in ev)
        return len(lay["cols"]) == 17 and all(e["din"].sum() >= 5 and e["dout"].sum() >= 5 for e in ev) and len(set(n_in.tolist())) >= 8

    claims = [("particle 0 is decided inside all 17 colliders", centre_in_all),
              ("every collider has members and non-members; particles are inside many different numbers of colliders", varied),
              ("an ellipsoid is among them exactly when asked for", lambda lay: any(c.kind == 5 for c in lay["cols"]) == ellipsoid)]
    return _from_points("tables ell" if ellipsoid else "tables", bits, pos, cols, claims, seed=16,
                        massless_at=[TABLE_CENTRE + 1e-3, TABLE_CENTRE - 1e-3])


# ---- empty ----------------------------------------------------------------------------------------------------------------

def empty(bits=6):
    T, E = 30, 7
    verts, idx = rest_mesh(bits, T, E)
    pos = default_state(verts, idx)
    cols = [Col(0, 1, p=(0.5, 0.5, 0.1), R=rot((1, 0, 0), 0.2)),
            Col(1, 2, p=(0.9, 0.9, 0.9), dims=(0.05, 0, 0)),
            Col(2, 3, p=(0.5, 0.5, 0.95), R=rot((1, 1, 0), 0.5), dims=(0.2, 0.2, 0.03)),
            Col(3, 4, p=(0.1, 0.5, 0.5), R=rot((0, 1, 0), 1.0), dims=(0.03, 0.1, 0)),
            Col(4, 5, p=(0.5, 0.08, 0.5), R=rot((0, 1, 1), 0.4), dims=(0.05, 0.05, 0)),
            Col(5, 6, p=(0.92, 0.5, 0.2), R=rot((1, 2, 0), 0.3), dims=(0.05, 0.03, 0.02))]
    claims = [("every pair is decided out", lambda lay: all(bool(np.all(ev["dout"])) for ev in evaluate(lay)))]
    return _finish("empty", bits, T, pos, cols, claims, seed=17)


# ---- watch ------------------------------------------------------------------------------------------------------------------

def watch_colliders(kind, bits=6):
    """one collider of the kind in a part of the domain the watch layout leaves empty (z > 0.84; the half-space: below
    z = 0.15 about, tilted).  Sphere and capsule have a radius of 0.6 dx and the box a corner, so that each can poke
    half a cell deep through the interior of a triangle of circumradius FACE_RADIUS dx whose corners stay outside"""
    dx = 1.0 / (1 << bits)
    spec = {0: dict(p=(0.5, 0.5, 0.15), R=rot((1, 0.3, 0), 0.05)),
            1: dict(p=(0.5, 0.5, 0.9), dims=(0.6 * dx, 0, 0)),
            2: dict(p=(0.5, 0.5, 0.9), R=rot((1, 2, 0.5), 0.6), dims=(2.0 * dx, 1.5 * dx, 1.25 * dx)),
            3: dict(p=(0.5, 0.5, 0.9), R=rot((0.3, 1, 0), 0.4), dims=(0.6 * dx, 3.0 * dx, 0)),
            4: dict(p=(0.5, 0.5, 0.9), R=rot((1, 0.2, 0.4), 0.7), dims=(0.02, 0.03, 0)),
            5: dict(p=(0.5, 0.5, 0.9), R=rot((0.2, 1, 1), 1.1), dims=(0.03, 0.02, 0.012))}[kind]
    return Col(kind, 1 + kind, v=(0.1, 0, -0.1), w=(0, 0.5, 1.0), **spec)


FACE_RADIUS = 1.5      # x dx: circumradius of the triangle of a watch face state


def watch(bits=6):
    """2000 particles: 400 triangles and 400 vertices in no face, where the rest mesh has them"""
    T, E = 400, 400
    verts, idx = rest_mesh(bits, T, E)
    pos = default_state(verts, idx)
    cols = [watch_colliders(k, bits) for k in range(6)]

    def far(lay):
        return all(bool(np.all(ev["phi"] >= 0.03)) and bool(np.all(ev["dout"])) for ev in evaluate(lay)) and \
            bool(np.all(lay["pos"][:, 2] < 0.84))

    claims = [("every particle is at least 0.03 from every watch collider and below z = 0.84", far),
              ("about 2000 particles", lambda lay: lay["n"] == 2000)]
    return _finish(f"watch {bits}", bits, T, pos, cols, claims, seed=18)


def centroid64(verts32, idx):
    """the float64 centroid of the float32 corners"""
    v = np.asarray(verts32, F).astype(D)
    return (v[idx[:, 0]] + v[idx[:, 1]] + v[idx[:, 2]]) / 3.0


def watch_points(lay, positions=None):
    """the points the watch looks at: (float64 centroids of the faces' float32 corners, then the vertices), original order"""
    pos = lay["pos"] if positions is None else positions
    verts = pos[lay["T"]:]
    return np.concatenate([centroid64(verts, lay["idx"]), verts.astype(D)])


def surface_anchor(c):
    """(a surface point S and the outward unit normal N there, body frame) where the watch states touch collider c: a
    smooth spot for the vertex states; for the face states the same spot -- the shapes are small or the spot is a tip"""
    a = c.dims.astype(D)
    if c.kind == 0:
        return np.array([0.01, 0.02, 0.0]), np.array([0.0, 0.0, 1.0])
    if c.kind == 1:
        n = _unit((0.2, -0.3, 1.0))
        return a[0] * n, n
    if c.kind == 2:
        s = np.array([1.0, 1.0, 1.0])
        return s * a, _unit(s)                       # a corner
    if c.kind == 3:
        return np.array([0, 0, a[1] + a[0]]), np.array([0.0, 0.0, 1.0])      # the tip of a cap
    if c.kind == 4:
        return np.array([0.3 * a[0], 0.1 * a[0], a[1]]), np.array([0.0, 0.0, 1.0])    # on a cap
    k = int(np.argmax(a))
    n = np.zeros(3)
    n[k] = 1.0
    S = a * _unit(np.where(np.arange(3) == k, 1.0, 0.02))
    return S, _unit(S / (a * a))


def watch_state(lay, c, phi_target, who, index_particle):
    """the layout's positions with ONE watched point moved to signed distance phi_target (float64, as exactly as float32
    positions allow) from collider c, along the normal at surface_anchor(c).
    who = "vertex": the vertex `index_particle` (an original id >= T) goes there.
    who = "face": the triangle whose face is `index_particle` (< T) is moved rigidly, re-made as an equilateral triangle of
    circumradius FACE_RADIUS dx in the tangent plane, so that its centroid is there and its corners stay outside.
    -> (positions (np, 3) float32 original order, the phi64 actually reached at the watched point)"""
    pos = lay["pos"].copy()
    T, dx = lay["T"], lay["dx"]
    S, N = surface_anchor(c)
    R64 = c.R.astype(D)
    Nw = R64 @ N

    def place(t):
        x = c.world((S + t * N)[None])[0]
        if who == "vertex":
            pos[index_particle] = x.astype(F)
            pt = pos[index_particle].astype(D)[None]
        else:
            t1 = _unit(np.cross(Nw, (0.3, 0.5, 0.8)))
            t2 = np.cross(Nw, t1)
            ang = np.array([0.3, 0.3 + 2 * np.pi / 3, 0.3 + 4 * np.pi / 3])
            tri = x + FACE_RADIUS * dx * (np.cos(ang)[:, None] * t1 + np.sin(ang)[:, None] * t2)
            corners = lay["idx"][index_particle]
            pos[T + corners] = tri.astype(F)
            pt = centroid64(pos[T:], lay["idx"][index_particle:index_particle + 1])
            pos[index_particle] = pt[0].astype(F)
        return float(world_sdf64(c, pt)[0][0])

    # secant steps on the float64 distance of the float32 state (phi is nearly affine in t along the normal)
    t0, g0 = phi_target, place(phi_target)
    t1 = t0 + (phi_target - g0) + 1e-7
    g1 = place(t1)
    for _ in range(12):
        if g1 == g0 or g1 == phi_target:
            break
        t0, g0, t1 = t1, g1, t1 + (phi_target - g1) * (t1 - t0) / (g1 - g0)
        g1 = place(t1)
    return pos, g1


def at_least(lay, c, phi_min, who, index_particle):
    """watch_state whose watched point has phi64 >= phi_min, by as little as float32 positions allow"""
    step = 2.0 ** -26
    target = phi_min
    for _ in range(64):
        pos, got = watch_state(lay, c, target, who, index_particle)
        if got >= phi_min:
            return pos, got
        target += step
    raise AssertionError("no float32 state at the requested distance")


LAYOUTS = dict(features=features, conventions=conventions, shell=shell, empty=empty, watch=watch, watch8=lambda: watch(8),
               tables=lambda: tables(False), tables_ell=lambda: tables(True),
               **{f"blocks_{n}": (lambda n=n: blocks(n)) for n in BLOCK_NP})
_CACHE = {}


def layout(name):
    if name not in _CACHE:
        _CACHE[name] = LAYOUTS[name]()
    return _CACHE[name]
