"""Float64 reference for mesh colliders (mpm_sdf_shape_from_mesh / mpm_sdf_collider_t, include/mpm_hip.h): the test
meshes, generated in code; brute-force point-triangle distance and generalised winding number; the lattice as the header
defines it; a restatement of the documented interpolant; and the pair rule."""
import numpy as np

F = np.float32


# ---- meshes (vertices in the body frame, int32 triangles) -------------------------------------------------------------

def icosphere(radius=0.05, levels=2):
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
         (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
         (9, 8, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(levels):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return (np.array(v) * radius).astype(F), np.array(f, np.int32)


def box(half):
    hx, hy, hz = half
    v = np.array([[sx * hx, sy * hy, sz * hz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], F)
    # corner index = 4 ix + 2 iy + iz; two triangles per face, outward
    f = [(0, 1, 3), (0, 3, 2), (4, 6, 7), (4, 7, 5), (0, 4, 5), (0, 5, 1), (2, 3, 7), (2, 7, 6), (0, 2, 6), (0, 6, 4),
         (1, 5, 7), (1, 7, 3)]
    return v, np.array(f, np.int32)


def torus(R=0.05, r=0.02, nu=24, nv=12):
    u = np.arange(nu) * 2 * np.pi / nu
    w = np.arange(nv) * 2 * np.pi / nv
    U, W = np.meshgrid(u, w, indexing="ij")
    v = np.stack([(R + r * np.cos(W)) * np.cos(U), (R + r * np.cos(W)) * np.sin(U), r * np.sin(W)], -1).reshape(-1, 3)
    f = []
    for i in range(nu):
        for j in range(nv):
            a, b = i * nv + j, ((i + 1) % nu) * nv + j
            c, d = ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
            f += [(a, b, c), (a, c, d)]
    return v.astype(F), np.array(f, np.int32)


def slab(half_xy=0.25, depth=0.125):
    """a thick slab whose top face is the body frame's z = 0 (dyadic corners: the lattice nodes near the top carry
    z_B exactly)"""
    v, f = box((half_xy, half_xy, depth / 2))
    v[:, 2] -= depth / 2
    return v, f


def mesh_extent(v):
    return float((v.max(0) - v.min(0)).max())


# ---- brute force ---------------------------------------------------------------------------------------------------------

def _seg_dist2(p, a, b):
    ab = b - a
    t = np.clip(np.einsum("...k,...k", p - a, ab) / np.maximum(np.einsum("...k,...k", ab, ab), 1e-300), 0, 1)
    d = p - (a + t[..., None] * ab)
    return np.einsum("...k,...k", d, d)


def point_triangle_dist2(p, a, b, c):
    """squared distance, points p (N, 1, 3) against triangles a, b, c (1, T, 3) -> (N, T)"""
    ab, ac = b - a, c - a
    n = np.cross(ab, ac)
    nn = np.einsum("...k,...k", n, n)
    ap = p - a
    # barycentric coordinates of the projection
    d00, d01, d11 = np.einsum("...k,...k", ab, ab), np.einsum("...k,...k", ab, ac), np.einsum("...k,...k", ac, ac)
    d20, d21 = np.einsum("...k,...k", ap, ab), np.einsum("...k,...k", ap, ac)
    den = d00 * d11 - d01 * d01
    with np.errstate(invalid="ignore", divide="ignore"):
        v = (d11 * d20 - d01 * d21) / den
        w = (d00 * d21 - d01 * d20) / den
        h2 = np.einsum("...k,...k", ap, n) ** 2 / nn
    inside = (v >= 0) & (w >= 0) & (v + w <= 1) & (nn > 0)
    edges = np.minimum(np.minimum(_seg_dist2(p, a, b), _seg_dist2(p, b, c)), _seg_dist2(p, c, a))
    return np.where(inside, h2, edges)


def winding_number(p, a, b, c):
    """generalised winding number (van Oosterom-Strackee solid angles / 4 pi), p (N, 1, 3) -> (N,)"""
    A, B, Cc = a - p, b - p, c - p
    la, lb, lc = (np.linalg.norm(X, axis=-1) for X in (A, B, Cc))
    det = np.einsum("...k,...k", A, np.cross(B, Cc))
    den = la * lb * lc + np.einsum("...k,...k", A, B) * lc + np.einsum("...k,...k", A, Cc) * lb + \
        np.einsum("...k,...k", B, Cc) * la
    return (2 * np.arctan2(det, den)).sum(-1) / (4 * np.pi)


def mesh_sdf(points, verts, tris, chunk=2048):
    """signed distance of points (N, 3) to the mesh: nearest triangle, negative where |winding number| > 0.5"""
    P = np.asarray(points, np.float64)
    V = np.asarray(verts, np.float64)
    a, b, c = (V[tris[:, k]][None] for k in range(3))
    out = np.empty(len(P))
    for s in range(0, len(P), chunk):
        p = P[s:s + chunk, None, :]
        d = np.sqrt(point_triangle_dist2(p, a, b, c).min(1))
        out[s:s + chunk] = np.where(np.abs(winding_number(p, a, b, c)) > 0.5, -d, d)
    return out


def lattice_layout(verts, cell, pad):
    """(n (3,), lo (3,) float32) as mpm_sdf_shape_from_mesh lays the lattice out"""
    V = np.asarray(verts, np.float64)
    mn, mx = V.min(0), V.max(0)
    n = (np.ceil((mx - mn) / np.float64(F(cell))) + 2 * pad + 1).astype(np.int64)
    lo = (mn.astype(F) - F(pad) * F(cell)).astype(F)
    return n, lo


def lattice_nodes(n, lo, cell):
    """node positions (n_z, n_y, n_x, 3), x fastest"""
    k, j, i = np.meshgrid(np.arange(n[2]), np.arange(n[1]), np.arange(n[0]), indexing="ij")
    return np.stack([lo[0] + i * np.float64(cell), lo[1] + j * np.float64(cell), lo[2] + k * np.float64(cell)], -1)


# ---- the documented interpolant ------------------------------------------------------------------------------------------

def interpolant(values, n, lo, cell, xb):
    """phi and the body-frame unit gradient at body-frame points xb (N, 3), from the lattice values (n_z, n_y, n_x)"""
    xb = np.asarray(xb, np.float64)
    lo = np.asarray(lo, np.float64)
    hi = lo + (np.asarray(n) - 1) * np.float64(cell)
    q = np.clip(xb, lo, hi)
    t = (q - lo) * np.float64(F(1) / F(cell))        # (the float reciprocal of the cell, as documented)
    i = np.minimum(np.floor(t).astype(np.int64), np.asarray(n) - 2)
    f = np.minimum(t - i, 1.0)
    V = np.asarray(values, np.float64)
    c = {}
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                c[dx, dy, dz] = V[i[:, 2] + dz, i[:, 1] + dy, i[:, 0] + dx]
    fx, fy, fz = f[:, 0], f[:, 1], f[:, 2]
    a = {(dy, dz): c[0, dy, dz] + fx * (c[1, dy, dz] - c[0, dy, dz]) for dy in (0, 1) for dz in (0, 1)}
    b0, b1 = a[0, 0] + fy * (a[1, 0] - a[0, 0]), a[0, 1] + fy * (a[1, 1] - a[0, 1])
    tri = b0 + fz * (b1 - b0)
    d = xb - q
    out = np.linalg.norm(d, axis=1)
    ex = {(dy, dz): c[1, dy, dz] - c[0, dy, dz] for dy in (0, 1) for dz in (0, 1)}
    ex0, ex1 = ex[0, 0] + fy * (ex[1, 0] - ex[0, 0]), ex[0, 1] + fy * (ex[1, 1] - ex[0, 1])
    gx = ex0 + fz * (ex1 - ex0)
    ey0, ey1 = a[1, 0] - a[0, 0], a[1, 1] - a[0, 1]
    gy = ey0 + fz * (ey1 - ey0)
    gz = b1 - b0
    g = np.where((out > 0)[:, None], d, np.stack([gx, gy, gz], 1))
    nn = np.einsum("ij,ij->i", g, g)
    with np.errstate(invalid="ignore", divide="ignore"):
        g = np.where((nn > 1e-30)[:, None], g / np.sqrt(nn)[:, None], np.array([0.0, 0.0, 1.0]))
    return tri + out, g, t


def world_sdf(values, n, lo, cell, col, x):
    """phi, world gradient and the lattice coordinate t of world points x for an SdfCollider (float32 pose)"""
    R = np.array(col.R_WB[:], F).astype(np.float64).reshape(3, 3)
    p = np.array(col.p_WB[:], F).astype(np.float64)
    xb = (np.asarray(x, np.float64) - p) @ R
    phi, gb, t = interpolant(values, n, lo, cell, xb)
    return phi, gb @ R.T, t


def rigid_v(col, x):
    d = np.asarray(x, np.float64) - np.array(col.p_WB[:], np.float64)
    return np.array(col.v[:], np.float64) + np.cross(np.array(col.w[:], np.float64), d)


def analytic_box_sdf(xb, half):
    q = np.abs(xb) - np.asarray(half)
    return np.linalg.norm(np.maximum(q, 0), axis=1) + np.minimum(q.max(1), 0)
