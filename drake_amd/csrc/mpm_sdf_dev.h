// Mesh colliders on the device (an extension: the reference's ComputeSignedDistanceToPoint ignores Mesh and Convex).
// A triangle mesh becomes a signed-distance lattice once (k_sdf_build); the pair generator, the watch and
// mpm_sdf_collider_signed_distance evaluate that lattice with ONE interpolant (mesh_locate + mesh_eval), documented in
// include/mpm_hip.h at mpm_sdf_collider_t.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mpm_math.h"

namespace mpm {

// ---- the lattice build (mpm_sdf_shape_from_mesh) ---------------------------------------------------------------------
// Brute force, O(nodes x triangles): one thread per lattice node, a workgroup per brick of 8 x 8 x 4 nodes.  The
// triangles pass through LDS in tiles of SDF_TILE, three float4 (the corners; w unused) each: every lane of a wave reads
// the same triangle at the same time, so the 16-byte reads broadcast.  Per node the minimum squared point-triangle
// distance (closest point by regions, C. Ericson, "Real-Time Collision Detection", 5.1.5) and the sum of the signed solid
// angles (A. van Oosterom, J. Strackee, IEEE Trans. Biomed. Eng. 30 (1983)), both in the triangles' order: a build is
// deterministic.  |winding number| > 0.5 is inside.
constexpr int SDF_TILE = 256;
constexpr int SDF_BX = 8, SDF_BY = 8, SDF_BZ = 4;

MPM_DEV float sdf_dot3(float ax, float ay, float az, float bx, float by, float bz) { return ax * bx + ay * by + az * bz; }

// squared distance from p (the origin after the shift: a, b, c are the corners minus p) to the triangle
MPM_DEV float tri_dist2(float3 a, float3 b, float3 c) {
    const float3 ab = make_float3(b.x - a.x, b.y - a.y, b.z - a.z), ac = make_float3(c.x - a.x, c.y - a.y, c.z - a.z);
    // ap = -a, bp = -b, cp = -c
    const float d1 = -sdf_dot3(ab.x, ab.y, ab.z, a.x, a.y, a.z), d2 = -sdf_dot3(ac.x, ac.y, ac.z, a.x, a.y, a.z);
    if (d1 <= 0.f && d2 <= 0.f) return sdf_dot3(a.x, a.y, a.z, a.x, a.y, a.z);                       // vertex a
    const float d3 = -sdf_dot3(ab.x, ab.y, ab.z, b.x, b.y, b.z), d4 = -sdf_dot3(ac.x, ac.y, ac.z, b.x, b.y, b.z);
    if (d3 >= 0.f && d4 <= d3) return sdf_dot3(b.x, b.y, b.z, b.x, b.y, b.z);                         // vertex b
    float3 q;
    const float vc = d1 * d4 - d3 * d2;
    const float d5 = -sdf_dot3(ab.x, ab.y, ab.z, c.x, c.y, c.z), d6 = -sdf_dot3(ac.x, ac.y, ac.z, c.x, c.y, c.z);
    const float vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) {                                                        // edge ab
        const float v = d1 / (d1 - d3);
        q = make_float3(a.x + v * ab.x, a.y + v * ab.y, a.z + v * ab.z);
    } else if (d6 >= 0.f && d5 <= d6) {                                                               // vertex c
        q = c;
    } else if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) {                                                 // edge ac
        const float w = d2 / (d2 - d6);
        q = make_float3(a.x + w * ac.x, a.y + w * ac.y, a.z + w * ac.z);
    } else if (va <= 0.f && (d4 - d3) >= 0.f && (d5 - d6) >= 0.f) {                                   // edge bc
        const float w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        q = make_float3(b.x + w * (c.x - b.x), b.y + w * (c.y - b.y), b.z + w * (c.z - b.z));
    } else {                                                                                          // the face
        // the distance to the plane along the unit normal: exact for a face whose corners share a coordinate
        const float nx = ab.y * ac.z - ab.z * ac.y, ny = ab.z * ac.x - ab.x * ac.z, nz = ab.x * ac.y - ab.y * ac.x;
        const float nn = sdf_dot3(nx, ny, nz, nx, ny, nz);
        if (nn > 0.f) {
            const float h = sdf_dot3(nx, ny, nz, a.x, a.y, a.z) / sqrtf(nn);
            return h * h;
        }
        const float denom = 1.f / (va + vb + vc), v = vb * denom, w = vc * denom;
        q = make_float3(a.x + ab.x * v + ac.x * w, a.y + ab.y * v + ac.y * w, a.z + ab.z * v + ac.z * w);
    }
    return sdf_dot3(q.x, q.y, q.z, q.x, q.y, q.z);
}

// the signed solid angle of the triangle seen from the origin (van Oosterom-Strackee)
MPM_DEV float tri_solid_angle(float3 a, float3 b, float3 c) {
    const float la = sqrtf(sdf_dot3(a.x, a.y, a.z, a.x, a.y, a.z)), lb = sqrtf(sdf_dot3(b.x, b.y, b.z, b.x, b.y, b.z)),
                lc = sqrtf(sdf_dot3(c.x, c.y, c.z, c.x, c.y, c.z));
    const float det = a.x * (b.y * c.z - b.z * c.y) - a.y * (b.x * c.z - b.z * c.x) + a.z * (b.x * c.y - b.y * c.x);
    const float den = la * lb * lc + sdf_dot3(a.x, a.y, a.z, b.x, b.y, b.z) * lc + sdf_dot3(a.x, a.y, a.z, c.x, c.y, c.z) * lb +
                      sdf_dot3(b.x, b.y, b.z, c.x, c.y, c.z) * la;
    return 2.f * atan2f(det, den);
}

// nodes of bricks [brick0, brick0 + gridDim.x), triangles [t_begin, t_end): tri = n_tri x 3 float4 corners; out = the
// lattice, x fastest.  A large mesh is split over launches along its triangles as well: each node's running minimum and
// solid-angle sum travel in `state` from one launch to the next (first: start from nothing; last: write the value), in
// the triangles' order -- the same sums, to the bit, as a single pass.
__global__ __launch_bounds__(256) void k_sdf_build(const float4* __restrict__ tri, int t_begin, int t_end, int nx, int ny,
                                                   int nz, int bx, int by, float lo_x, float lo_y, float lo_z, float cell,
                                                   int brick0, int first, int last, float2* __restrict__ state,
                                                   float* __restrict__ out) {
    __shared__ float4 s_tri[SDF_TILE * 3];
    const int b = brick0 + (int)blockIdx.x;
    const int i = (b % bx) * SDF_BX + (threadIdx.x & 7), j = ((b / bx) % by) * SDF_BY + ((threadIdx.x >> 3) & 7),
              k = (b / (bx * by)) * SDF_BZ + (threadIdx.x >> 6);
    const bool node = i < nx && j < ny && k < nz;
    const size_t at = ((size_t)k * ny + j) * nx + i;
    const float px = lo_x + (float)i * cell, py = lo_y + (float)j * cell, pz = lo_z + (float)k * cell;
    float d2 = 3.40282347e38f, omega = 0.f;
    if (!first && node) {
        const float2 st = state[at];
        d2 = st.x;
        omega = st.y;
    }
    for (int t0 = t_begin; t0 < t_end; t0 += SDF_TILE) {
        const int nt = min(SDF_TILE, t_end - t0);
        __syncthreads();   // (the previous tile has been read by every wave)
        for (int e = threadIdx.x; e < nt * 3; e += 256) s_tri[e] = tri[(size_t)t0 * 3 + e];
        __syncthreads();
        for (int t = 0; t < nt; ++t) {
            const float4 A = s_tri[t * 3], B = s_tri[t * 3 + 1], C = s_tri[t * 3 + 2];
            const float3 a = make_float3(A.x - px, A.y - py, A.z - pz), bb = make_float3(B.x - px, B.y - py, B.z - pz),
                         c = make_float3(C.x - px, C.y - py, C.z - pz);
            d2 = fminf(d2, tri_dist2(a, bb, c));
            omega += tri_solid_angle(a, bb, c);
        }
    }
    if (!node) return;
    if (!last) {
        state[at] = make_float2(d2, omega);
        return;
    }
    const float w = omega * (float)(0.25 / M_PI);
    const float d = sqrtf(d2);
    out[at] = fabsf(w) > 0.5f ? -d : d;
}

// the exact cull's box (see MeshCollider): the cells with a corner value below `thr`, as min / max cell index per axis
// (box[0..2] atomicMin, box[3..5] atomicMax)
__global__ __launch_bounds__(256) void k_sdf_cull_box(const float* __restrict__ val, int nx, int ny, int nz, float thr, int* box) {
    const int cx = nx - 1, cy = ny - 1;
    const long long n_cells = (long long)cx * cy * (nz - 1);
    int lo[3] = {0x7FFFFFFF, 0x7FFFFFFF, 0x7FFFFFFF}, hi[3] = {-1, -1, -1};
    for (long long c = blockIdx.x * 256ll + threadIdx.x; c < n_cells; c += (long long)gridDim.x * 256) {
        const int i = (int)(c % cx), j = (int)((c / cx) % cy), k = (int)(c / ((long long)cx * cy));
        const size_t o = ((size_t)k * ny + j) * nx + i, sy = nx, sz = (size_t)nx * ny;
        const float m = fminf(fminf(fminf(val[o], val[o + 1]), fminf(val[o + sy], val[o + sy + 1])),
                              fminf(fminf(val[o + sz], val[o + sz + 1]), fminf(val[o + sz + sy], val[o + sz + sy + 1])));
        if (m < thr) {
            lo[0] = min(lo[0], i); lo[1] = min(lo[1], j); lo[2] = min(lo[2], k);
            hi[0] = max(hi[0], i); hi[1] = max(hi[1], j); hi[2] = max(hi[2], k);
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (lo[a] != 0x7FFFFFFF) atomicMin(&box[a], lo[a]);
        if (hi[a] >= 0) atomicMax(&box[3 + a], hi[a]);
    }
}

// ---- the interpolant ---------------------------------------------------------------------------------------------------
// One entry of the engine's mesh-collider table (mpm_set_sdf_colliders): the pose of mpm_sdf_collider_t with its lattice.
// The cull: every cell outside [cmin, cmax] (cell indices, per axis) has all eight corner values >= the lattice cell, so a
// point whose clamped cell lies outside has phi >= trilinear >= about one cell -- never a pair, and never within a watch
// margin below half a cell.  The test needs no value: it costs the clamp and the cell index, which phi needs anyway.
// the gradient's floor: a squared length (value per cell inside the box, length outside) at or below it gives +z_B
constexpr float SDF_GRAD_FLOOR2 = 1e-30f;
struct MeshCollider {
    const float* val;     // the lattice, x fastest
    int n[3];             // nodes per axis (>= 2)
    int cmin[3], cmax[3]; // the cull's cells
    float lo[3], hi[3];   // the lattice box in the body frame: lo + (n - 1) cell
    float inv;            // 1 / cell
    float cell;
    uint32_t body;
    float p[3], R[9], v[3], w[3];
};

// Everything below is evaluated without contraction, the FMAs written out: the count kernel and the write kernel must
// decide membership with the same bits whatever either instance's scheduling.
MPM_DEV void mesh_body_coords(const MeshCollider& m, const float* x, float* xb) {
#pragma clang fp contract(off)
    const float d0 = x[0] - m.p[0], d1 = x[1] - m.p[1], d2 = x[2] - m.p[2];
    xb[0] = fmaf(m.R[6], d2, fmaf(m.R[3], d1, m.R[0] * d0));
    xb[1] = fmaf(m.R[7], d2, fmaf(m.R[4], d1, m.R[1] * d0));
    xb[2] = fmaf(m.R[8], d2, fmaf(m.R[5], d1, m.R[2] * d0));
}

// the clamped point's cell (ci) and fraction (f) in it, and x_B - q (d); false when the cull rules the point out
MPM_DEV bool mesh_locate(const MeshCollider& m, const float* xb, bool cull, int* ci, float* f, float* d) {
#pragma clang fp contract(off)
    bool keep = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float q = fminf(fmaxf(xb[a], m.lo[a]), m.hi[a]);
        d[a] = xb[a] - q;
        const float t = (q - m.lo[a]) * m.inv;
        const int i = min((int)t, m.n[a] - 2);
        ci[a] = i;
        f[a] = fminf(t - (float)i, 1.f);
        keep = keep && i >= m.cmin[a] && i <= m.cmax[a];
    }
    return keep || !cull;
}

// phi at the located point; with g != nullptr also the body-frame unit gradient
MPM_DEV float mesh_eval(const MeshCollider& m, const int* ci, const float* f, const float* d, float* g) {
#pragma clang fp contract(off)
    const size_t sy = (size_t)m.n[0], sz = (size_t)m.n[0] * m.n[1];
    const float* v = m.val + ((size_t)ci[2] * m.n[1] + ci[1]) * m.n[0] + ci[0];
    const float c000 = v[0], c100 = v[1], c010 = v[sy], c110 = v[sy + 1];
    const float c001 = v[sz], c101 = v[sz + 1], c011 = v[sz + sy], c111 = v[sz + sy + 1];
    const float a00 = fmaf(f[0], c100 - c000, c000), a10 = fmaf(f[0], c110 - c010, c010);
    const float a01 = fmaf(f[0], c101 - c001, c001), a11 = fmaf(f[0], c111 - c011, c011);
    const float b0 = fmaf(f[1], a10 - a00, a00), b1 = fmaf(f[1], a11 - a01, a01);
    const float tri = fmaf(f[2], b1 - b0, b0);
    const float out = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    const float phi = tri + out;
    if (g) {
        float gx, gy, gz;
        if (out > 0.f) {   // outside the lattice box: away from it
            gx = d[0]; gy = d[1]; gz = d[2];
        } else {           // the trilinear cell's own gradient (in value per cell: the common factor 1 / cell drops out)
            const float e00 = c100 - c000, e10 = c110 - c010, e01 = c101 - c001, e11 = c111 - c011;
            const float ex0 = fmaf(f[1], e10 - e00, e00), ex1 = fmaf(f[1], e11 - e01, e01);
            gx = fmaf(f[2], ex1 - ex0, ex0);
            const float ey0 = a10 - a00, ey1 = a11 - a01;
            gy = fmaf(f[2], ey1 - ey0, ey0);
            gz = b1 - b0;
        }
        const float nn = gx * gx + gy * gy + gz * gz;
        if (nn > SDF_GRAD_FLOOR2) {
            const float s = 1.f / sqrtf(nn);
            g[0] = gx * s; g[1] = gy * s; g[2] = gz * s;
        } else {           // (a flat spot: +z_B, as sdf_closed does)
            g[0] = 0.f; g[1] = 0.f; g[2] = 1.f;
        }
    }
    return phi;
}

// membership (phi < thr) of the world point x; the count and write kernels ask it with thr = 0, the watch with its margin
MPM_DEV bool mesh_below(const MeshCollider& m, const float* x, float thr) {
    float xb[3], f[3], d[3];
    int ci[3];
    mesh_body_coords(m, x, xb);
    if (!mesh_locate(m, xb, thr < 0.5f * m.cell, ci, f, d)) return false;
    return mesh_eval(m, ci, f, d, nullptr) < thr;
}

// phi and the unit world gradient at the world point x (no cull)
MPM_DEV float mesh_sdf(const MeshCollider& m, const float* x, float* grad) {
    float xb[3], f[3], d[3], gb[3];
    int ci[3];
    mesh_body_coords(m, x, xb);
    mesh_locate(m, xb, false, ci, f, d);
    const float phi = mesh_eval(m, ci, f, d, gb);
    mulv3(m.R, gb, grad);
    return phi;
}

// mpm_sdf_collider_signed_distance
__global__ __launch_bounds__(256) void k_ct_sdf_mesh_query(MeshCollider m, int n, const float* x, float* phi, float* grad) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const float xk[3] = {x[k * 3], x[k * 3 + 1], x[k * 3 + 2]};
    float g[3];
    phi[k] = mesh_sdf(m, xk, g);
    grad[k * 3] = g[0]; grad[k * 3 + 1] = g[1]; grad[k * 3 + 2] = g[2];
}

}  // namespace mpm
