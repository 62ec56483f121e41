// External force fields on the cloth (mpm_set_force_fields, include/mpm_hip.h): a table of at most 8 fields, each an
// acceleration a(x, v) per unit MASS built on an affine vector field u(x) = u0 + G (x - x0), optionally restricted to
// a closed axis-aligned box.  A particle's acceleration is the sum, in table order, over the fields that contain it:
//   MPM_FF_ACCEL        u(x)                                          faces and vertices
//   MPM_FF_DRAG         -gamma (v - u(x))                             faces and vertices
//   MPM_FF_NORMAL_DRAG  -gamma s n,  s = (v - u(x)) . n               face particles only
//                       (-gamma s |s| n with MPM_FF_QUADRATIC)        n = d / |d|, d = F[:,2], nothing if |d|^2 < 1e-30
// One inline function, force_field_acceleration, is what k_p2g<., ., 1> (mpm_step.h) calls per lane where it forms the
// particle's external impulse, and what the host entry mpm_force_field_acceleration runs: the same arithmetic, every
// sum of products an explicit fused multiply-add (so that neither compiler chooses where to fuse), the square root and
// the division correctly rounded.  The region test is on the float position.
//
// Roundings of one field's evaluation, for the bounds of tests/force_fields.py (first order, in units of 2^-24 of the
// sum of the absolute values of the terms; a value that enters a product twice counts twice):
//   x - x0                                   1
//   u_r = three fused multiply-adds onto u0  +3 = 4
//   ACCEL        a = fma(1, u, a)            +1 = 5
//   DRAG         w = v - u                   +1 = 5;  a = fma(-gamma, w, a)                   +1 = 6
//   NORMAL_DRAG  |d|^2 (3), sqrt (1), 1 / . (1), n = d * . (1)                                 = 6 on n
//                s = w . n: 5 (w) + 6 (n) + 3 (its own fused multiply-adds)                    = 14
//                c = gamma s: 15; quadratic c |s|: 15 + 14 + 1                                 = 30
//                fma(-c, n_r, a): + 6 (n) + 1                                                  = 37 (linear: 22)
// R = 37.
#pragma once

#ifdef __HIPCC__
#define MPM_FF_FN __host__ __device__ inline
#else
#define MPM_FF_FN inline
#endif

#include <math.h>

namespace mpm {

constexpr int FF_ACCEL = 0, FF_DRAG = 1, FF_NORMAL_DRAG = 2;   // mpm_force_field_t::kind
constexpr unsigned FF_QUADRATIC = 1u, FF_REGION = 2u;          // mpm_force_field_t::flags
constexpr int MAX_FORCE_FIELDS = 8;

struct ForceField {   // mirrors mpm_force_field_t (include/mpm_hip.h)
    int kind;
    unsigned flags;
    float gamma, u0[3], G[9], x0[3], lo[3], hi[3];
};
// as k_p2g reads it: in device memory, every lane the same entry (scalar loads), the trip count the table's
struct ForceFieldTable {
    int n, pad[3];
    ForceField f[MAX_FORCE_FIELDS];
};

// acc = sum over the fields of the table whose region contains x.  d: the face particle's director F[:,2] (read only
// when is_face); a vertex particle (is_face false) gets nothing from MPM_FF_NORMAL_DRAG.
MPM_FF_FN void force_field_acceleration(const ForceField* f, int n, const float x[3], const float v[3], const float d[3],
                                        bool is_face, float acc[3]) {
    acc[0] = acc[1] = acc[2] = 0.f;
    for (int k = 0; k < n; ++k) {
        // (the whole entry first, and no short-circuit evaluation below: on the device the entry is one block of scalar
        // loads with one wait, not a chain of dependent ones)
        const ForceField q = f[k];
        bool in = !(q.flags & FF_REGION) | ((x[0] >= q.lo[0]) & (x[0] <= q.hi[0]) & (x[1] >= q.lo[1]) & (x[1] <= q.hi[1]) &
                                            (x[2] >= q.lo[2]) & (x[2] <= q.hi[2]));
        const float r0 = x[0] - q.x0[0], r1 = x[1] - q.x0[1], r2 = x[2] - q.x0[2];
        // every kind ends in acc += coef * vec, one fused multiply-add per component: ACCEL 1 * u (= acc + u, the same
        // rounding), DRAG -gamma * (v - u), NORMAL_DRAG -c * n
        float vec[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) vec[r] = fmaf(q.G[r * 3 + 2], r2, fmaf(q.G[r * 3 + 1], r1, fmaf(q.G[r * 3], r0, q.u0[r])));
        float coef = q.kind == FF_ACCEL ? 1.f : -q.gamma;
        if (q.kind != FF_ACCEL) {
#pragma unroll
            for (int r = 0; r < 3; ++r) vec[r] = v[r] - vec[r];
        }
        if (q.kind == FF_NORMAL_DRAG) {   // (the sign of d cancels: n appears twice)
            const float d2 = fmaf(d[2], d[2], fmaf(d[1], d[1], d[0] * d[0]));
            in = in & is_face & (d2 >= 1e-30f);
            const float inv = 1.f / sqrtf(d2);   // (not finite where d2 = 0: such a lane is not `in`)
            const float n0 = d[0] * inv, n1 = d[1] * inv, n2 = d[2] * inv;
            const float s = fmaf(vec[2], n2, fmaf(vec[1], n1, vec[0] * n0));
            float c = q.gamma * s;
            if (q.flags & FF_QUADRATIC) c = c * fabsf(s);
            coef = -c;
            vec[0] = n0; vec[1] = n1; vec[2] = n2;
        }
        if (in) {
#pragma unroll
            for (int r = 0; r < 3; ++r) acc[r] = fmaf(coef, vec[r], acc[r]);
        }
    }
}

}  // namespace mpm
