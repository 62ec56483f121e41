// Tearing cloth, per cloth (mpm_set_tearing, include/mpm_hip.h): a face whose largest in-plane stretch exceeds the
// cloth's stretch_limit FAILS -- from that substep on it exerts no membrane, weave or damping force and no normal-column
// stress in ParticleToGrid.  The only state is one monotone byte per ORIGINAL face id (`torn`): the substep only ever
// sets it, mpm_set_torn_faces alone may clear it (scissors / restore).
//
// Per face with corners 0, 1, 2 and rest Dm^-1 = [Dm0 Dm1; 0 Dm3] (fq[2]), on the positions k_fem has just used:
//   F2 = [x1 - x0, x2 - x0] Dm^-1 (3 x 2),  C = F2^T F2 (the right Cauchy-Green tensor of the face's plane)
//   lambda1 = m + sqrt(q), the larger eigenvalue of C: the SQUARE of the largest principal stretch, with
//   m = 1/2 (C00 + C11),  q = (1/2 (C00 - C11))^2 + C01^2
//   the face fails when lambda1 > L,  L = (float)(stretch_limit^2) formed on the host in double and rounded once.
// The decision takes no square root: with h = L - m,  fails = (h < 0) || (q > h h).  (h < 0: m alone is past L; else
// both sides of sqrt(q) > h are non-negative and may be squared.)  A NaN position fails nothing: both comparisons are
// false.  L = 0 means the cloth never tears; otherwise stretch_limit is finite and > 1.
//
// Arithmetic of tear_face, the same on host and device (contraction is switched off inside it; every fused
// multiply-add is written out), per component d = 0, 1, 2 -- the chains of weave_face (mpm_weave.h):
//   e0 = x1 - x0, e1 = x2 - x0                 F2[d][0] = e0 Dm0        F2[d][1] = fma(e0, Dm1, e1 Dm3)
//   C00 = fma(F2[2][0], F2[2][0], fma(F2[1][0], F2[1][0], F2[0][0] F2[0][0]))     C11 alike on column 1, C01 on both
//   m = 1/2 (C00 + C11)      dlt = 1/2 (C00 - C11)      q = fma(dlt, dlt, C01 C01)
//   h = L - m                fails = (h < 0) || (q > h h)
//
// Roundings, for the bound of tests/tearing.py: first order, in units of 2^-24.  The atoms are the edge differences e
// (one rounding each, relative to themselves); Dm and L are given floats; a product with 1/2 is exact, and so is the
// product inside a fused multiply-add.  The two terms of F2[d][1] may cancel on a skewed face, so its error is relative
// to A1[d] = |e0 Dm1| + |e1 Dm3|, not to itself; from there on every error is propagated through the expression it
// enters (a square x^2 carries 2 |x| dx) rather than restated against absolute values -- C11 of a sliver would
// otherwise be charged A1^2 where it carries |F2[d][1]| A1:
//   dF0[d] = 2 |F2[d][0]|   (e, the product)             dF1[d] = 3 A1[d]   (e, the product, the fma)
//   dC00  = 7 C00           (2 x 2 per term, three roundings of the chain)
//   dC11  = sum_d 6 |F2[d][1]| A1[d] + 3 C11             dC01 = sum_d |F2[d][0]| (5 |F2[d][1]| + 3 A1[d])
//   dm    = 1/2 (dC00 + dC11) + |m|                      ddlt = 1/2 (dC00 + dC11) + |dlt|
//   dq    = 2 |dlt| ddlt + 2 |C01| dC01 + C01^2 + q      (the product C01 C01 and the fma: one rounding each)
//   dh    = dm + |h|                                     dhh  = 2 |h| dh + h^2
// On an isotropic face dlt and C01 vanish and q is second order: 2^-24 (ddlt^2 + dC01^2) is added to dq.  The sign of h
// is the sign of the exact difference of the floats L and m: a float subtraction never rounds across zero.  The verdict
// can differ from the exact one only where |lambda1 - L| <= dh + (dq + dhh) / (sqrt(q) + |h|), in the same units.
//
// Device.  k_tear, one lane per active face slot, with the launch geometry, gate and chunk order of k_weave, is
// launched LAST in launch_fem_faces (k_fem, k_weave, k_damp, k_tear) and only on an engine whose tables exist (some
// cloth has a limit, or some face is flagged).  Per lane: the face's original id from PSet::pid, its cloth from a table
// by face id, L from a table by cloth.  An intact face of a cloth with L > 0 is evaluated; if it fails its byte is set
// -- a plain store, one writer per id.  A torn face, whether torn just now or earlier, has its three corner records
// overwritten with +0.0f where k_fem wrote them (the routing of mpm_fem_face.inc: DP::VF for a corner of rank < 8, the
// face's triple of DP::G3 otherwise) and its DP::ta entry (the factor of the normal-column stress that ParticleToGrid
// scatters) set to zero: membrane, weave and damping contributions are erased together, since all three live in those
// records.  An intact face writes nothing.  A face sees only its own state: decisions within a substep are Jacobi, the
// result does not depend on the particle order or the determinism mode, and a substep that skips itself (gated_out)
// marks nothing.  No atomics.
// What a torn face KEEPS: its face particle stays in the scene with its mass, its centroid position and velocity
// (k_fem writes them before k_tear runs) and the update of its deformation gradient F; it still carries momentum
// through the grid and still takes part in grid contact.  Only its forces and its stress are gone.
//
// k_tear_eval (mpm_tear_measure): m, q and the would-fail verdict by original face id, state untouched.
// k_tear_count (mpm_tear_state): one workgroup per cloth counts the set bytes of its faces in id order in a fixed tree
// (lane t takes first + t, first + 256 + t, ...; xor shuffles inside a wave; the four waves in ascending order).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define MPM_TEAR_FN __host__ __device__ inline
#else
#define MPM_TEAR_FN inline
#endif

namespace mpm {

// x: [corner][component]; mq: (m, q); returns the verdict lambda1 > L (L <= 0 is the caller's business: the formula
// is evaluated as it stands)
MPM_TEAR_FN bool tear_face(float Dm0, float Dm1, float Dm3, float L, const float x[3][3], float mq[2]) {
#pragma clang fp contract(off)
    float F[3][2];
    for (int d = 0; d < 3; ++d) {
        const float e0 = x[1][d] - x[0][d], e1 = x[2][d] - x[0][d];
        F[d][0] = e0 * Dm0;
        F[d][1] = fmaf(e0, Dm1, e1 * Dm3);
    }
    const float C00 = fmaf(F[2][0], F[2][0], fmaf(F[1][0], F[1][0], F[0][0] * F[0][0]));
    const float C11 = fmaf(F[2][1], F[2][1], fmaf(F[1][1], F[1][1], F[0][1] * F[0][1]));
    const float C01 = fmaf(F[2][0], F[2][1], fmaf(F[1][0], F[1][1], F[0][0] * F[0][1]));
    const float m = .5f * (C00 + C11), dlt = .5f * (C00 - C11);
    const float q = fmaf(dlt, dlt, C01 * C01);
    const float h = L - m;
    mq[0] = m;
    mq[1] = q;
    return (h < 0.f) || (q > h * h);
}

// Host, in double: L = (float)(limit^2), rounded once.  false: the limit is neither 0 (never tears: L = 0) nor a finite
// number > 1 whose square is a finite float.
inline bool tear_limit(float stretch_limit, float* L) {
    *L = 0.f;
    if (stretch_limit == 0.f) return true;
    if (!(stretch_limit > 1.f) || !(stretch_limit < INFINITY)) return false;
    const float l = (float)((double)stretch_limit * (double)stretch_limit);
    if (!(l < INFINITY)) return false;
    *L = l;
    return true;
}

// Host: the tables of the kernels from the cloths' face ranges (first face, face count; cloths in call order cover
// [0, n_faces) without gaps) and the limits: L[cloth], cloth_of_face[n_faces], ranges[cloth] = (first, end).  false: a
// limit is refused (tear_limit) or a range leaves [0, n_faces).
inline bool tear_tables(size_t n_cloths, const size_t* first_face, const size_t* n_faces_of, const float* stretch_limit,
                        size_t n_faces, float* L, int* cloth_of_face, int* ranges2) {
    for (size_t c = 0; c < n_cloths; ++c) {
        if (!tear_limit(stretch_limit[c], &L[c])) return false;
        if (first_face[c] > n_faces || n_faces_of[c] > n_faces - first_face[c]) return false;
        ranges2[2 * c] = (int)first_face[c];
        ranges2[2 * c + 1] = (int)(first_face[c] + n_faces_of[c]);
        for (size_t f = first_face[c]; f < first_face[c] + n_faces_of[c]; ++f) cloth_of_face[f] = (int)c;
    }
    return true;
}

}  // namespace mpm

#ifdef __HIPCC__
#include "mpm_step.h"

namespace mpm {

struct TearArgs {
    const float* L;                 // [cloth] (float)(stretch_limit^2), 0: never tears
    const int* cloth_of_face;       // [original face id]
    uint8_t* torn;                  // [original face id] 0 intact, 1 torn; nullptr: the feature is off
};

// the verdict of the face in slot i of the current set against L (the corner slots are vertex slots of this engine:
// never partitioned)
MPM_DEV bool tear_slot(const PSet& S, unsigned i, const float4& f2, const float4& f3, float L, float mq[2]) {
    const unsigned s[3] = {(unsigned)__float_as_int(f3.y), (unsigned)__float_as_int(f3.z), (unsigned)__float_as_int(f3.w)};
    float4 xq[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) xq[k] = S.q[0][s[k]];
    float x[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        x[k][0] = xq[k].x; x[k][1] = xq[k].y; x[k][2] = xq[k].z;
    }
    return tear_face(f2.x, f2.y, f2.z, L, x, mq);
}

// Last of the face chain (k_fem / k_fem_mat, k_weave, k_damp, k_tear) on the same stream, with the same DP and launch
// geometry: the same faces, and a substep that skips itself (and is run again by the host) marks and erases nothing.
__global__ __launch_bounds__(256) void k_tear(DP p, TearArgs a) {
    if (gated_out(p)) return;
    const unsigned nfa = (unsigned)p.ctl->nfa;
    const unsigned chunk = xcd_chunk_active(blockIdx.x, nfa);
    const unsigned i = chunk * 256 + threadIdx.x;
    if (chunk == 0xFFFFFFFFu || i >= nfa) return;
    const PSet& S = p.set[p.ctl->cur];
    const int id = S.pid[i];
    const float4 f3 = S.fq[3][i];
    if (a.torn[id] == 0) {
        const float L = a.L[a.cloth_of_face[id]];
        if (!(L > 0.f)) return;
        float mq[2];
        if (!tear_slot(S, i, S.fq[2][i], f3, L, mq)) return;
        a.torn[id] = 1;   // (one writer per id)
    }
    const unsigned jb = (unsigned)__float_as_int(f3.x);
    const unsigned sc[3] = {(unsigned)__float_as_int(f3.y), (unsigned)__float_as_int(f3.z), (unsigned)__float_as_int(f3.w)};
    const float3 zero = make_float3(0.f, 0.f, 0.f);
#pragma unroll
    for (int c = 0; c < 3; ++c) {   // (the routing of mpm_fem_face.inc)
        const unsigned j = (jb >> (4 * c)) & 15u;
        float3* at = j < 8u ? reinterpret_cast<float3*>(p.VF + vf_entry(sc[c] - (unsigned)p.Nf, j) * 3u) : p.G3 + (size_t)i * 3 + c;
        *at = zero;
    }
    p.ta[i] = zero;
}

// mpm_tear_measure: by original face id, mq_out[2 id ..] = (m, q), fail_out[id] = the verdict against the cloth's L
// (0 on a cloth without a limit and while the feature is off: a.L == nullptr).  Changes no state.
__global__ __launch_bounds__(256) void k_tear_eval(DP p, TearArgs a, float* mq_out, uint8_t* fail_out) {
    const unsigned i = blockIdx.x * 256 + threadIdx.x;
    if (i >= (unsigned)p.ctl->nfa) return;
    const PSet& S = p.set[p.ctl->cur];
    const size_t id = (size_t)S.pid[i];
    const float L = a.L ? a.L[a.cloth_of_face[id]] : 0.f;
    float mq[2];
    const bool fails = tear_slot(S, i, S.fq[2][i], S.fq[3][i], L, mq);
    mq_out[2 * id] = mq[0];
    mq_out[2 * id + 1] = mq[1];
    fail_out[id] = (L > 0.f && fails) ? 1 : 0;
}

// One workgroup per cloth: out[cloth] = the number of set bytes of torn[first .. end) (ranges[cloth] = (first, end),
// original face ids).  All 256 lanes reach the barrier.
__global__ __launch_bounds__(256) void k_tear_count(const uint8_t* torn, const int2* ranges, uint32_t* out) {
    __shared__ uint32_t sh[4];
    const int2 rg = ranges[blockIdx.x];
    uint32_t acc = 0u;
    for (int id = rg.x + (int)threadIdx.x; id < rg.y; id += 256) acc += torn[id] != 0 ? 1u : 0u;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) acc += __shfl_xor(acc, off);
    if ((threadIdx.x & 63u) == 0u) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0u) out[blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

}  // namespace mpm
#endif  // __HIPCC__
