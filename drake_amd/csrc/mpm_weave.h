// Woven cloth, per cloth (mpm_set_weave, include/mpm_hip.h): an orthotropic St. Venant-Kirchhoff energy on the in-plane
// Green strain, resolved along per-face material axes, ADDED to the isotropic membrane of k_fem / k_fem_mat -- the
// fabric's matrix; a caller lowers the cloth's E and lets the weave carry the yarn directions.
//
// Per face with corners 0, 1, 2, rest Dm^-1 = [Dm0 Dm1; 0 Dm3] (Dm0 > 0, Dm3 > 0: Finalize's QR of the rest edges) and
// rest volume vol.  The face's rest frame is the one Dm^-1 implies: e1 along the rest edge 0 -> 1, e2 the in-plane
// perpendicular towards corner 2.  The warp is the unit vector a = (c, s) in that frame, the weft b = (-s, c).
//   F2  = [x1 - x0, x2 - x0] Dm^-1                 (3 x 2, the in-plane columns of F)
//   E   = 1/2 (F2^T F2 - I)                        (2 x 2, the Green strain)
//   Eaa = a^T E a,  Ebb = b^T E b,  Eab = a^T E b
//   Psi = 1/2 ka Eaa^2 + 1/2 kb Ebb^2 + kab Eaa Ebb + 2 G Eab^2        (per rest volume)
//   Saa = ka Eaa + kab Ebb,  Sbb = kb Ebb + kab Eaa,  Sab = 2 G Eab
//   S   = Saa a a^T + Sbb b b^T + Sab (a b^T + b a^T)
//   P   = F2 S,   G_rec = vol P grad_N,   grad_N = Dm^-T [[-1, 1, 0], [-1, 0, 1]]
// and the force on a vertex is -sum G_rec over its (face, corner) pairs.  Stateless, with an energy, rotation invariant
// (E is), and its total force and total torque vanish.  The table entry per cloth is (ka, kb, kab, 2G), formed on the host
// in double from the engineering constants E_warp, E_weft, nu (weft contraction per unit warp extension) and G, with
// D = 1 - nu^2 E_weft / E_warp:  ka = E_warp / D,  kb = E_weft / D,  kab = nu E_weft / D, each rounded once to float.  An
// entry of four zeros is a cloth without weave: its faces write nothing.
//
// Axes.  (c, s) per ORIGINAL face id, formed once at mpm_set_weave on the host in double from the rest positions
// (weave_face_axis below): the cloth's warp_dir, or the face's own entry of face_dirs, projected onto the face's rest
// plane, normalised, resolved on (e1, e2) and rounded to float.  The kernel does not renormalise.
//
// Device.  k_weave, one lane per active face slot, runs directly behind k_fem / k_fem_mat and BEFORE k_damp
// (launch_fem_faces: k_fem, k_weave, k_damp -- the float sum of a record depends on that order) and ADDS its three
// records to the ones k_fem has just written, where k_fem wrote them (DP::VF for a corner of rank < 8, the face's triple
// of DP::G3 otherwise): one writer per entry, no atomics; k_vforce and k_p2g's fused vertex forces then see the sum.  The
// face's cloth and axis come from tables per ORIGINAL face id (through PSet::pid): a re-sort needs no care, and a
// single-material engine -- whose fq[3].x carries no cloth -- takes the same path as a multi-material one.  k_weave
// gathers the corners' positions itself rather than reading the columns k_fem stored: one function, weave_face, then
// serves the substep, k_weave_eval (mpm_weave_forces, mpm_weave_strain, mpm_weave_energy) and the host
// (mpm_weave_face_records) with the same arithmetic.  k_weave_energy, one workgroup per cloth, adds the floats vol Psi
// that k_weave_eval wrote per original face id, in double, in id order in a fixed tree (mpm_measure.h's scheme): lane t
// takes first + t, first + 256 + t, ... in that order, xor shuffles inside a wave, the four waves in ascending order.  No
// atomic: a row is the same bits whatever the particle order.
//
// Arithmetic of weave_face, the same on host and device (contraction is switched off inside it; every fused
// multiply-add is written out), per component d = 0, 1, 2:
//   e0 = x1 - x0, e1 = x2 - x0                 F2[d][0] = e0 Dm0        F2[d][1] = fma(e0, Dm1, e1 Dm3)
//   C00 = fma(F2[2][0], F2[2][0], fma(F2[1][0], F2[1][0], F2[0][0] F2[0][0]))     C11 alike on column 1, C01 on both
//   E00 = 1/2 (C00 - 1)     E11 = 1/2 (C11 - 1)     E01 = 1/2 C01
//   cc = c c, ss = s s, cs = c s, t = 2 cs, q = cc - ss
//   Eaa = fma(ss, E11, fma(cc, E00, t E01))      Ebb = fma(cc, E11, fma(ss, E00, -(t E01)))
//   Eab = fma(cs, E11, fma(-cs, E00, q E01))
//   Saa = fma(ka, Eaa, kab Ebb)    Sbb = fma(kb, Ebb, kab Eaa)    Sab = (2G) Eab
//   S00 = fma(cc, Saa, fma(ss, Sbb, -(t Sab)))   S11 = fma(ss, Saa, fma(cc, Sbb, t Sab))
//   S01 = fma(cs, Saa, fma(-cs, Sbb, q Sab))
//   P[d][0] = vol fma(F2[d][0], S00, F2[d][1] S01)      P[d][1] = vol fma(F2[d][0], S01, F2[d][1] S11)
//   G[d][0] = fma(P[d][0], -Dm0, P[d][1] (-Dm1 - Dm3))  G[d][1] = fma(P[d][0], Dm0, P[d][1] Dm1)   G[d][2] = P[d][1] Dm3
//   vol Psi = vol fma(Sab, Eab, 1/2 fma(Saa, Eaa, Sbb Ebb))
//
// Roundings of one component of a record, for the bound of tests/weave.py: first order, in units of 2^-24 of the same
// expression with every term replaced by its absolute value.  The atoms are the edge differences e; Dm, vol, the
// coefficients, c and s are given floats.  C00 - 1 cancels at the rest shape, so the 1 is a TERM of the absolute-value
// expression: |E00| stands for 1/2 (|C00| + 1), and the bound does not vanish with the strain.  A factor's count adds to
// its product's, a sum carries the larger count of its terms plus its own rounding; a product with 2 or 1/2 is exact:
//   e                                                    1
//   F2[d][0]: e (1), the product (1)                     2      F2[d][1]: e (1), the product (1), the fma (1)    3
//   C00: terms 2 + 2, three roundings of the chain       7      C11: 3 + 3 + 3 = 9      C01: 2 + 3 + 3 = 8
//   E00: 7 + 1 (the difference) = 8                      E11: 10                 E01: 8
//   cc, ss, cs, t: 1                                     q = cc - ss: 2
//   Eaa, Ebb: t E01 = 1 + 8 + 1 = 10; cc E00 = 9: max + 1 = 11; ss E11 = 11: max + 1                              12
//   Eab: q E01 = 2 + 8 + 1 = 11; cs E00 = 9: max + 1 = 12; cs E11 = 11: max + 1                                  13
//   Saa, Sbb: kab Ebb = 12 + 1 = 13; ka Eaa = 12: max + 1 = 14            Sab = (2G) Eab: 13 + 1                  14
//   S00, S11: t Sab = 1 + 14 + 1 = 16; ss Sbb = 15: max + 1 = 17; cc Saa = 15: max + 1                           18
//   S01: q Sab = 2 + 14 + 1 = 17; cs Sbb = 15: max + 1 = 18; cs Saa = 15: max + 1                                19
//   P[d][0]: F2[d][1] S01 = 3 + 19 + 1 = 23; F2[d][0] S00 = 20: max + 1 = 24; times vol                          25
//   P[d][1]: F2[d][1] S11 = 3 + 18 + 1 = 22; F2[d][0] S01 = 21: max + 1 = 23; times vol                          24
//   G[d][0]: -Dm1 - Dm3 (1); P[d][1] times it = 24 + 1 + 1 = 26; P[d][0] Dm0 = 25: max + 1                       27
//   G[d][1]: P[d][1] Dm1 = 25; P[d][0] Dm0 = 25: max + 1 = 26             G[d][2] = P[d][1] Dm3                  25
// R = 27 (tests use 28: the one more covers the second-order terms).  A vertex force is the float sum of its n records
// in ascending original face id, n more roundings at most: R + n.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define MPM_WEAVE_FN __host__ __device__ inline
#else
#define MPM_WEAVE_FN inline
#endif

namespace mpm {

// coef: (ka, kb, kab, 2G); x: [corner][component]; rec: [corner][component], the records G (the force on corner k is
// -rec[k]); strain: (Eaa, Ebb, Eab); energy: vol Psi
MPM_WEAVE_FN void weave_face(float Dm0, float Dm1, float Dm3, float vol, const float coef[4], float c, float s,
                             const float x[3][3], float rec[3][3], float strain[3], float* energy) {
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
    const float E00 = .5f * (C00 - 1.f), E11 = .5f * (C11 - 1.f), E01 = .5f * C01;
    const float cc = c * c, ss = s * s, cs = c * s, t = 2.f * cs, q = cc - ss;
    const float Eaa = fmaf(ss, E11, fmaf(cc, E00, t * E01));
    const float Ebb = fmaf(cc, E11, fmaf(ss, E00, -(t * E01)));
    const float Eab = fmaf(cs, E11, fmaf(-cs, E00, q * E01));
    const float Saa = fmaf(coef[0], Eaa, coef[2] * Ebb), Sbb = fmaf(coef[1], Ebb, coef[2] * Eaa), Sab = coef[3] * Eab;
    const float S00 = fmaf(cc, Saa, fmaf(ss, Sbb, -(t * Sab)));
    const float S11 = fmaf(ss, Saa, fmaf(cc, Sbb, t * Sab));
    const float S01 = fmaf(cs, Saa, fmaf(-cs, Sbb, q * Sab));
    const float g00 = -Dm0, g10 = -Dm1 - Dm3;
    for (int d = 0; d < 3; ++d) {
        const float P0 = vol * fmaf(F[d][0], S00, F[d][1] * S01), P1 = vol * fmaf(F[d][0], S01, F[d][1] * S11);
        rec[0][d] = fmaf(P0, g00, P1 * g10);
        rec[1][d] = fmaf(P0, Dm0, P1 * Dm1);
        rec[2][d] = P1 * Dm3;
    }
    strain[0] = Eaa;
    strain[1] = Ebb;
    strain[2] = Eab;
    *energy = vol * fmaf(Sab, Eab, .5f * fmaf(Saa, Eaa, Sbb * Ebb));
}

// Host, in double: the warp (c, s) of one face from its rest corners X[corner][component] and a rest-space direction d.
// e1 = (X1 - X0) / |X1 - X0|, n = e1 x (X2 - X0) normalised, e2 = n x e1 (towards corner 2); d is projected onto the
// rest plane and normalised, (c, s) are its components on (e1, e2), rounded to float.  false: the projection is shorter
// than 1e-3 |d| (the yarn would stand on the face), d is zero or not finite, or the face has no area.
inline bool weave_face_axis(const float X[3][3], const float d[3], float cs[2]) {
    double a[3], b[3], e1[3], n[3], e2[3], dd[3];
    for (int k = 0; k < 3; ++k) {
        a[k] = (double)X[1][k] - (double)X[0][k];
        b[k] = (double)X[2][k] - (double)X[0][k];
        dd[k] = (double)d[k];
    }
    const double la = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
    const double ld = sqrt(dd[0] * dd[0] + dd[1] * dd[1] + dd[2] * dd[2]);
    if (!(la > 0.0) || !(ld > 0.0) || !(ld < (double)INFINITY)) return false;
    for (int k = 0; k < 3; ++k) e1[k] = a[k] / la;
    n[0] = e1[1] * b[2] - e1[2] * b[1];
    n[1] = e1[2] * b[0] - e1[0] * b[2];
    n[2] = e1[0] * b[1] - e1[1] * b[0];
    const double ln = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    if (!(ln > 0.0)) return false;
    for (int k = 0; k < 3; ++k) n[k] /= ln;
    e2[0] = n[1] * e1[2] - n[2] * e1[1];
    e2[1] = n[2] * e1[0] - n[0] * e1[2];
    e2[2] = n[0] * e1[1] - n[1] * e1[0];
    const double p1 = dd[0] * e1[0] + dd[1] * e1[1] + dd[2] * e1[2], p2 = dd[0] * e2[0] + dd[1] * e2[1] + dd[2] * e2[2];
    const double lp = sqrt(p1 * p1 + p2 * p2);
    if (!(lp >= 1e-3 * ld)) return false;
    cs[0] = (float)(p1 / lp);
    cs[1] = (float)(p2 / lp);
    return true;
}

// Host, in double: the table entry (ka, kb, kab, 2G) of the engineering constants, each rounded once to float.  false:
// a constant is negative or not finite (nu: not finite), D = 1 - nu^2 E_weft / E_warp <= 0, or E_warp = 0 with nu != 0.
inline bool weave_coefficients(float E_warp, float E_weft, float nu, float G, float coef[4]) {
    if (!(E_warp >= 0.f && E_weft >= 0.f && G >= 0.f) || !(E_warp < INFINITY && E_weft < INFINITY && G < INFINITY) ||
        !(fabsf(nu) < INFINITY))
        return false;
    double D = 1.0;
    if (E_warp > 0.f) D = 1.0 - (double)nu * (double)nu * (double)E_weft / (double)E_warp;
    else if (nu != 0.f) return false;
    if (!(D > 0.0)) return false;
    coef[0] = (float)((double)E_warp / D);
    coef[1] = (float)((double)E_weft / D);
    coef[2] = E_warp > 0.f ? (float)((double)nu * (double)E_weft / D) : 0.f;
    coef[3] = (float)(2.0 * (double)G);
    return coef[0] < INFINITY && coef[1] < INFINITY && fabsf(coef[2]) < INFINITY && coef[3] < INFINITY;
}

// kmax of the guard (mpm_weave_max_stable_dt): the larger of 2G and the larger eigenvalue of [[ka, kab], [kab, kb]]
inline double weave_kmax(const float coef[4]) {
    const double ka = coef[0], kb = coef[1], kab = coef[2];
    const double ev = .5 * (ka + kb) + sqrt(.25 * (ka - kb) * (ka - kb) + kab * kab);
    return ev > (double)coef[3] ? ev : (double)coef[3];
}

}  // namespace mpm

#ifdef __HIPCC__
#include "mpm_step.h"

namespace mpm {

struct WeaveArgs {
    const float4* coef;             // [cloth] (ka, kb, kab, 2G)
    const int* cloth_of_face;       // [original face id]
    const float2* axis;             // [original face id] (c, s); (0, 0) on a cloth without weave
};

// The face in slot i of the current set: its records, strains and energy, or false (its cloth has no weave: nothing to
// write).  The corner slots come from the face's own record and are vertex slots of this engine (never partitioned).
MPM_DEV bool weave_slot(const PSet& S, const WeaveArgs& a, unsigned i, const float4& f2, const float4& f3, float rec[3][3],
                        float strain[3], float* energy) {
    const int id = S.pid[i];
    const float4 c = a.coef[a.cloth_of_face[id]];
    if (c.x == 0.f && c.y == 0.f && c.z == 0.f && c.w == 0.f) return false;
    const float2 ax = a.axis[id];
    const unsigned s[3] = {(unsigned)__float_as_int(f3.y), (unsigned)__float_as_int(f3.z), (unsigned)__float_as_int(f3.w)};
    float4 xq[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) xq[k] = S.q[0][s[k]];
    float x[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        x[k][0] = xq[k].x; x[k][1] = xq[k].y; x[k][2] = xq[k].z;
    }
    const float coef[4] = {c.x, c.y, c.z, c.w};
    weave_face(f2.x, f2.y, f2.z, f2.w, coef, ax.x, ax.y, x, rec, strain, energy);
    return true;
}

// Behind k_fem / k_fem_mat and before k_damp on the same stream, with the same DP and launch geometry: the same faces,
// and a substep that skips itself (and is run again by the host) adds nothing.
__global__ __launch_bounds__(256) void k_weave(DP p, WeaveArgs a) {
    if (gated_out(p)) return;
    const unsigned nfa = (unsigned)p.ctl->nfa;
    const unsigned chunk = xcd_chunk_active(blockIdx.x, nfa);
    const unsigned i = chunk * 256 + threadIdx.x;
    if (chunk == 0xFFFFFFFFu || i >= nfa) return;
    const PSet& S = p.set[p.ctl->cur];
    const float4 f2 = S.fq[2][i], f3 = S.fq[3][i];
    float rec[3][3], strain[3], energy;
    if (!weave_slot(S, a, i, f2, f3, rec, strain, &energy)) return;
    const unsigned jb = (unsigned)__float_as_int(f3.x);
    const unsigned sc[3] = {(unsigned)__float_as_int(f3.y), (unsigned)__float_as_int(f3.z), (unsigned)__float_as_int(f3.w)};
#pragma unroll
    for (int c = 0; c < 3; ++c) {   // (the routing of mpm_fem_face.inc)
        const unsigned j = (jb >> (4 * c)) & 15u;
        float3* at = j < 8u ? reinterpret_cast<float3*>(p.VF + vf_entry(sc[c] - (unsigned)p.Nf, j) * 3u) : p.G3 + (size_t)i * 3 + c;
        const float3 g = *at;
        *at = make_float3(g.x + rec[c][0], g.y + rec[c][1], g.z + rec[c][2]);
    }
}

// mpm_weave_forces, mpm_weave_strain, mpm_weave_energy: by original face id, rec[9 id ..] = the face's records
// [corner][component], strain[3 id ..] = Eaa, Ebb, Eab, energy[id] = vol Psi (the faces of cloths without weave stay as
// the caller left them: zero)
__global__ __launch_bounds__(256) void k_weave_eval(DP p, WeaveArgs a, float* rec_out, float* strain_out, float* energy_out) {
    const unsigned i = blockIdx.x * 256 + threadIdx.x;
    if (i >= (unsigned)p.ctl->nfa) return;
    const PSet& S = p.set[p.ctl->cur];
    float rec[3][3], strain[3], energy;
    if (!weave_slot(S, a, i, S.fq[2][i], S.fq[3][i], rec, strain, &energy)) return;
    const size_t id = (size_t)S.pid[i];
    float* o = rec_out + 9 * id;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int d = 0; d < 3; ++d) o[3 * c + d] = rec[c][d];
    strain_out[3 * id] = strain[0];
    strain_out[3 * id + 1] = strain[1];
    strain_out[3 * id + 2] = strain[2];
    energy_out[id] = energy;
}

// One workgroup per cloth: out[cloth] = the double sum of energy[first .. end) (ranges[cloth] = (first, end), original
// face ids) in a fixed tree.  All 256 lanes reach the barrier.
__global__ __launch_bounds__(256) void k_weave_energy(const float* energy, const int2* ranges, double* out) {
    __shared__ double sh[4];
    const int2 rg = ranges[blockIdx.x];
    double acc = 0.0;
    for (int id = rg.x + (int)threadIdx.x; id < rg.y; id += 256) acc += (double)energy[id];
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) acc += __shfl_xor(acc, off);
    if ((threadIdx.x & 63u) == 0u) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0u) out[blockIdx.x] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

}  // namespace mpm
#endif  // __HIPCC__
