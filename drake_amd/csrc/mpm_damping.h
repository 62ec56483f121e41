// Stiffness-proportional damping of the cloth, per cloth (mpm_set_damping, include/mpm_hip.h): two coefficients in
// seconds, beta_membrane and beta_bending, the stiffness half of a Rayleigh pair.
//
// Membrane: Kelvin-Voigt on the in-plane Green strain.  For a face with corners 0, 1, 2, rest Dm^-1 = [Dm0 Dm1; 0 Dm3]
// and rest volume vol,
//   F2   = [x1 - x0, x2 - x0] Dm^-1   (3 x 2, the in-plane columns of F)      dF2 = [v1 - v0, v2 - v0] Dm^-1
//   Edot = 1/2 (F2^T dF2 + dF2^T F2)  (2 x 2, symmetric: the rate of the Green strain 1/2 (F2^T F2 - I))
//   S    = beta (2 mu Edot + lambda tr(Edot) I)        mu, lambda the cloth's Lame parameters, as the elastic model's
//   P    = F2 S                       (3 x 2)
//   G    = vol P grad_N,  grad_N = Dm^-T [[-1, 1, 0], [-1, 0, 1]]   the three corner records, as mpm_fem_face.inc's
// and the force on a vertex is -sum G over its (face, corner) pairs.  It is linear in v, zero for every rigid velocity
// field v0 + w x x whatever the deformation (Edot is the rate of a rotation invariant), its total and its total torque
// vanish, and it dissipates: -sum f.v = sum_faces vol S:Edot >= 0.  The director column of F (the gamma, K and c_F
// terms of the elastic model) is NOT damped: it is a state of the face particle advanced by the grid's velocity
// gradient, not by the corners, and the RPIC blend V is what acts on it.
//
// Bending: f = -beta_bending k Q v, the hinge operator of mpm_bending.h on the velocities; only on a cloth with
// mpm_set_bending stiffness k > 0.
//
// Device.  k_damp, one lane per active face slot, runs directly behind k_fem / k_fem_mat (launch_fem_faces) and ADDS
// its three records to the ones k_fem has just written, where k_fem wrote them (DP::VF for a corner of rank < 8, the
// face's triple of DP::G3 otherwise): one writer per entry, no atomics; k_vforce and k_p2g's fused vertex forces then
// see the sum.  The face's cloth comes from an int per ORIGINAL face id (through PSet::pid), so that a single-material
// engine -- whose fq[3].x carries no cloth -- takes the same path as a multi-material one; a face of a cloth with
// beta_membrane = 0 writes nothing (an int, not a byte: a single-material engine may hold any number of cloths).
// k_damp gathers the corners' positions and velocities itself rather than reading the in-plane columns k_fem stored:
// one function, damp_face, then serves the substep, mpm_damping_forces
// (k_damp_eval) and the host (mpm_damping_face_records) with the same arithmetic.  k_bend_damp runs behind k_bend
// (launch_fem_vertices) on the bending table itself -- bend_row on the velocity plane, every coefficient float(k Q_ij)
// times the beta_bending of the row's cloth, read per vertex -- and adds to DP::f.
//
// Arithmetic of damp_face, the same on host and device (contraction is switched off inside it; every fused
// multiply-add is written out), per component d = 0, 1, 2:
//   e0 = x1 - x0, e1 = x2 - x0                 F2[d][0] = e0 Dm0        F2[d][1] = fma(e0, Dm1, e1 Dm3)      (dF2 alike)
//   E00 = fma(F2[2][0], dF2[2][0], fma(F2[1][0], dF2[1][0], F2[0][0] dF2[0][0]))      E11 alike on column 1
//   E01 = 1/2 x the six-term chain  F2[d][0] dF2[d][1] (d = 0, 1, 2), then F2[d][1] dF2[d][0] (d = 0, 1, 2)
//   a = 2 (beta mu), b = beta lambda, tr = E00 + E11
//   S00 = fma(a, E00, b tr)   S11 = fma(a, E11, b tr)   S01 = a E01
//   P[d][0] = vol fma(F2[d][0], S00, F2[d][1] S01)      P[d][1] = vol fma(F2[d][0], S01, F2[d][1] S11)
//   G[d][0] = fma(P[d][0], -Dm0, P[d][1] (-Dm1 - Dm3))  G[d][1] = fma(P[d][0], Dm0, P[d][1] Dm1)   G[d][2] = P[d][1] Dm3
//
// Roundings of one component of a record, for the bound of tests/damping.py: first order, in units of 2^-24 of the
// same expression with every term replaced by its absolute value (the differences e and their velocity twins are the
// atoms); a factor's count adds to its product's, a sum carries the larger count of its terms plus its own rounding:
//   e                                                    1
//   F2[d][1]: e (1), the product (1), the fma (1)        3      (F2[d][0]: 2)          dF2 alike
//   E00, E11: terms 3 + 3, three roundings of the chain  9      E01: six roundings     12      tr: 9 + 1 = 10
//   a, b                                                 1
//   S00, S11: max(1 + 9, 1 + 10 + 1) + 1 = 13            S01 = a E01: 1 + 12 + 1       14
//   P: terms 3 + 14 = 17, product 1, fma 1, times vol 1  20
//   G: the term with -Dm1 - Dm3 (1): 20 + 1 + 1, fma 1   23
// R = 23 (tests use 24: the one more covers the second-order terms).  A vertex force is the float sum of its n records
// in ascending original face id, n more roundings at most: R + n.  A row of k_bend_damp counts as a row of k_bend plus
// one, the product beta c_ij.
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define MPM_DAMP_FN __host__ __device__ inline
#else
#define MPM_DAMP_FN inline
#endif

namespace mpm {

// x, v: [corner][component]; rec: [corner][component], the records G (the force on corner c is -rec[c])
MPM_DAMP_FN void damp_face(float Dm0, float Dm1, float Dm3, float vol, float mu, float lambda, float beta,
                           const float x[3][3], const float v[3][3], float rec[3][3]) {
#pragma clang fp contract(off)
    float F[3][2], dF[3][2];
    for (int d = 0; d < 3; ++d) {
        const float e0 = x[1][d] - x[0][d], e1 = x[2][d] - x[0][d];
        const float w0 = v[1][d] - v[0][d], w1 = v[2][d] - v[0][d];
        F[d][0] = e0 * Dm0;
        F[d][1] = fmaf(e0, Dm1, e1 * Dm3);
        dF[d][0] = w0 * Dm0;
        dF[d][1] = fmaf(w0, Dm1, w1 * Dm3);
    }
    const float E00 = fmaf(F[2][0], dF[2][0], fmaf(F[1][0], dF[1][0], F[0][0] * dF[0][0]));
    const float E11 = fmaf(F[2][1], dF[2][1], fmaf(F[1][1], dF[1][1], F[0][1] * dF[0][1]));
    float s = fmaf(F[2][0], dF[2][1], fmaf(F[1][0], dF[1][1], F[0][0] * dF[0][1]));
    s = fmaf(F[2][1], dF[2][0], fmaf(F[1][1], dF[1][0], fmaf(F[0][1], dF[0][0], s)));
    const float E01 = .5f * s;
    const float a = 2.f * (beta * mu), b = beta * lambda, tr = E00 + E11;
    const float S00 = fmaf(a, E00, b * tr), S11 = fmaf(a, E11, b * tr), S01 = a * E01;
    const float g00 = -Dm0, g10 = -Dm1 - Dm3;
    for (int d = 0; d < 3; ++d) {
        const float P0 = vol * fmaf(F[d][0], S00, F[d][1] * S01), P1 = vol * fmaf(F[d][0], S01, F[d][1] * S11);
        rec[0][d] = fmaf(P0, g00, P1 * g10);
        rec[1][d] = fmaf(P0, Dm0, P1 * Dm1);
        rec[2][d] = P1 * Dm3;
    }
}

}  // namespace mpm

#ifdef __HIPCC__
#include "mpm_bending.h"

namespace mpm {

struct DampArgs {
    const float4* coef;             // [cloth] (mu, lambda, beta_membrane, 0)
    const int* cloth_of_face;       // [original face id]
};

// The face in slot i of the current set: its records, or false (its cloth has beta_membrane = 0: nothing to write).
// The corner slots come from the face's own record and are vertex slots of this engine (never partitioned).
MPM_DEV bool damp_slot(const DP& p, const PSet& S, const DampArgs& a, unsigned i, const float4& f2, const float4& f3,
                       float rec[3][3]) {
    const float4 c = a.coef[a.cloth_of_face[S.pid[i]]];
    if (!(c.z > 0.f)) return false;
    float x[3][3], v[3][3];
    const unsigned s[3] = {(unsigned)__float_as_int(f3.y), (unsigned)__float_as_int(f3.z), (unsigned)__float_as_int(f3.w)};
    float4 xq[3], vq[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        xq[k] = S.q[0][s[k]];
        vq[k] = S.q[1][s[k]];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        x[k][0] = xq[k].x; x[k][1] = xq[k].y; x[k][2] = xq[k].z;
        v[k][0] = vq[k].x; v[k][1] = vq[k].y; v[k][2] = vq[k].z;
    }
    damp_face(f2.x, f2.y, f2.z, f2.w, c.x, c.y, c.z, x, v, rec);
    return true;
}

// Behind k_fem / k_fem_mat on the same stream, with the same DP and launch geometry: the same faces, and a substep that
// skips itself (and is run again by the host) adds nothing.
__global__ __launch_bounds__(256) void k_damp(DP p, DampArgs a) {
    if (gated_out(p)) return;
    const unsigned nfa = (unsigned)p.ctl->nfa;
    const unsigned chunk = xcd_chunk_active(blockIdx.x, nfa);
    const unsigned i = chunk * 256 + threadIdx.x;
    if (chunk == 0xFFFFFFFFu || i >= nfa) return;
    const PSet& S = p.set[p.ctl->cur];
    const float4 f2 = S.fq[2][i], f3 = S.fq[3][i];
    float rec[3][3];
    if (!damp_slot(p, S, a, i, f2, f3, rec)) return;
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

// mpm_damping_forces: out[9 * original face id ..] = the face's records, [corner][component] (the faces of cloths
// without membrane damping stay as the caller left them: zero)
__global__ __launch_bounds__(256) void k_damp_eval(DP p, DampArgs a, float* out) {
    const unsigned i = blockIdx.x * 256 + threadIdx.x;
    if (i >= (unsigned)p.ctl->nfa) return;
    const PSet& S = p.set[p.ctl->cur];
    float rec[3][3];
    if (!damp_slot(p, S, a, i, S.fq[2][i], S.fq[3][i], rec)) return;
    float* o = out + 9 * (size_t)S.pid[i];
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int d = 0; d < 3; ++d) o[3 * c + d] = rec[c][d];
}

// Row r of the bending table (mpm_bending.h) on the current velocities, for a vertex whose cloth has beta_bending > 0:
// f_i = sum_j -(beta c_ij) (v_j - v_i), bend_row on the velocity plane with every coefficient times beta.  Behind k_bend
// on the same stream, with the substep's DP (a substep that skips itself adds nothing).
__global__ __launch_bounds__(256) void k_bend_damp(DP p, BendArgs a, const float* beta_vertex) {
    if (gated_out(p)) return;
    const int r = (int)(blockIdx.x * 256 + threadIdx.x);
    bool bad = false;
    if (r < a.n_rows) {
        const float beta = beta_vertex[a.row_pid[r] - p.NfG];
        int s;
        float f[3];
        if (beta > 0.f && bend_row<1>(p, p.set[p.ctl->cur], a, r, s, f, bad, beta)) {
            p.f[0][s] += f[0];
            p.f[1][s] += f[1];
            p.f[2][s] += f[2];
        }
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(&p.ctl->error, ERR_CAPACITY);
}

// mpm_damping_forces: out[3 (pid - NfG) ..] = the row's force (other rows stay as the caller left them: zero)
__global__ __launch_bounds__(256) void k_bend_damp_eval(DP p, BendArgs a, const float* beta_vertex, float* out) {
    const int r = (int)(blockIdx.x * 256 + threadIdx.x);
    bool bad = false;
    if (r < a.n_rows) {
        const float beta = beta_vertex[a.row_pid[r] - p.NfG];
        int s;
        float f[3];
        if (beta > 0.f && bend_row<1>(p, p.set[p.ctl->cur], a, r, s, f, bad, beta)) {
            float* o = out + 3 * (size_t)(a.row_pid[r] - p.NfG);
            o[0] = f[0]; o[1] = f[1]; o[2] = f[2];
        }
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(&p.ctl->error, ERR_CAPACITY);
}

}  // namespace mpm
#endif  // __HIPCC__
