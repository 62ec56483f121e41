// The per-cloth report of mpm_measure (include/mpm_hip.h): mass, momenta, energies and strain extremes of every cloth,
// reduced on the device, and mpm_face_strain, the same face quantities written per face.
//
// Every number is formed in DOUBLE from the engine's float records, by the definitions of the header:
//   vertex particle   x, v, C its own records, m the float MPM_ARR_MASSES returns
//   face particle     x, v the means of its three corner vertices' current records (what the next CalcFemStateAndForce
//                     gives it: its own x / v records are stale inside and after lean batches), C its own record (the
//                     c8 plane for C8), m = the float product |vol| x density that ParticleToGrid forms
//   strain of a face  d1, d2 = (x_b - x_a, x_c - x_a) Dm^-1 from the current corners, d3 the stored normal column F[:,2];
//                     cloth_energy_density below, the one function the host entry mpm_cloth_energy_density compiles too
//   bending           E_i = -1/4 sum_{j != i} c_ij |x_j - x_i|^2 per row of the table k_bend reads (1/2 x^T k Q x summed
//                     over the rows: Q is symmetric with zero row sums); differences only, as bend_row
//
// The reduction runs in ID order, not in slot order.  A host-built table cuts every cloth's faces and every cloth's
// vertices into chunks of at most MEASURE_CHUNK consecutive original ids; one workgroup per chunk, lane t takes the ids
// first + t, first + 256 + t, ... in that order, finds each particle's slot through DP::imap, and the workgroup adds its
// lanes in a fixed tree (xor shuffles inside a wave, then the four waves in ascending order through LDS) into one
// mpm_cloth_measure_t of partial sums.  k_measure_final, one workgroup per cloth, adds the cloth's chunk rows: the list
// (face chunks, then vertex chunks) in eight contiguous runs, every run in ascending order, then the eight runs in
// ascending order.  No floating-point atomic anywhere: which slot a particle sits in, in which order its cell received
// it, deterministic mode on or off -- none of it reaches the arithmetic, and the rows are the same bits.
//
// On an engine with the flag table of mpm_tear.h a torn face contributes nothing to the three strain energies and is
// left out of the stretch extremes (mpm_face_strain: its s1, s2, r22 are reported, its V psi is 0); its mass, momenta,
// kinetic energies and its count stay.  Without the table nothing changes.
//
// A partitioned engine counts the particles the rank OWNS (q[0].w > 0) and skips ids without a slot; a face whose
// corner is not on the rank is skipped too (an owned face always has its corners: the vertex band is wider).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/mpm_hip.h"
#include "mpm_bending.h"
#include "mpm_step.h"

namespace mpm {

constexpr int MEASURE_CHUNK = 1024;    // ids per chunk: four per lane of a 256-lane workgroup
constexpr int MEASURE_SUMS = 20;       // the doubles of mpm_cloth_measure_t, in its order
constexpr int MEASURE_FIELDS = 26;     // ... then its 4 floats and 2 counts
constexpr int MEASURE_RUNS = 8;        // runs of k_measure_final

static_assert(sizeof(mpm_cloth_measure_t) == 184, "mpm_cloth_measure_t is 184 bytes");
static_assert(offsetof(mpm_cloth_measure_t, bending) == 8 * (MEASURE_SUMS - 1), "the doubles come first, in order");
static_assert(offsetof(mpm_cloth_measure_t, stretch_max) == 160 && offsetof(mpm_cloth_measure_t, speed_max) == 172 &&
                  offsetof(mpm_cloth_measure_t, faces) == 176,
              "floats, then counts");

// s1, s2, r22, psi_in, psi_n, psi_s of one face from the columns of its deformation gradient and the floats mu, lambda,
// K, gamma of its cloth.  s1 >= s2 are the singular values of [d1 d2]: with a = [d1 d2]^T [d1 d2], J = sqrt(det a),
// T = tr a, s1 + s2 = sqrt(T + 2 J) and s1 - s2 = sqrt(T - 2 J), the latter evaluated as
// sqrt(((a11 - a22)^2 + 4 a12^2) / (T + 2 J)) -- the same number ((T - 2J)(T + 2J) = T^2 - 4 J^2) without the
// cancellation of T - 2 J on a nearly isotropic face.
__host__ __device__ inline void cloth_energy_density(float mu, float lambda, float K, float gamma, const double* d1,
                                                     const double* d2, const double* d3, double* out) {
    const double a11 = d1[0] * d1[0] + d1[1] * d1[1] + d1[2] * d1[2];
    const double a12 = d1[0] * d2[0] + d1[1] * d2[1] + d1[2] * d2[2];
    const double a22 = d2[0] * d2[0] + d2[1] * d2[1] + d2[2] * d2[2];
    const double det = a11 * a22 - a12 * a12, T = a11 + a22;
    const double J = det > 0.0 ? sqrt(det) : 0.0;
    const double sp = sqrt(fmax(T + 2.0 * J, 0.0));
    double sm = sp;   // (J = 0: s2 = 0)
    if (det > 0.0) {
        const double dd = a11 - a22;
        sm = sqrt((dd * dd + 4.0 * a12 * a12) / (T + 2.0 * J));
    }
    const double s1 = .5 * (sp + sm), s2 = .5 * (sp - sm);
    const double n[3] = {d1[1] * d2[2] - d1[2] * d2[1], d1[2] * d2[0] - d1[0] * d2[2], d1[0] * d2[1] - d1[1] * d2[0]};
    const double nn = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    double r22 = 0.0, psi_n = 0.0, psi_s = 0.0;
    if (nn > 0.0) {
        r22 = (d3[0] * n[0] + d3[1] * n[1] + d3[2] * n[2]) / nn;
        if (r22 < 1.0) {
            const double t = 1.0 - r22;
            psi_n = (double)K / 3.0 * (t * t * t);
        }
        psi_s = .5 * (double)gamma * fmax(d3[0] * d3[0] + d3[1] * d3[1] + d3[2] * d3[2] - r22 * r22, 0.0);
    }
    out[0] = s1;
    out[1] = s2;
    out[2] = r22;
    out[3] = (double)mu * ((s1 - 1.0) * (s1 - 1.0) + (s2 - 1.0) * (s2 - 1.0)) + .5 * (double)lambda * ((J - 1.0) * (J - 1.0));
    out[4] = psi_n;
    out[5] = psi_s;
}

struct MeasureArgs {
    const int4* chunks;           // [n_face_chunks + n_vertex_chunks] (cloth, first id, end id, the first id's row of the
                                  // bending table or -1): original particle ids, faces [0, NfG), vertices [NfG, NpG)
    int n_face_chunks, n_vertex_chunks;
    mpm_cloth_measure_t* rows;    // [chunk] partial sums
    const ClothMat* mats;         // [cloth] of a multi-material engine, else null (DP::M holds for every cloth)
    BendArgs bend;                // the table in force (n_rows = 0: off)
    const uint8_t* torn;          // [original face id] the flags of mpm_tear.h, or null (no table: nothing below reads it)
};

// the partial sums of one lane, and of one workgroup
struct MeasureAcc {
    double s[MEASURE_SUMS];
    float stretch_max, stretch_min, normal_min, speed_max;
    unsigned faces, vertices;
};
MPM_DEV void measure_clear(MeasureAcc& a) {
#pragma unroll
    for (int k = 0; k < MEASURE_SUMS; ++k) a.s[k] = 0.0;
    a.stretch_max = 0.f;
    a.speed_max = 0.f;
    a.stretch_min = INFINITY;
    a.normal_min = INFINITY;
    a.faces = 0u;
    a.vertices = 0u;
}

// what vertex and face particles share: mass, first moments, momenta, kinetic energies, the potential of gravity
MPM_DEV void measure_particle(const DP& p, MeasureAcc& a, double m, const double* x, const double* v, const float* C) {
    const double D = .25 * (double)p.dx * (double)p.dx;
    a.s[0] += m;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        a.s[1 + d] += m * x[d];
        a.s[4 + d] += m * v[d];
    }
    a.s[7] += m * (x[1] * v[2] - x[2] * v[1]);
    a.s[8] += m * (x[2] * v[0] - x[0] * v[2]);
    a.s[9] += m * (x[0] * v[1] - x[1] * v[0]);
    a.s[10] += m * D * ((double)C[7] - (double)C[5]);
    a.s[11] += m * D * ((double)C[2] - (double)C[6]);
    a.s[12] += m * D * ((double)C[3] - (double)C[1]);
    a.s[13] += .5 * m * (v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    double cc = 0.0;
#pragma unroll
    for (int d = 0; d < 9; ++d) cc += (double)C[d] * (double)C[d];
    a.s[14] += .5 * m * D * cc;
    const int ax = p.M.gravity_axis;
    a.s[15] += -(m * (double)p.M.gravity * (ax == 0 ? x[0] : (ax == 1 ? x[1] : x[2])));
}

// The workgroup's lanes into one row: a fixed tree -- xor shuffles inside each wave (every lane ends with the wave's
// value), then the four waves in ascending order.  All 256 lanes call it.
__device__ inline void measure_reduce_store(MeasureAcc& a, mpm_cloth_measure_t* row) {
    __shared__ double sh_s[4][MEASURE_SUMS];
    __shared__ float sh_f[4][4];
    __shared__ unsigned sh_n[4][2];
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
#pragma unroll
        for (int k = 0; k < MEASURE_SUMS; ++k) a.s[k] += __shfl_xor(a.s[k], off);
        a.stretch_max = fmaxf(a.stretch_max, __shfl_xor(a.stretch_max, off));
        a.stretch_min = fminf(a.stretch_min, __shfl_xor(a.stretch_min, off));
        a.normal_min = fminf(a.normal_min, __shfl_xor(a.normal_min, off));
        a.speed_max = fmaxf(a.speed_max, __shfl_xor(a.speed_max, off));
        a.faces += __shfl_xor(a.faces, off);
        a.vertices += __shfl_xor(a.vertices, off);
    }
    const unsigned w = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
        for (int k = 0; k < MEASURE_SUMS; ++k) sh_s[w][k] = a.s[k];
        sh_f[w][0] = a.stretch_max; sh_f[w][1] = a.stretch_min; sh_f[w][2] = a.normal_min; sh_f[w][3] = a.speed_max;
        sh_n[w][0] = a.faces; sh_n[w][1] = a.vertices;
    }
    __syncthreads();
    const unsigned t = threadIdx.x;
    if (t < (unsigned)MEASURE_SUMS) {
        reinterpret_cast<double*>(row)[t] = ((sh_s[0][t] + sh_s[1][t]) + sh_s[2][t]) + sh_s[3][t];
    } else if (t == 32u) {
        row->stretch_max = fmaxf(fmaxf(sh_f[0][0], sh_f[1][0]), fmaxf(sh_f[2][0], sh_f[3][0]));
        row->stretch_min = fminf(fminf(sh_f[0][1], sh_f[1][1]), fminf(sh_f[2][1], sh_f[3][1]));
        row->normal_min = fminf(fminf(sh_f[0][2], sh_f[1][2]), fminf(sh_f[2][2], sh_f[3][2]));
        row->speed_max = fmaxf(fmaxf(sh_f[0][3], sh_f[1][3]), fmaxf(sh_f[2][3], sh_f[3][3]));
        row->faces = sh_n[0][0] + sh_n[1][0] + sh_n[2][0] + sh_n[3][0];
        row->vertices = sh_n[0][1] + sh_n[1][1] + sh_n[2][1] + sh_n[3][1];
    }
}

// One face by original id.  false: it is not counted (no slot on this engine, not owned, or a corner without a slot).
// e[0..5] = s1, s2, r22, V psi_in, V psi_n, V psi_s.
MPM_DEV bool measure_face(const DP& p, const PSet& S, int cur, const MeasureArgs& a, int cloth, int id, MeasureAcc* acc,
                          double* e) {
    const int s = p.imap[id];
    if (s < 0 || s >= p.Nf) return false;
    int ca, cb, cc;
    if (p.idx_orig[0]) {
        ca = p.idx_orig[0][id]; cb = p.idx_orig[1][id]; cc = p.idx_orig[2][id];
    } else {   // (a partitioned rank that gave the scene's tables back keeps the corners' ids per slot)
        const int4 g = p.fg[cur][s];
        ca = g.x; cb = g.y; cc = g.z;
    }
    if (ca < p.NfG || ca >= p.NpG || cb < p.NfG || cb >= p.NpG || cc < p.NfG || cc >= p.NpG) return false;
    const int sa = p.imap[ca], sb = p.imap[cb], sc = p.imap[cc];
    if (sa < p.Nf || sa >= p.Np || sb < p.Nf || sb >= p.Np || sc < p.Nf || sc >= p.Np) return false;
    if (p.dist.on && !(S.q[0][s].w > 0.f)) return false;
    const float4 f0 = S.fq[0][s], f2 = S.fq[2][s];
    const float4 xa = S.q[0][sa], xb = S.q[0][sb], xc = S.q[0][sc];
    const float rho = a.mats ? a.mats[cloth].rho : p.M.density;
    const float mu = a.mats ? a.mats[cloth].mu : p.M.mu, lambda = a.mats ? a.mats[cloth].lambda : p.M.lambda;
    const float K = a.mats ? a.mats[cloth].K : p.M.K, gamma = a.mats ? a.mats[cloth].gamma : p.M.gamma;
    const double A[3] = {(double)xa.x, (double)xa.y, (double)xa.z};
    const double e0[3] = {(double)xb.x - A[0], (double)xb.y - A[1], (double)xb.z - A[2]};
    const double e1[3] = {(double)xc.x - A[0], (double)xc.y - A[1], (double)xc.z - A[2]};
    const double Dm0 = (double)f2.x, Dm1 = (double)f2.y, Dm3 = (double)f2.z;   // Dm^-1 = [Dm0 Dm1; 0 Dm3]
    double d1[3], d2[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        d1[d] = e0[d] * Dm0;
        d2[d] = e0[d] * Dm1 + e1[d] * Dm3;
    }
    const double d3[3] = {(double)f0.x, (double)f0.y, (double)f0.z};
    cloth_energy_density(mu, lambda, K, gamma, d1, d2, d3, e);
    const double V = (double)f2.w;
    e[3] *= V;
    e[4] *= V;
    e[5] *= V;
    // a torn face (mpm_tear.h) stores no strain energy and is left out of the extremes; its mass and momenta stay
    const bool torn = a.torn && a.torn[id] != 0;
    if (torn) e[3] = e[4] = e[5] = 0.0;
    if (acc) {
        const float4 va = S.q[1][sa], vb = S.q[1][sb], vc = S.q[1][sc];
        const float4 q2 = S.q[2][s], q3 = S.q[3][s];
        const float C[9] = {q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w, S.c8[s]};
        const float mf = f2.w * rho;   // (the float ParticleToGrid forms)
        const double x[3] = {((double)xa.x + (double)xb.x + (double)xc.x) / 3.0, ((double)xa.y + (double)xb.y + (double)xc.y) / 3.0,
                             ((double)xa.z + (double)xb.z + (double)xc.z) / 3.0};
        const double v[3] = {((double)va.x + (double)vb.x + (double)vc.x) / 3.0, ((double)va.y + (double)vb.y + (double)vc.y) / 3.0,
                             ((double)va.z + (double)vb.z + (double)vc.z) / 3.0};
        measure_particle(p, *acc, (double)mf, x, v, C);
        acc->faces += 1u;
        if (torn) return true;
        acc->s[16] += e[3];
        acc->s[17] += e[4];
        acc->s[18] += e[5];
        acc->stretch_max = fmaxf(acc->stretch_max, (float)e[0]);
        acc->stretch_min = fminf(acc->stretch_min, (float)e[1]);
        acc->normal_min = fminf(acc->normal_min, (float)e[2]);
    }
    return true;
}

// one workgroup per face chunk
__global__ __launch_bounds__(256) void k_measure_faces(DP p, MeasureArgs a) {
    const int4 ch = a.chunks[blockIdx.x];
    const int cur = p.ctl->cur;
    const PSet& S = p.set[cur];
    MeasureAcc acc;
    measure_clear(acc);
    for (int id = ch.y + (int)threadIdx.x; id < ch.z; id += 256) {
        double e[6];
        measure_face(p, S, cur, a, ch.x, id, &acc, e);
    }
    measure_reduce_store(acc, a.rows + blockIdx.x);
}

// mpm_face_strain: out[4 id ..] = s1, s2, r22, V psi of the face with original id `id` (a single engine: every face has
// a slot; one that had none would keep what the caller's buffer held)
__global__ __launch_bounds__(256) void k_measure_face_strain(DP p, MeasureArgs a, float* out) {
    const int4 ch = a.chunks[blockIdx.x];
    const int cur = p.ctl->cur;
    const PSet& S = p.set[cur];
    for (int id = ch.y + (int)threadIdx.x; id < ch.z; id += 256) {
        double e[6];
        if (measure_face(p, S, cur, a, ch.x, id, nullptr, e))
            *reinterpret_cast<float4*>(out + 4 * (size_t)id) = make_float4((float)e[0], (float)e[1], (float)e[2], (float)((e[3] + e[4]) + e[5]));
    }
}

// row r of the bending table on the current positions: -1/4 sum_j c_ij |x_j - x_i|^2 (an entry whose column has no
// vertex slot enters as a zero difference, as in bend_row; the padding of a slice has coefficient 0)
MPM_DEV double measure_bend_row(const DP& p, const PSet& S, const BendArgs& b, int r, const float4& xi) {
    const unsigned b0 = b.slice_off[r >> 6], b1 = b.slice_off[(r >> 6) + 1];
    const int width = (int)((b1 - b0) / BEND_SLICE);
    const float2* ent = b.ent + b0 + (r & 63);
    double acc = 0.0;
    for (int q = 0; q < width; ++q) {
        const float2 rec = ent[(size_t)q * BEND_SLICE];
        const int pj = __float_as_int(rec.y);
        const int sj = pj >= p.NfG && pj < p.NpG ? p.imap[pj] : -1;
        if (sj < p.Nf || sj >= p.Np) continue;
        const float4 xj = S.q[0][sj];
        const double dx = (double)xj.x - (double)xi.x, dy = (double)xj.y - (double)xi.y, dz = (double)xj.z - (double)xi.z;
        acc += (double)rec.x * (dx * dx + dy * dy + dz * dz);
    }
    return -.25 * acc;
}

// one workgroup per vertex chunk
__global__ __launch_bounds__(256) void k_measure_vertices(DP p, MeasureArgs a) {
    const int4 ch = a.chunks[a.n_face_chunks + blockIdx.x];
    const PSet& S = p.set[p.ctl->cur];
    MeasureAcc acc;
    measure_clear(acc);
    for (int id = ch.y + (int)threadIdx.x; id < ch.z; id += 256) {
        const int s = p.imap[id];
        if (s < p.Nf || s >= p.Np) continue;
        const float4 q0 = S.q[0][s];
        if (p.dist.on && !(q0.w > 0.f)) continue;
        const float4 q1 = S.q[1][s], q2 = S.q[2][s], q3 = S.q[3][s];
        const float C[9] = {q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w, q1.w};
        // (the float MPM_ARR_MASSES returns: q[0].w is the mass in a multi-material engine, the volume otherwise)
        const float mf = a.mats ? fabsf(q0.w) : fabsf(q0.w) * p.M.density;
        const double x[3] = {(double)q0.x, (double)q0.y, (double)q0.z}, v[3] = {(double)q1.x, (double)q1.y, (double)q1.z};
        measure_particle(p, acc, (double)mf, x, v, C);
        acc.speed_max = fmaxf(acc.speed_max, (float)sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]));
        acc.vertices += 1u;
        const int r = ch.w < 0 ? -1 : ch.w + (id - ch.y);
        if (r >= 0 && r < a.bend.n_rows) acc.s[19] += measure_bend_row(p, S, a.bend, r, q0);
    }
    measure_reduce_store(acc, a.rows + a.n_face_chunks + blockIdx.x);
}

// One workgroup per cloth: ranges[cloth] = (first face chunk, end face chunk, first vertex chunk, end vertex chunk), the
// vertex chunks numbered as rows (n_face_chunks + ...).  Lane (run, field) adds its field over its run of the list in
// ascending order; lane (0, field) then adds the runs in ascending order and writes the field.
__global__ __launch_bounds__(256) void k_measure_final(MeasureArgs a, const int4* ranges, mpm_cloth_measure_t* out) {
    __shared__ double sh[MEASURE_RUNS][32];
    const int4 rg = ranges[blockIdx.x];
    const int nfc = rg.y - rg.x, n = nfc + (rg.w - rg.z);
    const int field = (int)(threadIdx.x & 31u), run = (int)(threadIdx.x >> 5);
    const int per = (n + MEASURE_RUNS - 1) / MEASURE_RUNS;
    const bool is_max = field == 20 || field == 23, is_min = field == 21 || field == 22;
    double acc = is_min ? (double)INFINITY : 0.0;
    if (field < MEASURE_FIELDS) {
        const int k1 = min(n, (run + 1) * per);
        for (int k = run * per; k < k1; ++k) {
            const char* row = reinterpret_cast<const char*>(a.rows + (k < nfc ? rg.x + k : rg.z + (k - nfc)));
            double v;
            if (field < MEASURE_SUMS) v = reinterpret_cast<const double*>(row)[field];
            else if (field < 24) v = (double)reinterpret_cast<const float*>(row + 160)[field - 20];
            else v = (double)reinterpret_cast<const unsigned*>(row + 176)[field - 24];
            acc = is_max ? fmax(acc, v) : (is_min ? fmin(acc, v) : acc + v);
        }
    }
    sh[run][field] = acc;
    __syncthreads();
    if (run == 0 && field < MEASURE_FIELDS) {
        double t = sh[0][field];
        for (int r = 1; r < MEASURE_RUNS; ++r) t = is_max ? fmax(t, sh[r][field]) : (is_min ? fmin(t, sh[r][field]) : t + sh[r][field]);
        char* row = reinterpret_cast<char*>(out + blockIdx.x);
        if (field < MEASURE_SUMS) reinterpret_cast<double*>(row)[field] = t;
        else if (field < 24) reinterpret_cast<float*>(row + 160)[field - 20] = (float)t;
        else reinterpret_cast<unsigned*>(row + 176)[field - 24] = (unsigned)t;
    }
}

}  // namespace mpm
