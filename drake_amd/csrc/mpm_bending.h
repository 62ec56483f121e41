// Bending stiffness of the cloth (mpm_set_bending, include/mpm_hip.h): the quadratic hinge energy of Bergou et al. 2006
// ("A quadratic bending model for inextensible surfaces") and Wardetzky et al. 2007 ("Discrete quadratic curvature
// energies") for a rest shape that is flat per hinge.  Every interior edge x0 x1 shared by exactly two faces of one
// cloth is a hinge (x0, x1 | x2, x3), x2 opposite the edge in face A, x3 in face B; with a0, a1 the REST angles of face
// A at x0, x1 and b0, b1 those of face B,
//   K = (cot a1 + cot b1, cot a0 + cot b0, -(cot a0 + cot a1), -(cot b0 + cot b1)),   c = 3 / (A_A + A_B),
//   E = 1/2 k sum_h c_h |sum_j K_hj x_j|^2 = 1/2 x^T (k Q) x,    f = -k Q x.
// Q is constant, symmetric, its rows sum to zero and sum_j K_hj X_j = 0 on the flat rest hinge: the force is linear in
// the positions (no angle, no trigonometry, no singular configuration), vanishes on every affine image of the rest
// shape, and its total and its total torque vanish identically.
//
// Host: bending_matrix assembles Q of one cloth in double (mpm_bending_matrix), bending_table lays the table of all
// cloths out (mpm_set_bending, whose device half is in mpm_cloth_host.h).  Device: k_bend, one lane per vertex of
// the cloths with k > 0, adds f to the vertex forces k_vforce left in DP::f (launch_fem_vertices); k_bend_eval writes
// the same numbers into a buffer in original vertex order (mpm_bending_forces).  The table is a vertex row table
// (mpm_row_table.h: sliced ELL, slices of 64 rows) of k Q without its diagonal: a record is (float coefficient, int bits
// of the column's particle id), 8 bytes -- a wave reads 512 contiguous bytes per step --, the padding record is (0, the
// row's own id).  Any valence is the same path.
//
// A row is evaluated as f_i = sum_j -c_ij (x_j - x_i), in stored (ascending column) order, one fused multiply-add per
// component and entry: the diagonal is -sum_j c_ij because the rows sum to zero, and differences against the row's own
// vertex keep the cancellation at the scale of the two-ring instead of the scale of |x|.  Table and order are those of
// the original vertex ids: the result is the same bits whatever the particle order.
//
// Roundings of one component of a row with n off-diagonal entries, for the bound of tests/bending.py (first order, in
// units of 2^-24 of S_i = sum_j |k Q_ij| |x_j - x_i|, which the test's B_i dominates):
//   c_ij = float(k Q_ij), the product formed in double       1
//   x_j - x_i                                                1
//   acc = fma(-c_ij, d, acc): one rounding of a partial sum, each partial sum at most S_i, n of them       n
// R_i = n + 2 (tests use n + 3: the one more covers the second-order terms).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "mpm_row_table.h"

#ifdef __HIPCC__
#include "mpm_step.h"

namespace mpm {

constexpr int BEND_SLICE = 64, BEND_BATCH = 8;

struct BendArgs {
    const int* row_pid;          // [n_rows] particle id (NfG + vertex) of the row's vertex, ascending
    const unsigned* slice_off;   // [slices + 1] first record of a slice; its width is (next - this) / 64
    const float2* ent;           // records (coefficient, int bits of the column's particle id)
    int n_rows;
};

// Row r of the table on the current positions.  Every index into a per-particle array comes through DP::imap from an id
// of the host-built table; a slot that is no vertex slot (a particle this engine does not hold) is reported, never used
// as an address: the entry then reads the row's own position (a zero difference).  false: the row's own vertex has no slot.
// PLANE 1 (mpm_damping.h): the same row on the velocities, PSet::q[1], every coefficient times `scale` (one more rounding).
template <int PLANE = 0>
MPM_DEV bool bend_row(const DP& p, const PSet& S, const BendArgs& a, int r, int& s_out, float f[3], bool& bad, float scale = 1.f) {
    const unsigned b0 = a.slice_off[r >> 6], b1 = a.slice_off[(r >> 6) + 1];
    const int width = (int)((b1 - b0) / BEND_SLICE);
    const int s = p.imap[a.row_pid[r]];
    s_out = s;
    if (s < p.Nf || s >= p.Np) {
        bad = true;
        return false;
    }
    const float4 xi = S.q[PLANE][s];
    const float2* ent = a.ent + b0 + (r & 63);
    float f0 = 0.f, f1 = 0.f, f2 = 0.f;
    // BEND_BATCH entries at a time: their records, then their slots, then their positions -- three round trips of
    // independent loads per batch instead of two dependent ones per entry (worth about 1 % of the phase on cloth_1m,
    // the phase is not bound by that latency alone).  An
    // entry past the width reads the slice's last record again and enters with coefficient 0: fma(-0, d, f) = f.
    for (int e0 = 0; e0 < width; e0 += BEND_BATCH) {
        float2 q[BEND_BATCH];
        int sj[BEND_BATCH];
        float4 xj[BEND_BATCH];
#pragma unroll
        for (int u = 0; u < BEND_BATCH; ++u) q[u] = ent[(size_t)min(e0 + u, width - 1) * BEND_SLICE];
#pragma unroll
        for (int u = 0; u < BEND_BATCH; ++u) sj[u] = p.imap[__float_as_int(q[u].y)];
#pragma unroll
        for (int u = 0; u < BEND_BATCH; ++u) {
            const bool ok = sj[u] >= p.Nf && sj[u] < p.Np;
            bad |= !ok;
            xj[u] = S.q[PLANE][ok ? sj[u] : s];
        }
#pragma unroll
        for (int u = 0; u < BEND_BATCH; ++u) {   // (in stored order)
            const float c = e0 + u < width ? -(PLANE ? scale * q[u].x : q[u].x) : -0.f;
            f0 = fmaf(c, xj[u].x - xi.x, f0);
            f1 = fmaf(c, xj[u].y - xi.y, f1);
            f2 = fmaf(c, xj[u].z - xi.z, f2);
        }
    }
    f[0] = f0; f[1] = f1; f[2] = f2;
    return true;
}

// Behind k_vforce on the same stream, with the substep's DP: a substep that skips itself (and is run again by the
// host) adds nothing, so that the force is added once.
__global__ __launch_bounds__(256) void k_bend(DP p, BendArgs a) {
    if (gated_out(p)) return;
    const int r = (int)(blockIdx.x * 256 + threadIdx.x);
    bool bad = false;
    if (r < a.n_rows) {
        int s;
        float f[3];
        if (bend_row(p, p.set[p.ctl->cur], a, r, s, f, bad)) {
            p.f[0][s] += f[0];
            p.f[1][s] += f[1];
            p.f[2][s] += f[2];
        }
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(&p.ctl->error, ERR_CAPACITY);
}

// mpm_bending_forces: out[3 (pid - NfG) ..] = the row's force (the rows of cloths without bending stay as the caller
// left them: zero)
__global__ __launch_bounds__(256) void k_bend_eval(DP p, BendArgs a, float* out) {
    const int r = (int)(blockIdx.x * 256 + threadIdx.x);
    bool bad = false;
    if (r < a.n_rows) {
        int s;
        float f[3];
        if (bend_row(p, p.set[p.ctl->cur], a, r, s, f, bad)) {
            float* o = out + 3 * (size_t)(a.row_pid[r] - p.NfG);
            o[0] = f[0]; o[1] = f[1]; o[2] = f[2];
        }
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(&p.ctl->error, ERR_CAPACITY);
}

}  // namespace mpm
#endif  // __HIPCC__

namespace mpm {

// Q of one cloth as CSR: ascending columns, the diagonal included, every pair of vertices that shares a hinge present
// (also where the value is an exact zero, as the cotangent of a right angle is)
struct BendCsr {
    std::vector<size_t> off;
    std::vector<int32_t> col;
    std::vector<double> val;
};

// From the float rest positions and the cloth's own indices (0-based, in range: the caller has checked), in double.
// Boundary edges and edges with more than two faces form no hinge.  false with `why` set: a face with a hinge has zero
// rest area or a cotangent that is not finite (`face_base` is added to the face number in the message).
inline bool bending_matrix(const float* pos, size_t n_verts, const int32_t* idx, size_t n_faces, size_t face_base,
                           BendCsr& out, std::string& why) {
    struct Side {
        int32_t u, v, w, face;   // edge (u < v), the vertex opposite it, the face
    };
    std::vector<Side> sides;
    sides.reserve(3 * n_faces);
    for (size_t f = 0; f < n_faces; ++f) {
        const int32_t t[3] = {idx[3 * f], idx[3 * f + 1], idx[3 * f + 2]};
        for (int c = 0; c < 3; ++c) {
            const int32_t a = t[c], b = t[(c + 1) % 3], w = t[(c + 2) % 3];
            sides.push_back(Side{std::min(a, b), std::max(a, b), w, (int32_t)f});
        }
    }
    std::sort(sides.begin(), sides.end(), [](const Side& p, const Side& q) {
        return p.u != q.u ? p.u < q.u : (p.v != q.v ? p.v < q.v : p.face < q.face);
    });
    auto X = [&](int32_t v, double* x) {
        for (int d = 0; d < 3; ++d) x[d] = (double)pos[3 * (size_t)v + d];
    };
    // cotangent of the angle at a between b - a and c - a, and twice the triangle's area
    auto cot_at = [&](int32_t a, int32_t b, int32_t c, double& area2) {
        double xa[3], xb[3], xc[3];
        X(a, xa); X(b, xb); X(c, xc);
        const double u[3] = {xb[0] - xa[0], xb[1] - xa[1], xb[2] - xa[2]}, v[3] = {xc[0] - xa[0], xc[1] - xa[1], xc[2] - xa[2]};
        const double n[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
        area2 = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        return (u[0] * v[0] + u[1] * v[1] + u[2] * v[2]) / area2;
    };
    struct Trip {
        int32_t r, c;
        double v;
    };
    std::vector<Trip> trips;
    for (size_t k = 0; k < sides.size();) {
        size_t m = k + 1;
        while (m < sides.size() && sides[m].u == sides[k].u && sides[m].v == sides[k].v) ++m;
        if (m - k == 2) {
            const Side &A = sides[k], &B = sides[k + 1];
            double areaA, areaB, t;
            const double a0 = cot_at(A.u, A.v, A.w, areaA), a1 = cot_at(A.v, A.u, A.w, t);
            const double b0 = cot_at(B.u, B.v, B.w, areaB), b1 = cot_at(B.v, B.u, B.w, t);
            for (const Side* s : {&A, &B}) {
                const bool isA = s == &A;
                const double ar = isA ? areaA : areaB, c0 = isA ? a0 : b0, c1 = isA ? a1 : b1;
                if (!(ar > 0.0) || !std::isfinite(ar) || !std::isfinite(c0) || !std::isfinite(c1)) {
                    why = "bending: face " + std::to_string(face_base + (size_t)s->face) +
                          (ar > 0.0 ? " has a rest cotangent that is not finite" : " has zero rest area");
                    return false;
                }
            }
            const int32_t id[4] = {A.u, A.v, A.w, B.w};
            const double K[4] = {a1 + b1, a0 + b0, -(a0 + a1), -(b0 + b1)};
            const double c = 3.0 / (.5 * areaA + .5 * areaB);
            if (!std::isfinite(c)) {
                why = "bending: face " + std::to_string(face_base + (size_t)A.face) + " has zero rest area";
                return false;
            }
            for (int p = 0; p < 4; ++p)
                for (int q = 0; q < 4; ++q) trips.push_back(Trip{id[p], id[q], c * K[p] * K[q]});
        }
        k = m;
    }
    // (stable: the contributions to an entry are summed in the order of the hinges, sorted by edge)
    std::stable_sort(trips.begin(), trips.end(), [](const Trip& p, const Trip& q) { return p.r != q.r ? p.r < q.r : p.c < q.c; });
    out.off.assign(n_verts + 1, 0);
    out.col.clear();
    out.val.clear();
    for (size_t k = 0; k < trips.size();) {
        size_t m = k;
        double s = 0.0;
        while (m < trips.size() && trips[m].r == trips[k].r && trips[m].c == trips[k].c) s += trips[m++].v;
        out.col.push_back(trips[k].c);
        out.val.push_back(s);
        out.off[(size_t)trips[k].r + 1] += 1;
        k = m;
    }
    for (size_t v = 0; v < n_verts; ++v) out.off[v + 1] += out.off[v];
    return true;
}

// The table k_bend reads, as the host lays it out (no device is touched): one row per vertex of the cloths with k > 0, in
// ascending vertex id, k folded in, the diagonal dropped, laid out by sliced_ell (mpm_row_table.h).
struct BendRecord {
    float coef, pid_bits;   // BendArgs::ent's float2: (coefficient, int bits of the column's particle id)
};
struct BendTable : RowTable<BendRecord> {
    std::vector<double> abs_sum;       // [row] sum_j |k Q_ij|, the diagonal included
};
// cloths: anything with first_vertex, n_verts, first_face, n_faces; h_pos: the rest positions, h_idx: the faces' vertex
// ids (0-based over all cloths); stiffness: n_cloths values (0: the cloth has no rows); slice: rows per slice (BEND_SLICE).
// false with `why` set: bending_matrix refused a cloth, or the table does not fit 2^31 records.
template <class Cloth>
inline bool bending_table(const std::vector<Cloth>& cloths, const float* h_pos, const int* h_idx, size_t nf, size_t n_cloths,
                          const float* stiffness, size_t slice, BendTable& out, std::string& why) {
    auto id_bits = [](int id) {
        float f;
        memcpy(&f, &id, sizeof f);
        return f;
    };
    out = BendTable{};
    std::vector<std::vector<BendRecord>> rows;
    for (size_t c = 0; c < n_cloths; ++c) {
        if (!(stiffness[c] > 0.f)) continue;
        const Cloth& cl = cloths[c];
        std::vector<int32_t> idx(3 * cl.n_faces);
        for (size_t i = 0; i < idx.size(); ++i) idx[i] = h_idx[3 * cl.first_face + i] - (int32_t)cl.first_vertex;
        BendCsr Q;
        if (!bending_matrix(h_pos + 3 * cl.first_vertex, cl.n_verts, idx.data(), cl.n_faces, cl.first_face, Q, why)) return false;
        const double k = (double)stiffness[c];
        for (size_t v = 0; v < cl.n_verts; ++v) {
            out.row_pid.push_back((int)(nf + cl.first_vertex + v));
            rows.emplace_back();
            double a = 0.0;
            for (size_t q = Q.off[v]; q < Q.off[v + 1]; ++q) {
                a += std::fabs(k * Q.val[q]);
                if ((size_t)Q.col[q] == v) continue;
                rows.back().push_back(BendRecord{(float)(k * Q.val[q]), id_bits((int)(nf + cl.first_vertex) + Q.col[q])});
            }
            out.abs_sum.push_back(a);
        }
    }
    // (padding: coefficient 0 and the row's own id)
    if (!sliced_ell(rows.size(), slice, [&](size_t r) { return rows[r].size(); }, [&](size_t r, size_t q) { return rows[r][q]; },
                    [&](size_t r) { return BendRecord{0.f, id_bits(out.row_pid[r])}; }, out.slice_off, out.ent)) {
        why = "bending: the table is too large";
        return false;
    }
    return true;
}

}  // namespace mpm
