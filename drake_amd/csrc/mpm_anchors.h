// Anchors: springs and cords from cloth vertices to rigid bodies (mpm_set_anchors, include/mpm_hip.h).  A pin (mpm_pins.h)
// is a hard constraint; an anchor is the compliant attachment: vertex `vertex` is joined to the point p_BQ of body `body`
// by the law of a link (mpm_links.h).  With t the body's clock at the start of the substep -- the clock of the pins,
// which k_pin advances behind GridToParticle --, p(t), R(t) = pin_pose(motion, t):
//   y = p(t) + R(t) p_BQ,   v_Q = v + w x (R(t) p_BQ)          in double, as k_pin forms them, each rounded to float once
//   f = link_force(k, L, c, tension_only, d = y32 - x, w = v_Q32 - v_vertex)     the inline function of mpm_links.h itself
// and body `body` receives the force impulse l = -(double)f (double)dt and the torque impulse ((double)y32 - p_WB) x l
// about the p_WB of its motion as set (the convention of pins), in the fixed-point accumulators pins, contact and grid
// bodies share (imp_fixed: the sums do not depend on the order).
//
// Host: anchor_table lays the caller's anchors out and forms the sums of the stability guard (no device is touched: a
// plain C++17 program can include this header).  Device: k_anchor_pose, one lane per motion slot, evaluates pin_pose
// once per body and substep into a small table of doubles; k_anchor, one lane per anchored vertex behind k_hinge_gather
// (launch_fem_vertices), adds the row's force to DP::f and the reactions to the accumulators; k_anchor_eval writes the
// same forces into a buffer in original vertex order and touches no accumulator (mpm_anchor_forces); k_anchor_energy,
// one lane per anchor, forms one double term, one float length and the float point (mpm_anchor_state).  The table is a
// vertex row table (mpm_row_table.h: sliced ELL, slices of 64 rows), a row's entries its vertex's anchors in anchor
// order.  An entry is two 16-byte words,
//   (motion slot | the tension-only flag in bit 31, k, L, c)  (p_BQ.x, p_BQ.y, p_BQ.z, accumulator index or 0xFFFFFFFF)
// -- the caller's floats, no host rounding enters --; the padding record is (0, 0, 0, 0) (0, 0, 0, 0xFFFFFFFF): k = L =
// c = 0 gives an exact zero through the seam branch whatever the pose, and no accumulator means no atomic.  The
// accumulator index is the caller's body; the kernel compares it with the accumulators' count.  Table and order are
// those of the original vertex ids: a vertex's force is the same bits whatever the particle order.
//
// Roundings of one component of one anchor's force, for the bound of tests/anchors.py (first order, in units of 2^-24):
// R_link = 18 of mpm_links.h on S = k (l + L) + c |w| (the float differences d = y32 - x and w = v_Q32 - v_vertex are
// in that count), and two terms a link does not have, because its ends are floats as given and an anchor's far end is
// computed:
//   y32 = float(y): 1 unit at the scale of |y|, which enters d and is multiplied by k              k |y|
//   v_Q32 = float(v_Q): 1 unit at the scale of |v_Q|, which enters w and is multiplied by c        c |v_Q|
// (the double arithmetic in front of either rounding is below 2^-50 of the same scales).  Per anchor and component:
// 18 S + k |y| + c |v_Q|.  A row with n entries adds them in stored order, one rounding of a partial sum per entry, each
// partial sum at most the row's sum of S: the row's force lies within 2^-24 ((18 + n) sum S + sum (k |y| + c |v_Q|)).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "mpm_links.h"
#include "mpm_row_table.h"

namespace mpm {

constexpr unsigned ANCHOR_TENSION_ONLY = 1u;          // mpm_anchor_t::flags
constexpr unsigned ANCHOR_FLAG_BIT = 0x80000000u;     // ... as it rides in a record's slot word
constexpr unsigned ANCHOR_NO_ACC = 0xFFFFFFFFu;       // a record without an accumulator (padding)
constexpr unsigned ANCHOR_NO_SLOT = 0x7FFFFFFFu;      // a record whose body has no motion yet (anchors_ready resolves it)
constexpr int ANCHOR_SLICE = 64;

struct Anchor {   // mirrors mpm_anchor_t (include/mpm_hip.h)
    uint32_t vertex, body;
    float p_BQ[3];
    float stiffness, rest_length, damping;
    uint32_t flags;
};

// The attachment point of p_BQ on a body posed at (pt, Rt) with spatial velocity (v, w): y and v_Q in double as k_pin
// forms them, each rounded to float once.  Contraction off: every kernel that calls this gets the same bits.
MPM_LINK_FN void anchor_point(const double* pt, const double* Rt, const double* v, const double* w, const float* q, float y[3],
                              float vq[3]) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    double r[3];
    for (int i = 0; i < 3; ++i) {
        r[i] = Rt[i * 3] * (double)q[0] + Rt[i * 3 + 1] * (double)q[1] + Rt[i * 3 + 2] * (double)q[2];
        y[i] = (float)(pt[i] + r[i]);
    }
    vq[0] = (float)(v[0] + (w[1] * r[2] - w[2] * r[1]));
    vq[1] = (float)(v[1] + (w[2] * r[0] - w[0] * r[2]));
    vq[2] = (float)(v[2] + (w[0] * r[1] - w[1] * r[0]));
}

}  // namespace mpm

#ifdef __HIPCC__
#include "mpm_pins.h"
#include "mpm_step.h"

namespace mpm {

struct AnchorPose {   // one motion slot at its clock (k_anchor_pose), 176 bytes
    double pt[3], Rt[9];      // p(t), R(t)
    double p[3], v[3], w[3];  // the motion's p_WB as set, v, w
    double pad;
};
struct AnchorRec {    // one entry of the row table: AnchorRecord as the kernels read it
    float4 a;         // (bits of motion slot | ANCHOR_FLAG_BIT, k, L, c)
    float4 b;         // (p_BQ, bits of the accumulator index)
};
struct AnchorArgs {
    const int* row_pid;          // [n_rows] particle id (NfG + vertex) of the row's vertex, ascending
    const unsigned* slice_off;   // [slices + 1] first record of a slice; its width is (next - this) / 64
    const AnchorRec* ent;
    int n_rows;
    const AnchorPose* pose = nullptr;   // [n_mot] what k_anchor_pose wrote (set per launch)
    int n_mot = 0;
};
struct AnchorAcc {
    long long* body_acc;   // [n_bodies][6] (tau, f) as in k_pin
    int n_bodies;
    double imp_fix;        // DP::fix_p
};

// One lane per motion slot, in front of the kernels that read the table: sin and cos once per body and substep
__global__ __launch_bounds__(64) void k_anchor_pose(const BodyMotionDev* mot, int n_mot, AnchorPose* out) {
    const int q = (int)(blockIdx.x * 64 + threadIdx.x);
    if (q >= n_mot) return;
    const BodyMotionDev m = mot[q];
    AnchorPose o;
    pin_pose(m, m.t, o.pt, o.Rt);
    for (int i = 0; i < 3; ++i) {
        o.p[i] = m.p[i];
        o.v[i] = m.v[i];
        o.w[i] = m.w[i];
    }
    o.pad = 0.0;
    out[q] = o;
}

// Row r of the table on the current positions and velocities, and -- where REACT -- the reactions of its entries into
// the workgroup's LDS accumulators (bodies below CT_LDS_BODIES) or the global ones.  The row's own particle index comes
// through DP::imap from the id of the host-built table; a slot that is no vertex slot is reported, never used as an
// address.  A motion slot past the table (an anchor that anchors_ready has not resolved cannot reach a launch) is clamped
// and reported.  false: the row's own vertex has no slot.
template <bool REACT>
MPM_DEV bool anchor_row(const DP& p, const PSet& S, const AnchorArgs& a, int r, int& s_out, float f[3], bool& bad,
                        const AnchorAcc& acc, float dt, unsigned long long (*s_acc)[6], bool& range) {
    const unsigned b0 = a.slice_off[r >> 6], b1 = a.slice_off[(r >> 6) + 1];
    const int width = (int)((b1 - b0) / ANCHOR_SLICE);
    const int s = p.imap[a.row_pid[r]];
    s_out = s;
    if (s < p.Nf || s >= p.Np) {
        bad = true;
        return false;
    }
    const float4 xi = S.q[0][s], vi = S.q[1][s];
    const AnchorRec* ent = a.ent + b0 + (r & 63);
    float f0 = 0.f, f1 = 0.f, f2 = 0.f;
    // LINK_BATCH entries at a time, as link_row: their records first (two 16-byte loads each, independent), then the
    // pose-table reads (a few bodies: the table stays in the cache).  An entry past the width loads nothing and enters as
    // padding (the width is the slice's, and a slice is one wave: the test is uniform).
    for (int e0 = 0; e0 < width; e0 += LINK_BATCH) {
        float4 qa[LINK_BATCH], qb[LINK_BATCH];
#pragma unroll
        for (int u = 0; u < LINK_BATCH; ++u) {
            qa[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            qb[u] = make_float4(0.f, 0.f, 0.f, __uint_as_float(ANCHOR_NO_ACC));
            if (e0 + u < width) {
                qa[u] = ent[(size_t)(e0 + u) * ANCHOR_SLICE].a;
                qb[u] = ent[(size_t)(e0 + u) * ANCHOR_SLICE].b;
            }
        }
#pragma unroll
        for (int u = 0; u < LINK_BATCH; ++u) {   // (in stored order)
            if (e0 + u >= width) continue;       // (uniform; padding inside the width goes through the arithmetic: an exact zero)
            const unsigned word = __float_as_uint(qa[u].x);
            unsigned slot = word & ~ANCHOR_FLAG_BIT;
            if (slot >= (unsigned)a.n_mot) {   // (the pose table has at least one entry: anchors_ready)
                bad = true;
                slot = 0u;
            }
            const AnchorPose& m = a.pose[slot];
            const float q[3] = {qb[u].x, qb[u].y, qb[u].z};
            float y[3], vq[3], g[3];
            anchor_point(m.pt, m.Rt, m.v, m.w, q, y, vq);
            const float d[3] = {y[0] - xi.x, y[1] - xi.y, y[2] - xi.z};
            const float w[3] = {vq[0] - vi.x, vq[1] - vi.y, vq[2] - vi.z};
            link_force(qa[u].y, qa[u].z, qa[u].w, (word & ANCHOR_FLAG_BIT) != 0u, d, w, g);
            f0 += g[0];
            f1 += g[1];
            f2 += g[2];
            if (REACT) {
                const unsigned b = __float_as_uint(qb[u].w);
                if (b < (unsigned)acc.n_bodies && (g[0] != 0.f || g[1] != 0.f || g[2] != 0.f)) {
                    // the body receives -f dt (a product of two floats: exact in double), torque about the motion's p_WB
                    const double l[3] = {-(double)g[0] * (double)dt, -(double)g[1] * (double)dt, -(double)g[2] * (double)dt};
                    const double c[3] = {(double)y[0] - m.p[0], (double)y[1] - m.p[1], (double)y[2] - m.p[2]};
                    const double h[3] = {c[1] * l[2] - c[2] * l[1], c[2] * l[0] - c[0] * l[2], c[0] * l[1] - c[1] * l[0]};
                    unsigned long long* dst = b < (unsigned)CT_LDS_BODIES ? &s_acc[b][0]
                                                                          : reinterpret_cast<unsigned long long*>(acc.body_acc + (size_t)b * 6);
                    for (int i = 0; i < 3; ++i) {
                        const unsigned long long qh = (unsigned long long)imp_fixed(h[i], acc.imp_fix, range);
                        const unsigned long long ql = (unsigned long long)imp_fixed(l[i], acc.imp_fix, range);
                        if (b < (unsigned)CT_LDS_BODIES) {
                            __hip_atomic_fetch_add(dst + i, qh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            __hip_atomic_fetch_add(dst + 3 + i, ql, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        } else {
                            __hip_atomic_fetch_add(dst + i, qh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            __hip_atomic_fetch_add(dst + 3 + i, ql, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        }
                    }
                }
            }
        }
    }
    f[0] = f0; f[1] = f1; f[2] = f2;
    return true;
}

// Behind k_hinge_gather (and every other vertex-force kernel) on the same stream, with the substep's DP: a substep that
// skips itself (and is run again by the host) adds neither force nor impulse, so that both are added once.
__global__ __launch_bounds__(256) void k_anchor(DP p, AnchorArgs a, AnchorAcc acc, float dt) {
    __shared__ unsigned long long s_acc[CT_LDS_BODIES][6];
    if (gated_out(p)) return;   // (uniform)
    for (int q = threadIdx.x; q < CT_LDS_BODIES * 6; q += 256) (&s_acc[0][0])[q] = 0ull;
    __syncthreads();
    const int r = (int)(blockIdx.x * 256 + threadIdx.x);
    bool bad = false, range = false;
    if (r < a.n_rows) {
        int s;
        float f[3];
        if (anchor_row<true>(p, p.set[p.ctl->cur], a, r, s, f, bad, acc, dt, s_acc, range)) {
            // (a row that adds nothing leaves the force as it is, bit for bit: x + 0 would turn a -0 into +0)
            if (f[0] != 0.f) p.f[0][s] += f[0];
            if (f[1] != 0.f) p.f[1][s] += f[1];
            if (f[2] != 0.f) p.f[2][s] += f[2];
        }
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(&p.ctl->error, ERR_CAPACITY);
    if (__ballot(range) && (threadIdx.x & 63) == 0) atomicOr(&p.ctl->error, ERR_RANGE);
    __syncthreads();
    for (int q = threadIdx.x; q < min(acc.n_bodies, CT_LDS_BODIES) * 6; q += 256) {
        const unsigned long long v = (&s_acc[0][0])[q];
        if (v != 0ull)
            __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(acc.body_acc) + q, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// mpm_anchor_forces: out[3 (pid - NfG) ..] = the row's force (vertices without an anchor stay as the caller left them)
__global__ __launch_bounds__(256) void k_anchor_eval(DP p, AnchorArgs a, float* out) {
    const int r = (int)(blockIdx.x * 256 + threadIdx.x);
    bool bad = false, range = false;
    if (r < a.n_rows) {
        int s;
        float f[3];
        if (anchor_row<false>(p, p.set[p.ctl->cur], a, r, s, f, bad, AnchorAcc{}, 0.f, nullptr, range)) {
            float* o = out + 3 * (size_t)(a.row_pid[r] - p.NfG);
            o[0] = f[0]; o[1] = f[1]; o[2] = f[2];
        }
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(&p.ctl->error, ERR_CAPACITY);
}

// mpm_anchor_state: anchor i's point y32, its length |y32 - x| formed in double and rounded to float once, and its term
// 1/2 k (l - L)^2 formed in double from the floats y32 and x (0 for an anchor that does not act: link_active on the float
// differences, as link_force decides).  one[i] = (bits of the vertex's particle id, bits of motion slot | ANCHOR_FLAG_BIT,
// k, L) (p_BQ, 0).  A vertex without a slot is reported; the anchor then counts as of zero length.
__global__ __launch_bounds__(256) void k_anchor_energy(DP p, const AnchorRec* one, int n, const AnchorPose* pose, int n_mot, double* term,
                                                       float* length, float* point) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    bool bad = false;
    if (i < n) {
        const PSet& S = p.set[p.ctl->cur];
        const AnchorRec q = one[i];
        const int s = p.imap[(int)__float_as_uint(q.a.x)];
        const unsigned word = __float_as_uint(q.a.y);
        unsigned slot = word & ~ANCHOR_FLAG_BIT;
        bad = s < p.Nf || s >= p.Np || slot >= (unsigned)n_mot;
        if (slot >= (unsigned)n_mot) slot = 0u;
        const AnchorPose& m = pose[slot];
        const float b[3] = {q.b.x, q.b.y, q.b.z};
        float y[3], vq[3];
        anchor_point(m.pt, m.Rt, m.v, m.w, b, y, vq);
        double e = 0.0;
        float l = 0.f;
        if (!bad) {
            const float4 x = S.q[0][s];
            const float d[3] = {y[0] - x.x, y[1] - x.y, y[2] - x.z};
            const double D0 = (double)y[0] - (double)x.x, D1 = (double)y[1] - (double)x.y, D2 = (double)y[2] - (double)x.z;
            const double ld = sqrt(D0 * D0 + D1 * D1 + D2 * D2);
            l = (float)ld;
            if (link_active(q.a.w, (word & ANCHOR_FLAG_BIT) != 0u, d)) {
                const double st = ld - (double)q.a.w;
                e = .5 * (double)q.a.z * st * st;
            }
        }
        term[i] = e;
        length[i] = l;
        point[3 * i] = y[0];
        point[3 * i + 1] = y[1];
        point[3 * i + 2] = y[2];
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(&p.ctl->error, ERR_CAPACITY);
}

}  // namespace mpm
#endif  // __HIPCC__

namespace mpm {

// The table k_anchor reads, as the host lays it out (no device is touched), and the sums of the stability guard
struct AnchorRecord {
    uint32_t slot;        // the body's motion slot (ANCHOR_NO_SLOT: none yet) | ANCHOR_FLAG_BIT for a tension-only anchor
    float k, L, c;
    float p_BQ[3];
    uint32_t acc;         // the body, as the index of its accumulator; ANCHOR_NO_ACC: padding
};
struct AnchorOne {
    uint32_t pid, slot;   // the vertex's particle id; the motion slot | ANCHOR_FLAG_BIT
    float k, L;
    float p_BQ[3];
    uint32_t pad;         // k_anchor_energy's record
};
struct AnchorTable : RowTable<AnchorRecord> {
    std::vector<AnchorOne> one;        // [anchor] k_anchor_energy's records
    std::vector<double> k_sum, c_sum;  // [row] sum of k, sum of c over the row's anchors
    bool unresolved = false;           // some record carries ANCHOR_NO_SLOT
};

// What mpm_set_anchors refuses, in the caller's numbering; empty: the table is fine
inline std::string anchor_table_refusal(const Anchor* anchors, size_t n, size_t n_verts) {
    if (!(n < (size_t)1 << 31)) return "anchors: the table is too large";
    for (size_t i = 0; i < n; ++i) {
        const Anchor& q = anchors[i];
        const std::string at = "anchors: anchor " + std::to_string(i);
        if (q.vertex >= n_verts) return at + " names a vertex that does not exist";
        if (!(std::isfinite(q.p_BQ[0]) && std::isfinite(q.p_BQ[1]) && std::isfinite(q.p_BQ[2]))) return at + ": p_BQ is not finite";
        if (!(std::isfinite(q.stiffness) && q.stiffness >= 0.f && std::isfinite(q.rest_length) && q.rest_length >= 0.f &&
              std::isfinite(q.damping) && q.damping >= 0.f))
            return at + ": stiffness, rest_length or damping is negative or not finite";
        if (q.flags & ~ANCHOR_TENSION_ONLY) return at + ": unknown flags";
    }
    return std::string();
}

// anchors: n checked anchors (anchor_table_refusal); nf: faces in front of the vertices in the particle numbering;
// slot_of(body): the body's motion slot, or ANCHOR_NO_SLOT; slice: rows per slice (ANCHOR_SLICE).  false with `why` set:
// the table does not fit 2^31 records.
template <class SlotOf>
inline bool anchor_table(const Anchor* anchors, size_t n, size_t nf, size_t n_verts, size_t slice, SlotOf slot_of, AnchorTable& out,
                         std::string& why) {
    out = AnchorTable{};
    // rows in ascending vertex id, a row's entries in anchor order: a counting sort over the vertices
    std::vector<size_t> first(n_verts + 1, 0);
    for (size_t i = 0; i < n; ++i) first[(size_t)anchors[i].vertex + 1] += 1;
    for (size_t v = 0; v < n_verts; ++v) first[v + 1] += first[v];
    std::vector<AnchorRecord> flat(n);
    {
        std::vector<size_t> fill(first.begin(), first.end() - 1);
        for (size_t i = 0; i < n; ++i) {
            const Anchor& q = anchors[i];
            const uint32_t flag = q.flags & ANCHOR_TENSION_ONLY ? ANCHOR_FLAG_BIT : 0u;
            const uint32_t slot = (uint32_t)slot_of(q.body) & ~ANCHOR_FLAG_BIT;
            out.unresolved |= slot == ANCHOR_NO_SLOT;
            flat[fill[q.vertex]++] = AnchorRecord{slot | flag, q.stiffness, q.rest_length, q.damping, {q.p_BQ[0], q.p_BQ[1], q.p_BQ[2]}, q.body};
            out.one.push_back(AnchorOne{(uint32_t)(nf + q.vertex), slot | flag, q.stiffness, q.rest_length, {q.p_BQ[0], q.p_BQ[1], q.p_BQ[2]}, 0u});
        }
    }
    std::vector<size_t> row_vertex;
    for (size_t v = 0; v < n_verts; ++v)
        if (first[v + 1] > first[v]) {
            row_vertex.push_back(v);
            out.row_pid.push_back((int)(nf + v));
            double ks = 0.0, cs = 0.0;
            for (size_t q = first[v]; q < first[v + 1]; ++q) {
                ks += (double)flat[q].k;
                cs += (double)flat[q].c;
            }
            out.k_sum.push_back(ks);
            out.c_sum.push_back(cs);
        }
    if (!sliced_ell(row_vertex.size(), slice, [&](size_t r) { return first[row_vertex[r] + 1] - first[row_vertex[r]]; },
                    [&](size_t r, size_t q) { return flat[first[row_vertex[r]] + q]; },
                    [&](size_t) { return AnchorRecord{0u, 0.f, 0.f, 0.f, {0.f, 0.f, 0.f}, ANCHOR_NO_ACC}; }, out.slice_off, out.ent)) {
        why = "anchors: the table is too large";
        return false;
    }
    return true;
}

// The guard's rates on the vertices' masses (mass[vertex]).  The body's end of an anchor is prescribed, so the factor is
// 1 where a link, whose two ends move, has 2: W = max_i (1 / m_i) sum k, G = max_i (1 / m_i) sum c over vertex i's
// anchors; the limit is link_limit(W, G).
inline void anchor_rates(const AnchorTable& t, const float* mass, size_t nf, double* W, double* G) {
    auto m = [&](size_t r) { return mass[(size_t)t.row_pid[r] - nf]; };
    *W = max_row_rate(t.k_sum.data(), t.row_pid.size(), 1.0, m);
    *G = max_row_rate(t.c_sum.data(), t.row_pid.size(), 1.0, m);
}

}  // namespace mpm
