// Links between cloth vertices (mpm_set_links, include/mpm_hip.h): seams, springs and tension-only cords that join two
// distinct vertices a, b of the same cloth or of two cloths.  With d = x_b - x_a and w = v_b - v_a the force on a is
//   seam   (L == 0)  f_j = fma(k, d_j, c w_j)                                  linear, isotropic, no square root
//   spring (L > 0)   l2 = fma(d2, d2, fma(d1, d1, d0 d0)),  l = sqrt(l2),  s = fma(w2, d2, fma(w1, d1, w0 d0)) / l,
//                    t = fma(c, s, k (l - L)),  g = t / l,  f_j = g d_j;       nothing where l2 < 1e-30
//   MPM_LINK_TENSION_ONLY: nothing (elastic and damping part alike) unless l > L, l the float above
// and the force on b is its negative.  One inline function, link_force, is what k_link calls per entry and what the host
// entry mpm_link_force runs: every operation written out, contraction off, the square root and both divisions
// correctly rounded.  Every intermediate is even (l2, l, s, t, g) or odd (d, w, f) in (d, w), and a float difference
// changes sign exactly when its operands are swapped: the force evaluated from b's side is, bit for bit, the negative of
// the force from a's side.  That is what lets a gather kernel -- one lane per linked vertex, no atomics -- conserve the
// momentum link by link.
//
// Host: link_table lays the caller's links out (mpm_set_links, whose device half is in mpm_cloth_host.h) and forms the
// sums of the stability guard.  Device: k_link, one lane per vertex with at least one link, adds to the vertex forces
// k_vforce (and k_bend, k_bend_damp) left in DP::f (launch_fem_vertices); k_link_eval writes the same numbers into a
// buffer in original vertex order (mpm_link_forces); k_link_energy forms one double term and one float length per link
// (mpm_link_energy).  The table is a vertex row table (mpm_row_table.h: sliced ELL, slices of 64 rows) with one row per
// linked vertex; a row's entries are that vertex's links in link order, so a link appears in two rows.  An entry is one
// 16-byte record (the other end's particle id with the tension-only flag in bit 31, which an id cannot use; k; L; c --
// the caller's floats, no host rounding enters): a wave reads 1 KiB of contiguous records per step.  The padding record
// is (the row's own id, 0, 0, 0), an exact zero through the seam branch.  Table and order are those of the original
// vertex ids: the result is the same bits whatever the particle order.
//
// Roundings of one component of one link's force, for the bound of tests/links.py (first order, in units of 2^-24 of
// S = k (l + L) + c |w|; the cancellation in l - L is at the scale of l + L, not of the stretch):
//   spring  d = x_b - x_a (1) and l2's three roundings (1.5 on l) and the square root (1): l carries 3.5
//           elastic part of t: k times [3.5 (l) + 1 (l - L)] + 1 (the product k (l - L))                   5.5 k (l + L)
//           s = (w . d) / l: w (1), d (1), the dot product's three roundings (3), the division (1), l (3.5)  9.5 c |w|
//           t's own fused multiply-add                                                                     1
//           g = t / l: the division (1) and l again (3.5)                                                  4.5
//           f_j = g d_j: the product (1) and d_j (1)                                                       2
//           in all at most 10.5 + 4.5 + 2 = 17
//   seam    d (1), w (1), c w_j (1), the fused multiply-add (1) = 4
// R_link = 18 (17 and one more for the second-order terms).  A row with n entries adds them in stored order, one
// rounding of a partial sum per entry, each partial sum at most the row's sum of S: R_i = 18 + n_i, on sum S.
//
// Breakable links (mpm_set_link_limits, mpm_set_broken_links, mpm_link_break_state, mpm_link_break_measure,
// mpm_link_breaks): link i may carry a break_length b_i (0: never breaks; else finite and > L).  The host forms
// B2_i = (float)((double)b_i (double)b_i), rounded once; link_breaks, shared by host and device, forms link_force's l2
// from d = x_b - x_a and answers l2 > B2 -- no square root, even in d, false for a NaN.  State: one byte per link in link
// order, monotone (a substep only sets it; mpm_set_broken_links alone clears it).  k_link_break, one lane per link, runs
// immediately in front of k_link while the breaking tables exist (some limit > 0 or some flag set): a link that is
// broken, or has B2 == 0, returns at once; otherwise its two ids come from k_link_energy's pair record, its two slots
// through DP::imap, its two positions from the current set -- three round trips of independent loads -- and where
// link_breaks says so the lane sets the byte and overwrites the link's two entries of LinkArgs::ent (entry_of_link,
// which link_table emits) with the rows' padding records (own id, 0, 0, 0): plain stores, one writer per link, an exact
// +0 through the seam branch.  k_link, behind it on the stream and unchanged, never sees the broken link again, in the
// substep in which it breaks included: elastic and damping part, every kind of link, both ends.  The verdict is formed
// once per link on the positions of the substep's start (Jacobi): it does not depend on the other links, the particle
// order or deterministic mode, and a substep that skips itself (gated_out) marks nothing.  No atomics but the error flag.
// mpm_set_broken_links rebuilds ent on the host with the flagged links' entries padded and uploads it into the arrays in
// force: that is also how a restore brings a link back.  mpm_links_max_stable_dt does NOT change when links break: it is
// formed over the whole table, and breaking only removes non-negative terms from its row sums, so it stays a valid, more
// conservative, guard.  Anchors (mpm_anchors.h) do not break yet.
// Roundings of l2 (first order, units of 2^-24 of l2): each d_j carries 1, so each square 2; the product and the two
// fused multiply-adds one each on partial sums of at most l2: 5, R_BREAK = 6 with one more for the second-order terms.
// The cost of k_link_break on an MI355X: 5.2 us per substep on cloth_1m with one link per vertex (168,200 links, limits
// on, none broken), k_link unchanged against the parent; a substep in which many links break has NOT been measured
// (DESIGN.md section 3.3p).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "mpm_row_table.h"

#ifdef __HIPCC__
#define MPM_LINK_FN __host__ __device__ inline
#else
#define MPM_LINK_FN inline
#endif

namespace mpm {

constexpr unsigned LINK_TENSION_ONLY = 1u;   // mpm_link_t::flags
constexpr unsigned LINK_FLAG_BIT = 0x80000000u;   // ... as it rides in a record's id word
constexpr int LINK_SLICE = 64, LINK_BATCH = 8;

struct Link {   // mirrors mpm_link_t (include/mpm_hip.h)
    uint32_t a, b;
    float stiffness, rest_length, damping;
    uint32_t flags;
};

// The force on the end the differences are taken FROM: d = x_other - x_own, w = v_other - v_own.  No branch: both laws
// are evaluated and one is selected (a lane of k_link holds entries of every kind); where l = 0 the spring's quotients
// are not finite and are never selected (l2 < 1e-30).
MPM_LINK_FN void link_force(float k, float L, float c, bool tension_only, const float d[3], const float w[3], float f[3]) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const float l2 = fmaf(d[2], d[2], fmaf(d[1], d[1], d[0] * d[0]));
    const float l = sqrtf(l2);
    const float s = fmaf(w[2], d[2], fmaf(w[1], d[1], w[0] * d[0])) / l;
    const float t = fmaf(c, s, k * (l - L));
    const float g = t / l;
    const bool spring = L > 0.f;
    const bool on = (!spring | (l2 >= 1e-30f)) & (!tension_only | (l > L));
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float seam = fmaf(k, d[j], c * w[j]);
        const float v = spring ? g * d[j] : seam;
        f[j] = on ? v : 0.f;
    }
}

// whether a link with these parameters acts at the float differences d (link_force's `on`)
MPM_LINK_FN bool link_active(float L, bool tension_only, const float d[3]) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const float l2 = fmaf(d[2], d[2], fmaf(d[1], d[1], d[0] * d[0]));
    return (!(L > 0.f) | (l2 >= 1e-30f)) & (!tension_only | (sqrtf(l2) > L));
}

// whether a link breaks at the float differences d against B2 = (float)(break_length^2): l2 is link_force's, the
// comparison is false for a NaN; *l2_out gets l2.  (The caller decides what B2 == 0 means.)
MPM_LINK_FN bool link_breaks(const float d[3], float B2, float* l2_out) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const float l2 = fmaf(d[2], d[2], fmaf(d[1], d[1], d[0] * d[0]));
    *l2_out = l2;
    return l2 > B2;
}

}  // namespace mpm

#ifdef __HIPCC__
#include "mpm_step.h"

namespace mpm {

struct LinkArgs {
    const int* row_pid;          // [n_rows] particle id (NfG + vertex) of the row's vertex, ascending
    const unsigned* slice_off;   // [slices + 1] first record of a slice; its width is (next - this) / 64
    const float4* ent;           // records (bits of the other end's particle id | LINK_FLAG_BIT, k, L, c)
    int n_rows;
};

// Row r of the table on the current positions and velocities.  Every index into a per-particle array comes through
// DP::imap from an id of the host-built table; a slot that is no vertex slot (a particle this engine does not hold) is
// reported, never used as an address: the entry then reads the row's own record (zero differences: an exact zero in
// either branch).  false: the row's own vertex has no slot.
MPM_DEV bool link_row(const DP& p, const PSet& S, const LinkArgs& a, int r, int& s_out, float f[3], bool& bad) {
    const unsigned b0 = a.slice_off[r >> 6], b1 = a.slice_off[(r >> 6) + 1];
    const int width = (int)((b1 - b0) / LINK_SLICE);
    const int s = p.imap[a.row_pid[r]];
    s_out = s;
    if (s < p.Nf || s >= p.Np) {
        bad = true;
        return false;
    }
    const float4 xi = S.q[0][s], vi = S.q[1][s];
    const float4* ent = a.ent + b0 + (r & 63);
    float f0 = 0.f, f1 = 0.f, f2 = 0.f;
    // LINK_BATCH entries at a time: their records, then their slots, then their positions and velocities -- three round
    // trips of independent loads per batch instead of dependent pairs per entry (k_bend's lesson).  An entry past the
    // width loads nothing and enters as padding: the row's own id and record, k = L = c = 0 (skipping those loads took
    // k_link from 29.6 to 24.6 us on cloth_1m with one link per vertex).
    for (int e0 = 0; e0 < width; e0 += LINK_BATCH) {
        float4 q[LINK_BATCH];
        int sj[LINK_BATCH];
        float4 xj[LINK_BATCH], vj[LINK_BATCH];
        // (the width is the slice's, and a slice is one wave: `live` is the same in all 64 lanes, its branches skip)
#pragma unroll
        for (int u = 0; u < LINK_BATCH; ++u) {
            q[u] = make_float4(__uint_as_float((unsigned)a.row_pid[r]), 0.f, 0.f, 0.f);
            if (e0 + u < width) q[u] = ent[(size_t)(e0 + u) * LINK_SLICE];
        }
#pragma unroll
        for (int u = 0; u < LINK_BATCH; ++u) {
            sj[u] = s;
            if (e0 + u < width) sj[u] = p.imap[(int)(__float_as_uint(q[u].x) & ~LINK_FLAG_BIT)];
        }
#pragma unroll
        for (int u = 0; u < LINK_BATCH; ++u) {
            const bool ok = sj[u] >= p.Nf && sj[u] < p.Np;
            bad |= !ok;
            xj[u] = xi;
            vj[u] = vi;
            if (e0 + u < width) {
                const int t = ok ? sj[u] : s;
                xj[u] = S.q[0][t];
                vj[u] = S.q[1][t];
            }
        }
#pragma unroll
        for (int u = 0; u < LINK_BATCH; ++u) {   // (in stored order)
            const float d[3] = {xj[u].x - xi.x, xj[u].y - xi.y, xj[u].z - xi.z};
            const float w[3] = {vj[u].x - vi.x, vj[u].y - vi.y, vj[u].z - vi.z};
            float g[3];
            link_force(q[u].y, q[u].z, q[u].w, (__float_as_uint(q[u].x) & LINK_FLAG_BIT) != 0u, d, w, g);
            f0 += g[0];
            f1 += g[1];
            f2 += g[2];
        }
    }
    f[0] = f0; f[1] = f1; f[2] = f2;
    return true;
}

// Behind k_vforce (and k_bend, k_bend_damp) on the same stream, with the substep's DP: a substep that skips itself (and
// is run again by the host) adds nothing, so that the force is added once.
__global__ __launch_bounds__(256) void k_link(DP p, LinkArgs a) {
    if (gated_out(p)) return;
    const int r = (int)(blockIdx.x * 256 + threadIdx.x);
    bool bad = false;
    if (r < a.n_rows) {
        int s;
        float f[3];
        if (link_row(p, p.set[p.ctl->cur], a, r, s, f, bad)) {
            p.f[0][s] += f[0];
            p.f[1][s] += f[1];
            p.f[2][s] += f[2];
        }
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(&p.ctl->error, ERR_CAPACITY);
}

// mpm_link_forces: out[3 (pid - NfG) ..] = the row's force (vertices without a link stay as the caller left them: zero)
__global__ __launch_bounds__(256) void k_link_eval(DP p, LinkArgs a, float* out) {
    const int r = (int)(blockIdx.x * 256 + threadIdx.x);
    bool bad = false;
    if (r < a.n_rows) {
        int s;
        float f[3];
        if (link_row(p, p.set[p.ctl->cur], a, r, s, f, bad)) {
            float* o = out + 3 * (size_t)(a.row_pid[r] - p.NfG);
            o[0] = f[0]; o[1] = f[1]; o[2] = f[2];
        }
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(&p.ctl->error, ERR_CAPACITY);
}

// mpm_link_energy: link i's term 1/2 k (l - L)^2, formed in double from the float positions (0 for a link that does
// not act: link_active on the float differences, as link_force decides), and its length, formed in double and rounded
// to float once.  pair[i] = (bits of a's
// particle id, bits of b's | LINK_FLAG_BIT, k, L).  An end without a vertex slot is reported; the link then counts as
// of zero length.  broken (may be null): the flags of the breakable links; a broken link's term is 0, its length is
// reported like any other.
__global__ __launch_bounds__(256) void k_link_energy(DP p, const float4* pair, int n, const uint8_t* broken, double* term,
                                                     float* length) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    bool bad = false;
    if (i < n) {
        const PSet& S = p.set[p.ctl->cur];
        const float4 q = pair[i];
        const int sa = p.imap[(int)__float_as_uint(q.x)], sb = p.imap[(int)(__float_as_uint(q.y) & ~LINK_FLAG_BIT)];
        const bool ok = sa >= p.Nf && sa < p.Np && sb >= p.Nf && sb < p.Np;
        bad = !ok;
        double e = 0.0;
        float l = 0.f;
        if (ok) {
            const float4 xa = S.q[0][sa], xb = S.q[0][sb];
            const float d[3] = {xb.x - xa.x, xb.y - xa.y, xb.z - xa.z};
            const double D0 = (double)xb.x - (double)xa.x, D1 = (double)xb.y - (double)xa.y, D2 = (double)xb.z - (double)xa.z;
            const double ld = sqrt(D0 * D0 + D1 * D1 + D2 * D2);
            l = (float)ld;
            const bool gone = broken && broken[i] != 0;
            if (!gone && link_active(q.w, (__float_as_uint(q.y) & LINK_FLAG_BIT) != 0u, d)) {
                const double st = ld - (double)q.w;
                e = .5 * (double)q.z * st * st;
            }
        }
        term[i] = e;
        length[i] = l;
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(&p.ctl->error, ERR_CAPACITY);
}

struct LinkBreakArgs {
    const float4* pair;         // [link] k_link_energy's records: the two ends' particle ids
    const float* B2;            // [link] (float)(break_length^2), 0: never breaks; nullptr: the tables do not exist
    const unsigned* entry;      // [2 link] where the link's two entries are in `ent`: a's row, then b's row
    uint8_t* broken;            // [link] 0 intact, 1 broken
    float4* ent;                // LinkArgs::ent of the table in force
    int n;
};

// Link i's float differences d = x_b - x_a on the current set, three round trips of independent loads (ids, slots,
// positions).  false, with `bad` set: an end has no vertex slot; nothing is read through it.
MPM_DEV bool link_ends(const DP& p, const PSet& S, const float4* pair, int i, unsigned& ida, unsigned& idb, float d[3], bool& bad) {
    const float4 q = pair[i];
    ida = __float_as_uint(q.x);
    idb = __float_as_uint(q.y) & ~LINK_FLAG_BIT;
    const int sa = p.imap[(int)ida], sb = p.imap[(int)idb];
    if (!(sa >= p.Nf && sa < p.Np && sb >= p.Nf && sb < p.Np)) {
        bad = true;
        return false;
    }
    const float4 xa = S.q[0][sa], xb = S.q[0][sb];
    d[0] = xb.x - xa.x;
    d[1] = xb.y - xa.y;
    d[2] = xb.z - xa.z;
    return true;
}

// Immediately in front of k_link on the same stream, with the substep's DP, while the breaking tables exist: one lane
// per link.  A link that breaks is marked and loses its two entries of the table k_link is about to read (one writer per
// link: plain stores); a substep that skips itself marks nothing.
__global__ __launch_bounds__(256) void k_link_break(DP p, LinkBreakArgs a) {
    if (gated_out(p)) return;
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    bool bad = false;
    if (i < a.n && a.broken[i] == 0) {
        const float B2 = a.B2[i];
        if (B2 != 0.f) {
            unsigned ida, idb;
            float d[3], l2;
            if (link_ends(p, p.set[p.ctl->cur], a.pair, i, ida, idb, d, bad) && link_breaks(d, B2, &l2)) {
                a.broken[i] = 1;
                a.ent[a.entry[2 * (size_t)i]] = make_float4(__uint_as_float(ida), 0.f, 0.f, 0.f);
                a.ent[a.entry[2 * (size_t)i + 1]] = make_float4(__uint_as_float(idb), 0.f, 0.f, 0.f);
            }
        }
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(&p.ctl->error, ERR_CAPACITY);
}

// mpm_link_break_measure: l2 and the would-break verdict per link on the current state, broken links like the others;
// the verdict is 0 for a link without a limit and while the tables do not exist (B2 == nullptr).  An end without a
// vertex slot is reported; the link then gets l2 = 0 and verdict 0.  Changes no state.
__global__ __launch_bounds__(256) void k_link_break_eval(DP p, const float4* pair, const float* B2, int n, float* l2_out,
                                                         uint8_t* breaks_out) {
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    bool bad = false;
    if (i < n) {
        const float b2 = B2 ? B2[i] : 0.f;
        unsigned ida, idb;
        float d[3], l2 = 0.f;
        bool breaks = false;
        if (link_ends(p, p.set[p.ctl->cur], pair, i, ida, idb, d, bad)) breaks = link_breaks(d, b2, &l2);
        l2_out[i] = l2;
        breaks_out[i] = (b2 != 0.f && breaks) ? 1 : 0;
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(&p.ctl->error, ERR_CAPACITY);
}

}  // namespace mpm
#endif  // __HIPCC__

namespace mpm {

// The table k_link reads, as the host lays it out (no device is touched), and the sums of the stability guard
struct LinkRecord {
    uint32_t id;          // the other end's particle id (nf + vertex) | LINK_FLAG_BIT for a tension-only link
    float k, L, c;        // LinkArgs::ent's float4
};
struct LinkPair {
    uint32_t a, b;        // the ends' particle ids, b's | LINK_FLAG_BIT for a tension-only link
    float k, L;           // k_link_energy's float4
};
struct LinkTable : RowTable<LinkRecord> {
    std::vector<LinkPair> pair;        // [link] k_link_energy's records
    std::vector<double> k_sum, c_sum;  // [row] sum of k, sum of c over the row's links
    std::vector<unsigned> entry_of_link;   // [2 link] where the link's entry in a's row, then in b's row, is in `ent`
};

// What mpm_set_links refuses, in the caller's numbering; empty: the table is fine
inline std::string link_table_refusal(const Link* links, size_t n, size_t n_verts) {
    if (!(n < (size_t)1 << 30)) return "links: the table is too large";
    for (size_t i = 0; i < n; ++i) {
        const Link& q = links[i];
        const std::string at = "links: link " + std::to_string(i);
        if (q.a >= n_verts || q.b >= n_verts) return at + " names a vertex that does not exist";
        if (q.a == q.b) return at + " joins a vertex to itself";
        if (!(std::isfinite(q.stiffness) && q.stiffness >= 0.f && std::isfinite(q.rest_length) && q.rest_length >= 0.f &&
              std::isfinite(q.damping) && q.damping >= 0.f))
            return at + ": stiffness, rest_length or damping is negative or not finite";
        if (q.flags & ~LINK_TENSION_ONLY) return at + ": unknown flags";
    }
    return std::string();
}

// links: n checked links (link_table_refusal); nf: faces in front of the vertices in the particle numbering; slice: rows
// per slice (LINK_SLICE).  false with `why` set: the table does not fit 2^31 records.
inline bool link_table(const Link* links, size_t n, size_t nf, size_t n_verts, size_t slice, LinkTable& out, std::string& why) {
    out = LinkTable{};
    // rows in ascending vertex id, a row's entries in link order: a counting sort over the vertices
    std::vector<size_t> first(n_verts + 1, 0);
    for (size_t i = 0; i < n; ++i) {
        first[(size_t)links[i].a + 1] += 1;
        first[(size_t)links[i].b + 1] += 1;
    }
    for (size_t v = 0; v < n_verts; ++v) first[v + 1] += first[v];
    std::vector<LinkRecord> flat(2 * n);
    std::vector<size_t> flat_of_link(2 * n);   // (a link's two places in `flat`: duplicate pairs get places of their own)
    {
        std::vector<size_t> fill(first.begin(), first.end() - 1);
        for (size_t i = 0; i < n; ++i) {
            const Link& q = links[i];
            const uint32_t flag = q.flags & LINK_TENSION_ONLY ? LINK_FLAG_BIT : 0u;
            flat_of_link[2 * i] = fill[q.a];
            flat[fill[q.a]++] = LinkRecord{(uint32_t)(nf + q.b) | flag, q.stiffness, q.rest_length, q.damping};
            flat_of_link[2 * i + 1] = fill[q.b];
            flat[fill[q.b]++] = LinkRecord{(uint32_t)(nf + q.a) | flag, q.stiffness, q.rest_length, q.damping};
            out.pair.push_back(LinkPair{(uint32_t)(nf + q.a), (uint32_t)(nf + q.b) | flag, q.stiffness, q.rest_length});
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
    // (padding: the row's own id and zeros)
    if (!sliced_ell(row_vertex.size(), slice, [&](size_t r) { return first[row_vertex[r] + 1] - first[row_vertex[r]]; },
                    [&](size_t r, size_t q) { return flat[first[row_vertex[r]] + q]; },
                    [&](size_t r) { return LinkRecord{(uint32_t)out.row_pid[r], 0.f, 0.f, 0.f}; }, out.slice_off, out.ent)) {
        why = "links: the table is too large";
        return false;
    }
    // entry q of row r is at slice_off[r / slice] + q slice + r % slice (mpm_row_table.h)
    std::vector<size_t> row_of_vertex(n_verts, 0);
    for (size_t r = 0; r < row_vertex.size(); ++r) row_of_vertex[row_vertex[r]] = r;
    out.entry_of_link.resize(2 * n);
    for (size_t i = 0; i < n; ++i)
        for (size_t end = 0; end < 2; ++end) {
            const size_t v = end ? links[i].b : links[i].a, r = row_of_vertex[v], q = flat_of_link[2 * i + end] - first[v];
            out.entry_of_link[2 * i + end] = (unsigned)((size_t)out.slice_off[r / slice] + q * slice + r % slice);
        }
    return true;
}

// mpm_set_link_limits: B2[i] = (float)((double)b_i (double)b_i) for n checked limits; the refusal in the caller's
// numbering, empty where the limits are fine.  (A non-zero limit whose square rounds to 0 is refused too: B2 == 0 is
// what the kernel reads as "never breaks".)
inline std::string link_limits(const float* break_length, const Link* links, size_t n, float* B2) {
    for (size_t i = 0; i < n; ++i) {
        const float b = break_length[i];
        const std::string at = "link limits: link " + std::to_string(i);
        if (!std::isfinite(b) || b < 0.f) return at + ": break_length is negative or not finite";
        if (b != 0.f && !(b > links[i].rest_length)) return at + ": break_length is neither 0 nor > rest_length";
        B2[i] = (float)((double)b * (double)b);
        if (!std::isfinite(B2[i]) || (b != 0.f && !(B2[i] > 0.f))) return at + ": the square of break_length is not a finite positive float";
    }
    return std::string();
}

// The guard's rates on the vertices' masses (mass[vertex]): W = max_i (2 / m_i) sum_j k_ij, G = max_i (2 / m_i) sum_j c_ij
inline void link_rates(const LinkTable& t, const float* mass, size_t nf, double* W, double* G) {
    auto m = [&](size_t r) { return mass[(size_t)t.row_pid[r] - nf]; };
    *W = max_row_rate(t.k_sum.data(), t.row_pid.size(), 2.0, m);
    *G = max_row_rate(t.c_sum.data(), t.row_pid.size(), 2.0, m);
}
// mpm_links_max_stable_dt: symplectic Euler on x'' = -W x - G x' (v' = v + dt (-W x - G v), x' = x + dt v') is stable
// iff W dt^2 + 2 G dt <= 4.  The positive root of that quadratic, 4 / (G + sqrt(G^2 + 4 W)) (2 / G where W = 0), as the
// float not above it; INFINITY when nothing limits the step.  W and G are maxima over rows that need not be one row's, and
// a table's stiffness and damping matrices need not commute: the root is a bound all the same (tests/test_guards.py takes
// the one-step matrix's spectral radius; DESIGN.md, "What the dt guards bound", has the margins).  It bounds the links'
// force alone, with every spring at its rest length; the load W dt^2 + 2 G dt is convex in dt and 4 at the root, so the
// loads of several such guards in force sum to at most 4 at dt = 1 / sum (1 / root).
inline float link_limit(double W, double G) {
    if (!(W > 0.0) && !(G > 0.0)) return INFINITY;
    if (!std::isfinite(W) || !std::isfinite(G)) return 0.f;
    const double lim = 4.0 / (G + std::sqrt(G * G + 4.0 * W));
    float dt = (float)lim;
    while (dt > 0.f && ((double)dt > lim || W * (double)dt * (double)dt + 2.0 * G * (double)dt > 4.0)) dt = std::nextafterf(dt, 0.f);
    return dt;
}

}  // namespace mpm
