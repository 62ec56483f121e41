// Enclosed-volume pressure per cloth (mpm_set_pressure, include/mpm_hip.h): a gauge pressure g acts on every face of a
// pressurised cloth along its winding normal.  Per cloth,
//   MPM_PRESSURE_CONSTANT  g = the caller's p: any finite value, either sign, the mesh may be open (a follower load of p
//                          per unit of CURRENT area)
//   MPM_PRESSURE_GAS       an isothermal gas in a closed, consistently wound cloth: with V the cloth's current signed
//                          volume, g = min(pv / V, p_max) - p_ambient where V > 0 and g = p_max - p_ambient otherwise,
//                          formed in double and rounded to float once: never a NaN or an infinity; a collapsed or
//                          inverted cloth gets the capped pressure, and mpm_pressure_state says so
// Volume: V = 1/6 sum_faces x_a . (x_b x x_c), every term formed in double from the float positions, summed in id order.
// Force on vertex i: every face around it, rotated cyclically to read (i, b, c), gives (x_b - x_i) x (x_c - x_i); the
// entries are added in ascending face id, then multiplied ONCE by g / 6:
//   f_i = (g / 6) sum (x_b - x_i) x (x_c - x_i)
// all in float, every operation written out, contraction off (pressure_entry and pressure_scale below: what k_pressure
// calls per entry and what the host entry mpm_pressure_vertex_force runs).  Differences only: the force is translation
// invariant to the bit.  On an interior vertex of a closed, consistently wound mesh this is exactly g dV/dx_i (the terms
// x_i x sum (x_b - x_c) cancel around a closed fan), so the force is conservative: E = -p V for a constant pressure,
// E = -pv ln V + p_ambient V for the gas while it is not capped.
//
// NO dt GUARD.  The gas's stiffness is (pv / V^2) grad V grad V^T plus a geometric term; it depends on the state and is
// unbounded as V -> 0 below the cap.  A limit computed at the rest shape would promise something it cannot keep, so
// there is none: mpm_pressure_state lets a caller watch V and g.
//
// Device: three kernels behind k_link in launch_fem_vertices, every one starting with gated_out(p) (a substep that skips
// itself and is run again by the host adds the force once).  k_pressure_volume, one workgroup of 256 per chunk of at most
// PRESSURE_CHUNK consecutive original face ids that never straddle a cloth, forms the chunk's sum of x_a . (x_b x x_c)
// (lanes in the fixed tree of measure_reduce_store: xor shuffles inside a wave, then the four waves in ascending order);
// k_pressure_gauge, one workgroup per cloth, adds the cloth's chunk sums in the fixed order of k_measure_final (eight
// contiguous runs, each ascending, then the runs ascending), forms g and writes {V, E, g, capped} per cloth into device
// memory: no host round trip, a batch of substeps stays on the device.  Both run in a substep only where some cloth is
// in gas mode, and then over the gas cloths' faces alone.  k_pressure, one lane per row of a vertex row table
// (mpm_row_table.h; one row per vertex of a pressurised cloth, 8-byte records (particle id of b, particle id of c) in
// ascending face id, padding (own id, own id): both differences are zero, an exact zero whatever the state), adds the
// row's force to DP::f.  Table, chunk list and order are those of the original ids: V, g and the forces are the same
// bits whatever the particle order.  No atomics but the error flag.
//
// VENTED GAS (mpm_set_tear_coupling with MPM_TEAR_VENTS_GAS, mpm_pressure_vented): a cloth in gas mode with at least one
// torn face (mpm_tear.h) is VENTED: its gauge is +0.0f, its energy 0, capped 0; its volume is still reported.  "Vented" is
// not stored: k_pressure_volume reads the tear flag of every face it visits (by the same original id, in the same round
// trip as the corner ids), ORs them along the sum's path and writes one word per chunk beside the partial sum;
// k_pressure_gauge ORs the cloth's chunks in its fixed order and, if any is set, writes the vented state and does not
// form a gauge.  Re-evaluated in every substep and in every query from the flags, so a restored cloth
// (mpm_set_torn_faces) re-inflates by the gas law on its current volume.  k_pressure is unchanged: it reads the state's
// gauge, and s = 0 / 6 makes every force an exact zero.  k_tear runs with the face kernels, in front of these, so a face
// that fails in a substep vents its cloth in that same substep.  The pointer to the flags is set per launch and null unless
// the mode is set and the tear tables exist: null is the arithmetic and the stores of an engine without the mode.
// NOT MODELLED: a leak rate and partial venting.  One torn face empties the cloth at once, whatever the size of the hole,
// and pv does not change: the gas is all there again when the faces are restored.
//
// Roundings of one component of a row's force, for the bound of tests/pressure.py, in units of 2^-24 of
// T = |g| / 6 sum_entries |d_b| |d_c|, d_b = x_b - x_i, d_c = x_c - x_i:
//   one entry's component d_b[j] d_c[k] - d_b[k] d_c[j]: each product carries its two differences (1 + 1) and its own
//   rounding (1), and |d_b[j] d_c[k]| + |d_b[k] d_c[j]| <= |d_b| |d_c| (Cauchy-Schwarz): 3; the subtraction: 1      4
//   g / 6 (1) and the one product with it (1)                                                                        2
//   second-order terms                                                                                               1
// R_pressure = 7.  A row with n entries adds them in stored order, one rounding of a partial sum per entry, each partial
// sum at most sum |d_b| |d_c|: R_i = 7 + n_i.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "mpm_row_table.h"

#ifdef __HIPCC__
#define MPM_PRESSURE_FN __host__ __device__ inline
#else
#define MPM_PRESSURE_FN inline
#endif

namespace mpm {

constexpr unsigned PRESSURE_OFF = 0u, PRESSURE_CONSTANT = 1u, PRESSURE_GAS = 2u;   // mpm_cloth_pressure_t::mode
constexpr int PRESSURE_SLICE = 64, PRESSURE_BATCH = 8;
constexpr int PRESSURE_CHUNK = 1024;   // face ids per chunk: four per lane of a 256-lane workgroup
constexpr int PRESSURE_RUNS = 8;       // runs of k_pressure_gauge

struct ClothPressure {   // mirrors mpm_cloth_pressure_t (include/mpm_hip.h)
    uint32_t mode;
    float p, pv, p_ambient, p_max;
};
struct ClothPressureState {   // mirrors mpm_cloth_pressure_state_t
    double volume, energy;
    float gauge;
    uint32_t capped;
};

// acc += (x_b - x_i) x (x_c - x_i), one entry of a row
MPM_PRESSURE_FN void pressure_entry(const float xi[3], const float xb[3], const float xc[3], float acc[3]) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const float b0 = xb[0] - xi[0], b1 = xb[1] - xi[1], b2 = xb[2] - xi[2];
    const float c0 = xc[0] - xi[0], c1 = xc[1] - xi[1], c2 = xc[2] - xi[2];
    const float n0 = b1 * c2 - b2 * c1;
    const float n1 = b2 * c0 - b0 * c2;
    const float n2 = b0 * c1 - b1 * c0;
    acc[0] = acc[0] + n0;
    acc[1] = acc[1] + n1;
    acc[2] = acc[2] + n2;
}
// f = (g / 6) acc: the one multiplication, last
MPM_PRESSURE_FN void pressure_scale(float g, const float acc[3], float f[3]) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
    const float s = g / 6.f;
    f[0] = s * acc[0];
    f[1] = s * acc[1];
    f[2] = s * acc[2];
}
// a whole row: n entries (x_b[3 e ..], x_c[3 e ..]) in stored order
MPM_PRESSURE_FN void pressure_vertex_force(float g, const float x_own[3], size_t n, const float* x_b, const float* x_c, float f[3]) {
    float acc[3] = {0.f, 0.f, 0.f};
    for (size_t e = 0; e < n; ++e) pressure_entry(x_own, x_b + 3 * e, x_c + 3 * e, acc);
    pressure_scale(g, acc, f);
}

// The gauge pressure, energy and cap of one cloth from its volume (double throughout, the gauge rounded to float once)
MPM_PRESSURE_FN ClothPressureState pressure_gauge(const ClothPressure& q, double V) {
    ClothPressureState s;
    s.volume = V;
    s.energy = 0.0;
    s.gauge = 0.f;
    s.capped = 0u;
    if (q.mode == PRESSURE_CONSTANT) {
        s.gauge = q.p;
        s.energy = -((double)q.p * V);
    } else if (q.mode == PRESSURE_GAS) {
        const double pv = (double)q.pv, pa = (double)q.p_ambient, pm = (double)q.p_max;
        const bool free_gas = V > 0.0 && pv / V < pm;
        s.capped = free_gas ? 0u : 1u;
        s.gauge = (float)((free_gas ? pv / V : pm) - pa);
        if (free_gas) s.energy = -pv * log(V) + pa * V;
    }
    return s;
}
// ... of a VENTED cloth (the header, VENTED GAS): the volume is reported, the gauge is +0, the energy 0, no cap
MPM_PRESSURE_FN ClothPressureState pressure_vented(double V) {
    ClothPressureState s;
    s.volume = V;
    s.energy = 0.0;
    s.gauge = 0.f;
    s.capped = 0u;
    return s;
}

}  // namespace mpm

#ifdef __HIPCC__
#include "mpm_step.h"

namespace mpm {

struct PressureArgs {
    const int* row_pid;          // [n_rows] particle id (NfG + vertex) of the row's vertex, ascending
    const unsigned* slice_off;   // [slices + 1] first record of a slice; its width is (next - this) / 64
    const int2* ent;             // records (particle id of b, particle id of c)
    int n_rows;
    const int* row_cloth;              // [n_rows] the row's cloth
    const ClothPressure* par;          // [cloth] the caller's table
    const ClothPressureState* state;   // [cloth] what k_pressure_gauge wrote (read for the cloths in gas mode)
};
struct PressureVolumeArgs {
    const int4* chunks;          // [chunk] (cloth, first face id, end face id, 0): original ids
    double* partial;             // [chunk] sum of x_a . (x_b x x_c)
    const int4* ranges;          // [cloth] (first chunk, end chunk, 0, 0)
    const ClothPressure* par;    // [cloth], or null: no cloth is pressurised
    ClothPressureState* state;   // [cloth]
    int only_gas;                // the substep's launch: the cloths in gas mode alone are written
    uint32_t* vent;              // [chunk] beside `partial`: non-zero where a face of the chunk is torn (written while torn != null)
    const uint8_t* torn;         // [original face id] TearArgs::torn, set per launch (the header, VENTED GAS); nullptr: nothing vents
};

// Row r of the table on the current positions.  Every index into a per-particle array comes through DP::imap from an id
// of the host-built table; a slot that is no vertex slot is reported, never used as an address: the entry then reads the
// row's own position (zero differences: an exact zero).  false: the row's own vertex has no slot.
MPM_DEV bool pressure_row(const DP& p, const PSet& S, const PressureArgs& a, int r, int& s_out, float f[3], bool& bad) {
    const unsigned b0 = a.slice_off[r >> 6], b1 = a.slice_off[(r >> 6) + 1];
    const int width = (int)((b1 - b0) / PRESSURE_SLICE);
    const int own = a.row_pid[r];
    const int s = p.imap[own];
    s_out = s;
    if (s < p.Nf || s >= p.Np) {
        bad = true;
        return false;
    }
    const int cloth = a.row_cloth[r];
    const ClothPressure par = a.par[cloth];
    const float g = par.mode == PRESSURE_GAS ? a.state[cloth].gauge : par.p;
    const float4 x4 = S.q[0][s];
    const float xi[3] = {x4.x, x4.y, x4.z};
    const int2* ent = a.ent + b0 + (r & 63);
    float acc[3] = {0.f, 0.f, 0.f};
    // PRESSURE_BATCH entries at a time: their records, then their slots, then their positions -- three round trips of
    // independent loads per batch (k_bend's lesson, as in link_row).  An entry past the width loads nothing and enters
    // as padding: the row's own slot and position.
    for (int e0 = 0; e0 < width; e0 += PRESSURE_BATCH) {
        int2 q[PRESSURE_BATCH];
        int sb[PRESSURE_BATCH], sc[PRESSURE_BATCH];
        float4 xb[PRESSURE_BATCH], xc[PRESSURE_BATCH];
        // (the width is the slice's, and a slice is one wave: `live` is the same in all 64 lanes, its branches skip)
#pragma unroll
        for (int u = 0; u < PRESSURE_BATCH; ++u) {
            q[u] = make_int2(own, own);
            if (e0 + u < width) q[u] = ent[(size_t)(e0 + u) * PRESSURE_SLICE];
        }
#pragma unroll
        for (int u = 0; u < PRESSURE_BATCH; ++u) {
            sb[u] = s;
            sc[u] = s;
            if (e0 + u < width) {
                // (an id outside the particle numbering cannot index imap either)
                const bool idb = q[u].x >= 0 && q[u].x < p.NpG, idc = q[u].y >= 0 && q[u].y < p.NpG;
                sb[u] = idb ? p.imap[q[u].x] : -1;
                sc[u] = idc ? p.imap[q[u].y] : -1;
            }
        }
#pragma unroll
        for (int u = 0; u < PRESSURE_BATCH; ++u) {
            const bool okb = sb[u] >= p.Nf && sb[u] < p.Np, okc = sc[u] >= p.Nf && sc[u] < p.Np;
            bad |= !(okb && okc);
            xb[u] = x4;
            xc[u] = x4;
            if (e0 + u < width) {
                xb[u] = S.q[0][okb && okc ? sb[u] : s];
                xc[u] = S.q[0][okb && okc ? sc[u] : s];
            }
        }
#pragma unroll
        for (int u = 0; u < PRESSURE_BATCH; ++u) {   // (in stored order)
            const float B[3] = {xb[u].x, xb[u].y, xb[u].z}, Cc[3] = {xc[u].x, xc[u].y, xc[u].z};
            pressure_entry(xi, B, Cc, acc);
        }
    }
    pressure_scale(g, acc, f);
    return true;
}

// Behind k_link (and k_vforce, k_bend, k_bend_damp) on the same stream, with the substep's DP
__global__ __launch_bounds__(256) void k_pressure(DP p, PressureArgs a) {
    if (gated_out(p)) return;
    const int r = (int)(blockIdx.x * 256 + threadIdx.x);
    bool bad = false;
    if (r < a.n_rows) {
        int s;
        float f[3];
        if (pressure_row(p, p.set[p.ctl->cur], a, r, s, f, bad)) {
            p.f[0][s] += f[0];
            p.f[1][s] += f[1];
            p.f[2][s] += f[2];
        }
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(&p.ctl->error, ERR_CAPACITY);
}

// mpm_pressure_forces: out[3 (pid - NfG) ..] = the row's force (vertices without a row stay as the caller left them)
__global__ __launch_bounds__(256) void k_pressure_eval(DP p, PressureArgs a, float* out) {
    const int r = (int)(blockIdx.x * 256 + threadIdx.x);
    bool bad = false;
    if (r < a.n_rows) {
        int s;
        float f[3];
        if (pressure_row(p, p.set[p.ctl->cur], a, r, s, f, bad)) {
            float* o = out + 3 * (size_t)(a.row_pid[r] - p.NfG);
            o[0] = f[0]; o[1] = f[1]; o[2] = f[2];
        }
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(&p.ctl->error, ERR_CAPACITY);
}

// One workgroup per face chunk; lane t takes the ids first + t, first + 256 + t, ... in that order: at most four, as a
// chunk holds at most PRESSURE_CHUNK ids.  Every term x_a . (x_b x x_c) is formed in double from the float positions,
// the corners as measure_face finds them; the four faces' corner ids, then their slots, then their positions go out
// together (three round trips, not twelve).  A face or a corner without a slot is reported and counts as zero.  `base`:
// the first chunk of the launch (the gas cloths' list and the list of all cloths share the arrays).
__global__ __launch_bounds__(256) void k_pressure_volume(DP p, PressureVolumeArgs a, int base) {
#pragma clang fp contract(off)
    static_assert(PRESSURE_CHUNK == 4 * 256, "four ids per lane");
    if (gated_out(p)) return;
    __shared__ double sh[4];
    __shared__ uint32_t shv[4];
    const int k = base + (int)blockIdx.x;
    const int4 ch = a.chunks[k];
    const int cur = p.ctl->cur;
    const PSet& S = p.set[cur];
    bool bad = false;
    bool ok[4];
    int c[4][3], s[4][3];
    float4 x[4][3];
    uint8_t flag[4] = {0, 0, 0, 0};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int id = ch.y + (int)threadIdx.x + 256 * u;
        ok[u] = id < ch.z;
        c[u][0] = c[u][1] = c[u][2] = -1;
        if (!ok[u]) continue;
        // (the face's tear flag, by the same original id and in the same round trip as its corner ids)
        if (a.torn) flag[u] = a.torn[id];
        if (p.idx_orig[0]) {
            c[u][0] = p.idx_orig[0][id]; c[u][1] = p.idx_orig[1][id]; c[u][2] = p.idx_orig[2][id];
        } else {   // (a rank that gave the scene's tables back keeps the corners' ids per slot)
            const int fs = p.imap[id];
            if (fs >= 0 && fs < p.Nf) {
                const int4 g = p.fg[cur][fs];
                c[u][0] = g.x; c[u][1] = g.y; c[u][2] = g.z;
            }
        }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const bool ids = c[u][0] >= p.NfG && c[u][0] < p.NpG && c[u][1] >= p.NfG && c[u][1] < p.NpG && c[u][2] >= p.NfG && c[u][2] < p.NpG;
        bad |= ok[u] && !ids;
        ok[u] = ok[u] && ids;
        s[u][0] = s[u][1] = s[u][2] = -1;
        if (ok[u]) {
            s[u][0] = p.imap[c[u][0]]; s[u][1] = p.imap[c[u][1]]; s[u][2] = p.imap[c[u][2]];
        }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const bool slots = s[u][0] >= p.Nf && s[u][0] < p.Np && s[u][1] >= p.Nf && s[u][1] < p.Np && s[u][2] >= p.Nf && s[u][2] < p.Np;
        bad |= ok[u] && !slots;
        ok[u] = ok[u] && slots;
        x[u][0] = x[u][1] = x[u][2] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok[u]) {
            x[u][0] = S.q[0][s[u][0]]; x[u][1] = S.q[0][s[u][1]]; x[u][2] = S.q[0][s[u][2]];
        }
    }
    double acc = 0.0;
#pragma unroll
    for (int u = 0; u < 4; ++u) {   // (in id order; a face that does not count adds an exact zero)
        const double a0 = (double)x[u][0].x, a1 = (double)x[u][0].y, a2 = (double)x[u][0].z;
        const double b0 = (double)x[u][1].x, b1 = (double)x[u][1].y, b2 = (double)x[u][1].z;
        const double c0 = (double)x[u][2].x, c1 = (double)x[u][2].y, c2 = (double)x[u][2].z;
        acc += (a0 * (b1 * c2 - b2 * c1) + a1 * (b2 * c0 - b0 * c2)) + a2 * (b0 * c1 - b1 * c0);
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) acc += __shfl_xor(acc, off);
    if ((threadIdx.x & 63u) == 0u) sh[threadIdx.x >> 6] = acc;
    // (the chunk's flags, ORed along the sum's path: through the wave, then the four waves through the LDS)
    uint32_t any = 0u;
    if (a.torn) {   // (a kernel argument: the same in every lane)
        any = (uint32_t)(flag[0] | flag[1] | flag[2] | flag[3]);
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) any |= __shfl_xor(any, off);
        if ((threadIdx.x & 63u) == 0u) shv[threadIdx.x >> 6] = any;
    }
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(&p.ctl->error, ERR_CAPACITY);
    __syncthreads();
    if (threadIdx.x == 0u) {
        a.partial[k] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
        if (a.torn) a.vent[k] = ((shv[0] | shv[1]) | shv[2]) | shv[3];
    }
}

// One workgroup (one wave) per cloth: lane r < PRESSURE_RUNS adds its run of the cloth's chunk sums in ascending order,
// lane 0 adds the runs in ascending order, divides by 6 and forms the gauge.
__global__ __launch_bounds__(64) void k_pressure_gauge(DP p, PressureVolumeArgs a) {
    if (gated_out(p)) return;
    __shared__ double sh[PRESSURE_RUNS];
    __shared__ uint32_t shv[PRESSURE_RUNS];
    const int c = (int)blockIdx.x;
    ClothPressure par;
    par.mode = PRESSURE_OFF;
    par.p = par.pv = par.p_ambient = par.p_max = 0.f;
    if (a.par) par = a.par[c];
    if (a.only_gas && par.mode != PRESSURE_GAS) return;   // (the same for the whole workgroup)
    const int4 rg = a.ranges[c];
    const int n = rg.y - rg.x, per = (n + PRESSURE_RUNS - 1) / PRESSURE_RUNS;
    const int run = (int)threadIdx.x;
    if (run < PRESSURE_RUNS) {
        double acc = 0.0;
        const int k1 = min(n, (run + 1) * per);
        for (int k = run * per; k < k1; ++k) acc += a.partial[rg.x + k];
        sh[run] = acc;
        if (a.torn) {   // (the chunks' flags in the same fixed order)
            uint32_t any = 0u;
            for (int k = run * per; k < k1; ++k) any |= a.vent[rg.x + k];
            shv[run] = any;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        double t = sh[0];
        for (int r = 1; r < PRESSURE_RUNS; ++r) t += sh[r];
        uint32_t any = 0u;
        if (a.torn)
            for (int r = 0; r < PRESSURE_RUNS; ++r) any |= shv[r];
        if (any != 0u && par.mode == PRESSURE_GAS) a.state[c] = pressure_vented(t / 6.0);
        else a.state[c] = pressure_gauge(par, t / 6.0);
    }
}

}  // namespace mpm
#endif  // __HIPCC__

namespace mpm {

// ---- host: the closedness check, the rest volume, the table ----------------------------------------------------------
// mpm_mesh_is_closed: every directed edge of the faces (a -> b, b -> c, c -> a) occurs exactly once and its reverse
// exactly once -- a closed, consistently wound 2-manifold mesh in the sense the volume's gradient needs.  false:
// edge[0] -> edge[1] is the first directed edge, in face order, of which that is not true.  The ids must be in
// [0, n_verts) (the caller checks).
inline bool mesh_is_closed(const int32_t* idx, size_t n_faces, int32_t edge[2]) {
    std::vector<uint64_t> keys(3 * n_faces);
    auto key = [](int32_t a, int32_t b) { return (uint64_t)(uint32_t)a << 32 | (uint64_t)(uint32_t)b; };
    for (size_t f = 0; f < n_faces; ++f)
        for (int k = 0; k < 3; ++k) keys[3 * f + k] = key(idx[3 * f + k], idx[3 * f + (k + 1) % 3]);
    std::sort(keys.begin(), keys.end());
    auto count = [&](uint64_t q) {
        const auto r = std::equal_range(keys.begin(), keys.end(), q);
        return (size_t)(r.second - r.first);
    };
    for (size_t f = 0; f < n_faces; ++f)
        for (int k = 0; k < 3; ++k) {
            const int32_t a = idx[3 * f + k], b = idx[3 * f + (k + 1) % 3];
            if (a == b || count(key(a, b)) != 1 || count(key(b, a)) != 1) {
                edge[0] = a;
                edge[1] = b;
                return false;
            }
        }
    return true;
}

// 1/6 sum x_a . (x_b x x_c) over faces [first, first + n) in double from float positions, in face order
inline double mesh_volume(const float* pos, const int* idx, size_t first_face, size_t n_faces) {
    double sum = 0.0;
    for (size_t f = first_face; f < first_face + n_faces; ++f) {
        const float *xa = pos + 3 * (size_t)idx[3 * f], *xb = pos + 3 * (size_t)idx[3 * f + 1], *xc = pos + 3 * (size_t)idx[3 * f + 2];
        const double a0 = xa[0], a1 = xa[1], a2 = xa[2], b0 = xb[0], b1 = xb[1], b2 = xb[2], c0 = xc[0], c1 = xc[1], c2 = xc[2];
        sum += (a0 * (b1 * c2 - b2 * c1) + a1 * (b2 * c0 - b0 * c2)) + a2 * (b0 * c1 - b1 * c0);
    }
    return sum / 6.0;
}

// What mpm_set_pressure refuses before it looks at a mesh; empty: the numbers are fine
inline std::string pressure_refusal(const ClothPressure* t, size_t n) {
    for (size_t c = 0; c < n; ++c) {
        const ClothPressure& q = t[c];
        const std::string at = "pressure: cloth " + std::to_string(c);
        if (!(std::isfinite(q.p) && std::isfinite(q.pv) && std::isfinite(q.p_ambient) && std::isfinite(q.p_max)))
            return at + ": a number is not finite";
        if (q.mode > PRESSURE_GAS) return at + ": unknown mode";
        if (q.mode == PRESSURE_GAS && !(q.pv > 0.f && q.p_ambient >= 0.f && q.p_max > q.p_ambient))
            return at + ": gas mode needs pv > 0, p_ambient >= 0 and p_max > p_ambient";
    }
    return std::string();
}

// The table k_pressure reads, as the host lays it out (no device is touched)
struct PressureRecord {
    uint32_t b, c;   // PressureArgs::ent's int2: the particle ids (nf + vertex) of the face's two other corners
};
struct PressureTable : RowTable<PressureRecord> {
    std::vector<int> row_cloth;   // [row]
};

// cloths: anything with first_vertex, n_verts, first_face, n_faces; h_idx: the faces' vertex ids (0-based over all
// cloths); modes: one ClothPressure per cloth (PRESSURE_OFF: the cloth has no rows); slice: rows per slice
// (PRESSURE_SLICE).  One row per vertex of a pressurised cloth in ascending vertex id (a vertex in no face has an empty
// row), its entries in ascending face id.  false with `why` set: the table does not fit 2^31 records.
template <class Cloth>
inline bool pressure_table(const std::vector<Cloth>& cloths, const int* h_idx, size_t nf, const ClothPressure* modes, size_t slice,
                           PressureTable& out, std::string& why) {
    out = PressureTable{};
    std::vector<size_t> row_vertex, first(1, 0);
    std::vector<PressureRecord> flat;
    for (size_t c = 0; c < cloths.size(); ++c) {
        if (modes[c].mode == PRESSURE_OFF) continue;
        const Cloth& cl = cloths[c];
        // a counting sort of the cloth's corners over its vertices: face order inside a row
        std::vector<size_t> at(cl.n_verts + 1, 0);
        for (size_t f = cl.first_face; f < cl.first_face + cl.n_faces; ++f)
            for (int k = 0; k < 3; ++k) at[(size_t)h_idx[3 * f + k] - cl.first_vertex + 1] += 1;
        for (size_t v = 0; v < cl.n_verts; ++v) at[v + 1] += at[v];
        const size_t base = flat.size();
        flat.resize(base + at[cl.n_verts]);
        std::vector<size_t> fill(at.begin(), at.end() - 1);
        for (size_t f = cl.first_face; f < cl.first_face + cl.n_faces; ++f)
            for (int k = 0; k < 3; ++k) {
                const size_t v = (size_t)h_idx[3 * f + k] - cl.first_vertex;
                flat[base + fill[v]++] = PressureRecord{(uint32_t)(nf + (size_t)h_idx[3 * f + (k + 1) % 3]),
                                                        (uint32_t)(nf + (size_t)h_idx[3 * f + (k + 2) % 3])};
            }
        for (size_t v = 0; v < cl.n_verts; ++v) {
            row_vertex.push_back(cl.first_vertex + v);
            out.row_pid.push_back((int)(nf + cl.first_vertex + v));
            out.row_cloth.push_back((int)c);
            first.push_back(base + at[v + 1]);
        }
    }
    // (padding: the row's own id twice)
    if (!sliced_ell(row_vertex.size(), slice, [&](size_t r) { return first[r + 1] - first[r]; },
                    [&](size_t r, size_t q) { return flat[first[r] + q]; },
                    [&](size_t r) { return PressureRecord{(uint32_t)out.row_pid[r], (uint32_t)out.row_pid[r]}; }, out.slice_off,
                    out.ent)) {
        why = "pressure: the table is too large";
        return false;
    }
    return true;
}

// The chunk list of k_pressure_volume over the cloths with take(c): runs of at most PRESSURE_CHUNK consecutive face ids
// that never straddle a cloth, appended to `chunks`; ranges[c] = (first chunk, end chunk) in `chunks` (empty for the
// others).  The cut of a cloth's faces depends on the cloth alone: the same sums whichever list a cloth is in.
template <class Cloth, class Take, class Int4>
inline void pressure_chunks(const std::vector<Cloth>& cloths, Take take, std::vector<Int4>& chunks, std::vector<Int4>& ranges) {
    ranges.resize(cloths.size());
    for (size_t c = 0; c < cloths.size(); ++c) {
        Int4 rg{};
        rg.x = rg.y = (int)chunks.size();
        rg.z = rg.w = 0;
        if (take(c)) {
            const int first = (int)cloths[c].first_face, end = first + (int)cloths[c].n_faces;
            for (int b = first; b < end; b += PRESSURE_CHUNK) {
                Int4 ch{};
                ch.x = (int)c;
                ch.y = b;
                ch.z = std::min(end, b + PRESSURE_CHUNK);
                ch.w = 0;
                chunks.push_back(ch);
            }
            rg.y = (int)chunks.size();
        }
        ranges[c] = rg;
    }
}

}  // namespace mpm
