// The four kernels of a contact-free substep.
//   k_fem     : CalcFemStateAndForce        (cuda_mpm_kernels.cuh:183-294)
//   k_vforce  : vertex forces as a gather over adjacent faces (replaces the 9
//               float atomics per face of :287-292)
//   k_p2g     : ParticleToGrid              (cuda_mpm_kernels.cuh:418-543)
//   k_grid    : touched-block sum + UpdateGrid (cuda_mpm_kernels.cuh:545-796)
//   k_g2p     : GridToParticle              (cuda_mpm_kernels.cuh:798-924)
#pragma once
#include "mpm_device.h"
#include "mpm_fields.h"
#include "mpm_zone_buffer.h"

namespace mpm {

// ---------------------------------------------------------------------------
// FEM: one thread per face particle (slot order => coalesced face arrays).
// ---------------------------------------------------------------------------
// Gated substeps: the four re-sort launches only precede every few substeps of mpm_run_substeps (they
// cost ~3 us each when idle).  A substep enqueued without them checks here whether a re-sort is pending
// (raised by the G2P of an earlier substep): if so all of its kernels return at once and the host runs
// that substep again, with the re-sort, at its next synchronisation point.
MPM_DEV bool gated_out(const DP& p) {
    return ((p.gated & 1) && p.ctl->need_rebuild) || ((p.gated & 2) && (p.ctl->error & ERR_SLABS)) ||
           ((p.gated & 4) && (int)(p.ctl->watch_hit - p.watch_base) >= 0);
}

// FM: the arithmetic of the divisions and square roots (mpm_math.h: 0 = correctly rounded, the default; 1 = hardware
// approximation + one Newton step, mpm_set_fast_math).  The body is mpm_fem_face.inc.
template <int FM>
__global__ __launch_bounds__(256) void k_fem(DP p, float dt) {
#define MPM_FEM_MATERIAL_SETUP
#define MPM_FEM_M p.M
#define MPM_FEM_VOLW p.dist.on ? S.q[0][i].w : f2.w
#include "mpm_fem_face.inc"
#undef MPM_FEM_MATERIAL_SETUP
#undef MPM_FEM_M
#undef MPM_FEM_VOLW
}

// A cloth's material in a multi-material engine (mpm_add_qr_cloth_with_material): the Lame parameters as mpm_finalize
// forms the engine's, and rho, by which the FEM turns the face's volume into the mass its q[0].w holds.
struct ClothMat {
    float mu, lambda, gamma, K, cF, rho, pad0, pad1;
};
// the cloth of a face rides above the corners' ranks in fq[3].x (bits 0-11: DP::VF)
constexpr int FACE_CLOTH_SHIFT = 12;
// the engine's material with the per-cloth fields of the face's cloth
MPM_DEV Material cloth_material(const Material& engine, const ClothMat* mats, const float4& f3) {
    const ClothMat t = mats[(unsigned)__float_as_int(f3.x) >> FACE_CLOTH_SHIFT];
    Material m = engine;
    m.mu = t.mu; m.lambda = t.lambda; m.gamma = t.gamma; m.K = t.K; m.cF = t.cF; m.density = t.rho;
    return m;
}

// k_fem for a multi-material engine, launched instead of it with the same geometry: the face's material comes from its
// cloth's entry of `mats`, and the face particle's q[0].w becomes its mass, volume x rho -- the float a single-material
// engine with this density forms in ParticleToGrid.  (A multi-material engine is never partitioned.)
template <int FM>
__global__ __launch_bounds__(256) void k_fem_mat(DP p, float dt, const ClothMat* mats) {
#define MPM_FEM_MATERIAL_SETUP const Material M = cloth_material(p.M, mats, f3);
#define MPM_FEM_M M
#define MPM_FEM_VOLW f2.w * M.density
#include "mpm_fem_face.inc"
#undef MPM_FEM_MATERIAL_SETUP
#undef MPM_FEM_M
#undef MPM_FEM_VOLW
}

// the force on vertex k from its entries of DP::VF; false = they say "walk the CSR" (nothing usable summed)
// PLANES: how many of the eight planes of a chunk are read -- VF_PLANES_ALL, or VF_PLANES_REGULAR for an engine whose
// meshes have no vertex with more faces than that (vf_planes_of: the planes left out hold +0, and the sum below ends
// with `+= -0` for each of them, which changes no bit of it -- not even the sign of a zero sum, (+-0) + (-0) = +-0).
// Such an engine has no marked vertex either.
template <int PLANES>
MPM_DEV bool vertex_force_vf(const DP& p, int k, float& f0, float& f1, float& f2) {
    static_assert(PLANES == VF_PLANES_REGULAR || PLANES == VF_PLANES_ALL, "the two instances the launches choose between");
    // (one address for all the loads: the planes of a chunk are 384 bytes apart, an immediate offset)
    const float* e0 = p.VF + vf_entry((unsigned)k, 0) * 3;
    float3 g[PLANES];
#pragma unroll
    for (int j = 0; j < PLANES; ++j) g[j] = *reinterpret_cast<const float3*>(e0 + (size_t)j * VF_CHUNK * 3);
    f0 = f1 = f2 = 0.f;
#pragma unroll
    for (int j = 0; j < PLANES; ++j) {   // (ascending original face id, as vertex_force_from; an empty entry adds -0)
        f0 += -g[j].x;
        f1 += -g[j].y;
        f2 += -g[j].z;
    }
    return PLANES < VF_PLANES_ALL || __float_as_uint(g[0].x) != VF_MARK;
}

// more than 8 faces around vertex k: walk the original adjacency (the triples of these faces' corners are in G3)
MPM_DEV void vertex_force_csr(const DP& p, const PSet& S, int k, float& f0, float& f1, float& f2) {
    const int s = p.Nf + k;
    f0 = f1 = f2 = 0.f;
    const int vo = S.pid[s] - p.NfG;
    for (int e = p.adj_off[vo]; e < p.adj_off[vo + 1]; ++e) {
        const int fc = p.adj_fc[e];
        const int fs = p.imap[fc >> 2];
        const float3 g = fs >= 0 ? p.G3[(size_t)fs * 3 + (fc & 3)]
                                 : make_float3(S.q[0][s].w > 0.f ? __int_as_float(0x7FC00000) : 0.f, 0.f, 0.f);
        f0 += -g.x;
        f1 += -g.y;
        f2 += -g.z;
    }
}

// Vertex force = - sum over adjacent (face, corner) of that corner's force triple, summed in ascending original face
// id (the order sequential atomics would produce): the vertex's row of DP::VF, or the adjacency CSR for a vertex with
// more than eight faces.
template <int PLANES>
MPM_DEV void vertex_force_value(const DP& p, const PSet& S, int k, float& f0, float& f1, float& f2) {
    if (!vertex_force_vf<PLANES>(p, k, f0, f1, f2)) vertex_force_csr(p, S, k, f0, f1, f2);
}
template <int PLANES>
MPM_DEV void vertex_force(const DP& p, const PSet& S, int k) {   // ... written to p.f
    float f0, f1, f2;
    vertex_force_value<PLANES>(p, S, k, f0, f1, f2);
    const int s = p.Nf + k;
    p.f[0][s] = f0;
    p.f[1][s] = f1;
    p.f[2][s] = f2;
}

// (the phase-by-phase API and the partitioned-domain chains; mpm_run_substeps lets k_p2g do this per work
// item, see k_p2g's FORCES).  PLANES: see vertex_force_vf; launch_fem_vertices picks the instance.
template <int PLANES>
__global__ __launch_bounds__(256) void k_vforce(DP p) {
    if (gated_out(p)) return;
    const unsigned nva = (unsigned)p.ctl->nva;
    const unsigned chunk = xcd_chunk_active(blockIdx.x, nva);
    const int k = (int)(chunk * 256 + threadIdx.x);
    if (chunk == 0xFFFFFFFFu || k >= (int)nva) return;
    vertex_force<PLANES>(p, p.set[p.ctl->cur], k);
}

// ---------------------------------------------------------------------------
// P2G
//
// One workgroup per work item (a home block, or a run of the wave groups of a
// heavy one) accumulates the block's (TILE_W)^3 node tile in LDS and stores it
// as a slab.  Inside the item the transfer is organised per
// base cell: all particles that share a base cell scatter to the same 27 nodes,
//     node(n) += sum_p w_n(p) * (m_p, q_p + Bdx_p * (i,j,k)_n)
// which is a small dense contraction over the cell's P particles: 16 staged columns per particle (3 x (momentum
// term, 3 affine terms), mass) against 27 weights.  It runs on the f32 matrix pipe (v_mfma_f32_16x16x4_f32: exact f32
// FMA chains, the VALU rate, but the sum over particles needs no cross-lane shuffles and no per-particle LDS atomics).
// Every wave works on its own 64-particle groups, without workgroup barriers:
//   1. every lane loads one particle (four 16-byte records), finds its base cell in the tile and builds its columns,
//   2. the wave groups its 64 particles by base cell (ballot loop, ranks by v_mbcnt) and stages
//      them in a wave-private LDS area, with the products px[i] * py[j] of their B-spline factors,
//   3. per cell: 4 particles per MFMA step, 2 MFMAs per step (nodes 0-14 and 15-26).  Since round 6 the staged
//      columns are the A operand and the weights the B operand: a lane's four accumulator registers
//      are then the four TERMS (1, i, j, k) of one (node, component), folded in the lane with a product, two
//      fused multiply-adds and a sum (one product more in fixed point) -- rounds 1-5 had nodes as rows and folded
//      across a quad with DPP -- and added to the tile: 2 LDS atomics (64 distinct words each) per cell, doubles or
//      64-bit fixed point (EXACT).
// Replaces the warp-segmented scatter of cuda_mpm_kernels.cuh:418-543; the
// order of particles inside a block is irrelevant.
// ---------------------------------------------------------------------------
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// staged floats per particle (one row of 23): the 13 columns of Y that carry numbers, the nine products px[i] * py[j]
// of the particle's B-spline factors (index 3 i + j) and fz.  Y[0..7] sit in floats 0..7, the products in 8..16, fz in
// 17 and Y[8..12] in 18..22: the Y windows of two consecutive rows then fall on disjoint halves of the 32 banks of
// ds_read_b32 (rows of 23 floats with Y in 0..12 would overlap in four banks).  67 rows per wave: 64 particles and the
// three rows past them that a step starting at row 61..63 reads (and masks).
constexpr int STG = 23, STG_PXY = 8, STG_FZ = 17, STG_ROWS = 67;
MPM_DEV int stg_col(int c) { return c < 8 ? c : c + 10; }   // float of Y[c] in a row

// LDS accumulation is done in 64-bit fixed point: on gfx950 a wave-wide ds_add_f32
// costs ~190 LDS cycles per instruction (measured, scratch/lds_atomic_bench.hip)
// against ~10 for ds_add_u64, and integer sums are exact and order independent.
// float -> Q-format int64 with single-precision instructions only: q = v * scale is exact (power
// of two); |q| = hi * 2^32 + lo with hi = floor(|q| / 2^32) and lo = |q| - hi * 2^32 in [0, 2^32),
// both exact because they are parts of the same 24-bit mantissa (doing this on the SIGNED value
// would form 2^32 - |q| for small negative q, which does not fit a float: +-128 quanta of noise).
// Below 2^24 quanta q has fractional bits: they are rounded to nearest even, so the conversion is
// unbiased whatever the particle count.  `worst` collects the bit pattern of the largest |q| (NaN and
// infinity have the largest patterns of all): the caller compares it with 2^62 once, at the end -- a
// boolean per call lives in a scalar register pair and costs scalar instructions in every loop.
MPM_DEV void lds_add_fixed(long long* a, float q, unsigned& worst) {   // q = value * scale
    const float aq = fabsf(q);
    const float h = floorf(aq * 0x1p-32f);
    const unsigned lo = (unsigned)rintf(fmaf(-h, 0x1p32f, aq));
    const unsigned long long mag = ((unsigned long long)(unsigned)h << 32) | lo;
    const unsigned long long fx = q < 0.f ? 0ull - mag : mag;
    __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(a), fx, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_WORKGROUP);
    worst = max(worst, __float_as_uint(aq));
}

// coefficients (c0 + c1 f + c2 f^2) of the quadratic B-spline weight of stencil offset a
MPM_DEV void bspline_coeff(int a, bool on, float& c0, float& c1, float& c2) {
    c0 = a == 0 ? 1.125f : (a == 1 ? -.25f : .125f);
    c1 = a == 0 ? -1.5f : (a == 1 ? 2.f : -.5f);
    c2 = a == 1 ? -1.f : .5f;
    if (!on) c0 = c1 = c2 = 0.f;
}

struct Stencil {
    int rx, ry, rz;      // base cell relative to the tile origin (block origin - FREE_ZONE)
    float fx[3];
    float wx[3], wy[3], wz[3];
    unsigned out_bits;   // rx | ry | rz before the clamp: > TILE_W - 3 when the base cell is outside the tile (MPM_ERR_DRIFT)
};

MPM_DEV Stencil make_stencil(const DP& p, float x, float y, float z, int ox, int oy, int oz) {
    Stencil s;
    const uint32_t hi = (uint32_t)((1 << p.bits) - 3);
    const uint32_t bx = min(base_cell(x, p.dxinv), hi), by = min(base_cell(y, p.dxinv), hi),
                   bz = min(base_cell(z, p.dxinv), hi);
    s.fx[0] = x * p.dxinv - (float)bx;
    s.fx[1] = y * p.dxinv - (float)by;
    s.fx[2] = z * p.dxinv - (float)bz;
    bspline3(s.fx[0], s.wx);
    bspline3(s.fx[1], s.wy);
    bspline3(s.fx[2], s.wz);
    int rx = (int)bx - ox, ry = (int)by - oy, rz = (int)bz - oz;
    const int hi_h = TILE_W - 3;
    static_assert(((TILE_W - 3) & (TILE_W - 2)) == 0, "rx | ry | rz <= hi_h is only equivalent to all three in range for hi_h = 2^k - 1");
    s.out_bits = (unsigned)(rx | ry | rz);   // (a negative coordinate sets the high bits)
    rx = min(max(rx, 0), hi_h);
    ry = min(max(ry, 0), hi_h);
    rz = min(max(rz, 0), hi_h);
    s.rx = rx; s.ry = ry; s.rz = rz;
    return s;
}

// neighbour blocks (27-bit set) reached by the 3^3 stencil of base cell (rx, ry, rz) of a tile
// (an outer product of three 3-bit sets, formed with shifts and masks; k_p2g tabulates it per lane at its start)
MPM_DEV unsigned tile_reach_mask(int rx, int ry, int rz) {
    // Per axis the stencil of base cell r in 0..7 (tile coordinates, block origin at FREE_ZONE = 2) reaches the
    // block offsets {-1,0}, {0}, {0,+1}, {+1} for r >> 1 = 0, 1, 2, 3: as 3-bit sets 3, 2, 6, 4.
    static_assert(FREE_ZONE == 2, "the packed tables below are for a free zone of 2 cells");
    const int ix = rx >> 1, iy = ry >> 1, iz = rz >> 1;
    // bit (a * 9 + b * 3 + c) = mx[a] & my[b] & mz[c].  z set replicated at bits 0, 3, 6 and y set spread over
    // bits 3b..3b+2, both 9 bits per table entry:
    const unsigned long long Z = 0x926D924DBull, Y = 0xE07E0703Full;
    const unsigned m9 = (unsigned)((Z >> (9 * iz)) & (Y >> (9 * iy))) & 0x1FFu;
    const unsigned rep = m9 * 0x40201u;                       // m9 at bits 0, 9, 18
    const int lo = (ix + 1) >> 1, hi = (ix >> 1) + 1;         // x offsets lo..hi
    const unsigned xexp = ((1u << (9 * (hi + 1))) - 1u) ^ ((1u << (9 * lo)) - 1u);
    return rep & xexp;
}

constexpr int P2G_WAVES = 8, P2G_THREADS = 64 * P2G_WAVES;
// two workgroups per CU: 8 waves each at <= 128 VGPRs (4 per SIMD)
// FORCES: where a vertex lane finds the internal force on its vertex.
//   0  in p.f (k_vforce ran before this kernel: the phase-by-phase API, meshes with a vertex of more than eight faces)
//   1  in the planes of DP::VF (PLANES of the eight), summed here (one round trip of coalesced loads; a partitioned
//      domain went through per-slot adjacency records and G3 until round 5: two dependent round trips, eight gathers)
// 1 saves the k_vforce launch of every substep.  Rounds 2-3 computed the forces of ALL vertices of an item in a
// prologue of their own (two dependent round trips and a barrier that every workgroup of the launch walks through at
// the same time: ~6 us in which nothing else happens); now each vertex lane fetches them with its particle records:
// k_p2g 48.9 -> 45.3 us (event time, same box), -> 43.9 with the group descriptor a group ahead, -> 41 with the vertex-side records (DP::VF).
// EXACT: how the node sums of a work item are accumulated in its LDS tile.
//   1  64-bit fixed point (lds_add_fixed): integer sums, exact, independent of the order in which the waves' atomics
//      arrive -- what makes a trajectory reproducible to the bit in deterministic mode (mpm_set_deterministic), at 13
//      vector instructions per value and cell for the conversion (a third of the per-cell epilogue);
//   0  double precision (ds_add_f64: native on gfx950, 17-21 cycles per wave instruction, scratch/lds_atomic_bench.hip --
//      ds_add_f32 is the one that takes 194): one conversion instruction per value.  The sum of the <= ~100 float
//      contributions to a node is exact in double, hence independent of the order, as long as they span less than 2^29
//      in magnitude; beyond that its LAST bit (2^-53 of the sum, rounded to float afterwards) may depend on the order.
//      The default: without the canonical particle order of deterministic mode the order INSIDE a cell already
//      differs from run to run at float level.
// one step of the per-cell contraction: rows = the 16 columns of the staged particles (A operand), columns = 16 node
// rows (B operand); the transposed form of round 6, see point 3 above and DESIGN.md section 3.2
MPM_DEV f32x4 p2g_mfma(float y, float w, f32x4 acc) { return __builtin_amdgcn_mfma_f32_16x16x4f32(y, w, acc, 0, 0, 0); }
// FIELDS: 1 = the engine has a table of external force fields (mpm_set_force_fields, mpm_fields.h): every particle's
// acceleration a(x, v) is evaluated where its staged momentum column is formed and enters it as m (a dt) -- no pass of
// its own over the particles, every record it needs is in the lane's registers.  The table's pointer is the one
// argument of the pack TABLE (= ForceFieldTable), which only these instances have: the FIELDS = 0 instances keep their
// arguments and their code (launch_p2g picks the instance).  __restrict__: the table is read-only to the kernel, its
// loads are scalar.
MPM_DEV const ForceFieldTable* p2g_field_table(const ForceFieldTable* t) { return t; }
// PLANES: the planes of DP::VF a vertex lane reads (FORCES = 1; see vertex_force_vf): launch_p2g picks the instance from
// the engine's largest valence, next to EXACT and FIELDS -- a runtime count had cost more in scalar branches around the
// loads than the loads themselves (DESIGN_HISTORY.md section 8, round 4).
template <int FORCES, int EXACT, int FIELDS = 0, int PLANES = VF_PLANES_ALL, typename... TABLE>
__global__ __launch_bounds__(P2G_THREADS) __attribute__((amdgpu_waves_per_eu(P2G_WAVES / 2, P2G_WAVES / 2))) void k_p2g(DP p, float dt, const TABLE* __restrict__... table) {
    static_assert(sizeof...(TABLE) == FIELDS, "the table is the argument of the FIELDS = 1 instances only");
    if (gated_out(p)) return;
    // chain substep: the entry counters of the halo send buffers, which the k_grid<0> behind this kernel fills
    if (blockIdx.x == 0 && threadIdx.x < 2 && p.halo_hdr[threadIdx.x]) p.halo_hdr[threadIdx.x][0] = 0u;
    __shared__ long long tile[TILE_N * 4];  // (mvx, mvy, mvz, m) per node: fixed point, or the bits of doubles (EXACT)
    // wave-private staging: 64 particles (+3 slack rows touched by the operand reads)
    __shared__ __attribute__((aligned(16))) float stage_all[P2G_WAVES][STG_ROWS * STG];
    __shared__ unsigned s_mask;
    static_assert(sizeof(long long) * TILE_N * 4 + sizeof(float) * P2G_WAVES * STG_ROWS * STG + 4 <= 81920,
                  "two workgroups per CU need <= 80 KB of LDS each");
    Ctl* ctl = p.ctl;
    const PSet& S = p.set[ctl->cur];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const float gdt = p.M.gravity * dt;
    const float sdt = -dt * p.Dinv;
    float* stage = stage_all[wv];

    // ---- lane constants of the contraction ---------------------------------
    // Node n = 9 i + 3 j + k = 3 a + k with a = 3 i + j.  B-operand column j16 of MFMA 0 is node j16 (lanes 0..14), of
    // MFMA 1 node j16 + 12 (lanes 3..14): both share k = j16 % 3 and their pairs (i, j) are a0 = j16 / 3 and a0 + 4, so
    // a lane reads its two staged products px * py with one ds_read2_b32 (floats a0 and a0 + 4 of the row's nine) and
    // multiplies both by the same pz.  The other slots (MFMA 0 lane 15, MFMA 1 lanes 0..2 and 15) carry no node: their
    // weights are whatever finite floats of the row the same reads return, and their columns of the result are dropped.
    const int j16 = lane & 15, g4 = lane >> 4;
    const int node[2] = {j16 < 15 ? j16 : -1, j16 >= 3 && j16 < 15 ? j16 + 12 : -1};
    float cz0, cz1, cz2;   // pz: the weight polynomial of k = j16 % 3
    bspline_coeff(j16 % 3, true, cz0, cz1, cz2);
    const int ycol = j16 < 13 ? stg_col(j16) : 0;    // A operand: Y[j16] (rows 13..15 of the product are dropped)
    const int xycol = STG_PXY + j16 / 3;              // px * py of (a0) and, 4 floats on, of (a0 + 4)
    // epilogue: (1, i, j, k)[r] of this lane's node of MFMA t, times the fixed-point scale of this lane's component g4 (a
    // power of two: scaling before or after the sums gives the same bits)
    float fac[2][4];
    int delta[2];        // float offset of this lane's node/component in the tile, -1 if none
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        // lane (j16, g4) of MFMA t ends up with the four terms of node[t], component g4
        const int n = node[t];
        const int ni = n / 9, nj = (n / 3) % 3, nk = n % 3;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            fac[t][r] = n < 0 ? 0.f : (r == 0 ? 1.f : (float)(r == 1 ? ni : (r == 2 ? nj : nk)));
            if (g4 == 3 && r != 0) fac[t][r] = 0.f;   // (A rows 13..15: lanes 13..15 read Y[0] in their place)
        }
        delta[t] = n >= 0 ? ((ni * TILE_W + nj) * TILE_W + nk) * 4 + g4 : -1;
    }
    {
        const float fscale = EXACT ? (float)(g4 == 3 ? p.fix_m : p.fix_p) : 1.f;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) fac[t][r] *= fscale;
    }
    // lane l = (ix, iy, iz) in 2-bit fields: the neighbour blocks reached from base cells (2 ix.., 2 iy.., 2 iz..) of the tile
    const unsigned reach_of_lane = tile_reach_mask(2 * (lane >> 4), 2 * ((lane >> 2) & 3), 2 * (lane & 3));
    // A step reads 4 staged rows; rows that do not belong to the cell (the next cell's particles,
    // rows never written) are masked in the B operand only, so every row must hold finite numbers
    for (int k = lane; k < STG_ROWS * STG; k += 64) stage[k] = 0.f;

    // Work items (a home block, or a run of the wave groups of a heavy one) are taken round-robin
    // from the heaviest-first order: workgroup w processes entries w, w + G, ...; with G resident
    // workgroups that is one heavy item each plus the light tail, and it needs neither a queue
    // atomic nor extra barriers per item.
    const unsigned n_items = ctl->n_items;
    for (unsigned q = blockIdx.x; q < n_items; q += gridDim.x) {
        __syncthreads();  // the previous item's slab has been written
        const int4 fa = p.item_flat[2 * q], fb = p.item_flat[2 * q + 1];
        const unsigned item = (unsigned)fa.x;
        const unsigned long long tb0 = (diag_flags(p) & 4) ? __builtin_readcyclecounter() : 0ull;
        for (int n = tid; n < TILE_N * 4; n += P2G_THREADS) tile[n] = 0;
        if (tid == 0) s_mask = 0;
        int bx, by, bz;
        block_coords((uint32_t)fa.z, bx, by, bz);
        const int ox = bx * 4 - FREE_ZONE, oy = by * 4 - FREE_ZONE, oz = bz * 4 - FREE_ZONE;
        const int4 rg = make_int4(fb.x, fb.y, fb.z, 0);
        const int nfb = rg.y - rg.x;
        // Every wave streams through its own groups of <= 64 particles; no workgroup barrier inside.
        // Groups are runs of whole cells (faces and vertices of the same cells together), laid out
        // at the last rebuild: a group usually spans two base cells.
        const int ngroups = fa.w;
        const int4* groups = p.home_groups + fb.w;
        struct Raw {
            float x[3], v[3], vol, C[9];
            // tau factors a, b (faces) and force (vertices) in separate registers: merging them
            // into one array makes the compiler route the prefetch through scratch memory
            float ta[3], tb[3], frc[3];
            bool act, is_face;
        };
        // the force on a vertex particle from k_vforce's p.f
        auto force_of = [&](unsigned ii, float* f) {
            const float* fbase = p.f[0] + ii;
#pragma unroll
            for (int d = 0; d < 3; ++d) f[d] = fbase[(size_t)d * p.f_stride];
        };
        // a group's descriptor is fetched one group ahead of its records: no dependent round trip in front of the record
        // loads (45.3 -> 43.9 us once the vertex forces came with the records; DESIGN_HISTORY.md section 3.2)
        auto desc_of = [&](int g) { return groups[min(g, ngroups - 1)]; };
        int4 gd_next = make_int4(0, 0, 0, 0);
        auto load_raw = [&](int4 gr) {
            Raw r;
            const int gf = gr.y - gr.x, gn = gf + (gr.w - gr.z);
            r.act = lane < gn;
            r.is_face = lane < gf;
            // unsigned index: lets the loads use the scalar-base + 32-bit-offset addressing form
            const unsigned any_slot = (unsigned)(nfb ? rg.x : rg.z);   // (a particle of the item: always valid)
            const unsigned ii = r.act ? (unsigned)(r.is_face ? gr.x + lane : gr.z + (lane - gf)) : any_slot;
            // (one base pointer and a stride for the four planes: see DP::q_stride)
            const float4* qb = S.q[0] + ii;
            const float4 q0 = qb[0], q1 = qb[p.q_stride], q2 = qb[2 * (size_t)p.q_stride], q3 = qb[3 * (size_t)p.q_stride];
            r.x[0] = q0.x; r.x[1] = q0.y; r.x[2] = q0.z; r.vol = q0.w;
            r.v[0] = q1.x; r.v[1] = q1.y; r.v[2] = q1.z;
            unpack_C(q1, q2, q3, r.C);
            // Face lanes need the tau factors, vertex lanes the force.  Both are loaded by ALL lanes, from a
            // valid slot of the other kind where the lane has no use for them (one cache line for the wave), instead
            // of `if (face) load ab else load f` over zero-filled registers: the fill of registers that the other
            // lanes' loads are still writing made the compiler put `s_waitcnt vmcnt` in front of it, i.e. the wave
            // waited for its whole prefetch (a memory round trip per group) before starting the contraction.
            {
                const unsigned fi = r.is_face ? ii : (unsigned)(nfb ? rg.x : 0), vi = r.is_face ? any_slot : ii;
                const float3 a = p.ta[fi];
                const float3 b = *reinterpret_cast<const float3*>(&S.fq[0][fi]);   // F[:,2], see pack_F
                r.ta[0] = a.x; r.ta[1] = a.y; r.ta[2] = a.z; r.tb[0] = b.x; r.tb[1] = b.y; r.tb[2] = b.z;
                const bool vert = r.act && !r.is_face;
                if (FORCES == 1) {
                    vertex_force_vf<PLANES>(p, vert ? (int)ii - p.Nf : 0, r.frc[0], r.frc[1], r.frc[2]);   // (vertex 0 for the other lanes: valid memory)
                } else {
                    force_of(vi, r.frc);
                }
                // (p.f is what a caller downloads as the forces: between the substeps of one batch nobody can)
                if (FORCES != 0 && vert && !p.lean_g2p) {
                    p.f[0][ii] = r.frc[0]; p.f[1][ii] = r.frc[1]; p.f[2][ii] = r.frc[2];
                }
            }
            return r;
        };
        Raw cur;
        __syncthreads();
        unsigned mymask = 0;
        bool halo_bad = false;
        unsigned out_worst = 0, fix_worst = 0;   // error conditions, collected as integers in vector registers
        if (wv < ngroups) gd_next = desc_of(wv);
        const bool prof = (diag_flags(p) & 4) != 0 && wv == 0;
        unsigned long long tq[3] = {0, 0, 0}, pc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (prof && lane == 0) atomicAdd(&p.dbgbuf[14], (unsigned long long)__builtin_readcyclecounter() - tb0);   // prologue
        for (int g = wv; g < ngroups; g += P2G_WAVES) {
            // ---- 1. one particle per lane ---------------------------------------
            // (a group's records are loaded when its turn comes: fetched a group ahead, as in rounds 1-3, they held 25
            // registers through the contraction, 128 VGPRs + scratch, and cost more than the wait)
            if (prof) tq[0] = __builtin_readcyclecounter();
            cur = load_raw(gd_next);
            gd_next = desc_of(g + P2G_WAVES);
            const bool act = cur.act, is_face = cur.is_face;
            const Stencil st = make_stencil(p, cur.x[0], cur.x[1], cur.x[2], ox, oy, oz);
            // partitioned domain: a ghost copy (vol < 0) scatters nothing, its owner does
            const bool own = cur.vol > 0.f;
            const float m = own ? cur.vol * p.M.density : 0.f;
            float Y[16];
            {
                float B[9];
                float fext[3] = {0.f, 0.f, 0.f};
                // (explicit fused multiply-adds where a sum of products could be fused in more than one way: left to the
                // compiler, the choice -- and the last bit of the result -- changes from build to build with the code around it)
#pragma unroll
                for (int r = 0; r < 9; ++r) B[r] = cur.C[r] * m;
                if (is_face) {
#pragma unroll
                    for (int r = 0; r < 3; ++r)
#pragma unroll
                        for (int c = 0; c < 3; ++c) B[r * 3 + c] = fmaf(sdt, cur.ta[r] * cur.tb[c], B[r * 3 + c]);
                } else {
#pragma unroll
                    for (int r = 0; r < 3; ++r) fext[r] = cur.frc[r] * dt;
                }
                if constexpr (FIELDS != 0) {
                    // (uniform loads: every lane reads the same entries of the table)
                    const ForceFieldTable* ft = p2g_field_table(table...);
                    float a[3];
                    force_field_acceleration(ft->f, ft->n, cur.x, cur.v, cur.tb, is_face, a);
#pragma unroll
                    for (int r = 0; r < 3; ++r) fext[r] = fmaf(m, a[r] * dt, fext[r]);
                }
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    // (both forms and a select: one fma with the addend -0 off the gravity axis gives the same bits in three
                    // vector instructions fewer per group and measured no faster)
                    float qq = r == p.M.gravity_axis ? fmaf(cur.v[r], m, m * gdt) : cur.v[r] * m;
                    qq += fext[r];
                    const float dot = fmaf(B[r * 3 + 2], st.fx[2], fmaf(B[r * 3], st.fx[0], B[r * 3 + 1] * st.fx[1]));
                    qq = fmaf(-p.dx, dot, qq);
                    Y[r * 4 + 0] = qq;
                    Y[r * 4 + 1] = B[r * 3 + 0] * p.dx;
                    Y[r * 4 + 2] = B[r * 3 + 1] * p.dx;
                    Y[r * 4 + 3] = B[r * 3 + 2] * p.dx;
                }
                Y[12] = m; Y[13] = 0.f; Y[14] = 0.f; Y[15] = 0.f;
                if (p.dist.on && !own) {   // (only a partitioned domain has ghost copies: a scalar branch otherwise)
#pragma unroll
                    for (int k = 0; k < 12; ++k) Y[k] = 0.f;
                }
            }
            out_worst = max(out_worst, act ? st.out_bits : 0u);
            if (p.dist.on && act && own) {
                // the stencil of an owned particle must stay inside the blocks the neighbour receives
                const int gx = ox + st.rx;
                halo_bad |= gx < p.dist.own_lo - p.dist.zone_cells || gx + 2 >= p.dist.own_hi + p.dist.zone_cells;
            }
            if (diag_flags(p) & 2) {
                float acc = 0.f;
#pragma unroll
                for (int k = 0; k < 16; ++k) acc += Y[k];
                if (acc == 1.2345e30f) tile[0] = (long long)acc;
                continue;
            }
            // ---- 2. group the wave's particles by base cell ---------------------
            const int key = (st.rx * 8 + st.ry) * 8 + st.rz;
            const unsigned long long actmask = __ballot(act);
            int pos = 0;
            {
                unsigned long long todo = actmask;
                int base = 0;
                while (todo) {
                    const int lk = __builtin_amdgcn_readlane(key, __builtin_ctzll(todo));
                    const bool mine = key == lk;
                    const unsigned long long same = __ballot(mine) & todo;
                    // (an active lane whose key is lk is in `same`: a key leaves `todo` with all of its lanes at once; the
                    // position of an inactive lane is never used.  Rank inside the run: v_mbcnt counts the bits below the
                    // lane and adds the run's base in the same two instructions)
                    const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(same >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)same, (unsigned)base));
                    if (mine) pos = rank;
                    base += (int)__popcll(same);
                    todo &= ~same;
                }
            }
            // ---- 3. stage at the grouped position (wave-private LDS, in-order) --
            if (act) {
                // the B-spline factors once per particle, each as fma(fma(c2, f, c1), f, c0) with bspline_coeff's
                // coefficients; the contraction forms the weight of node (i, j, k) as (px[i] * py[j]) * pz[k]
                float px[3], py[3];
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    float c0, c1, c2;
                    bspline_coeff(a, true, c0, c1, c2);
                    px[a] = fmaf(fmaf(c2, st.fx[0], c1), st.fx[0], c0);
                    py[a] = fmaf(fmaf(c2, st.fx[1], c1), st.fx[1], c0);
                }
                float* sp = stage + pos * STG;
#pragma unroll
                for (int c = 0; c < 13; ++c) sp[stg_col(c)] = Y[c];
#pragma unroll
                for (int a = 0; a < 9; ++a) sp[STG_PXY + a] = px[a / 3] * py[a % 3];
                sp[STG_FZ] = st.fx[2];
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            if (diag_flags(p) & 1) continue;
            // ---- 4. per-cell contraction on the matrix pipe ----------------------
            unsigned long long todo = actmask;
            int s0 = 0;
            // operands of the next step: Y[j16], the two products px * py and fz of row (step + g4)
            float ny, nfz;
            f32x2 nxy;
            // ... read from the cell's first row + `off` (this lane's three addresses, set once per cell)
            const float *ry, *rxy, *rz;
            auto load_ops = [&](int off) {
                ny = ry[off]; nxy = f32x2{rxy[off], rxy[off + 4]}; nfz = rz[off];
            };
            auto cell_rows = [&](int s) {   // the next cell starts at row s
                const float* row = stage + (s + g4) * STG;
                ry = row + ycol; rxy = row + xycol; rz = row + STG_FZ;
                load_ops(0);
            };
            cell_rows(0);
            if (prof) tq[1] = __builtin_readcyclecounter();
            __builtin_amdgcn_s_setprio(2);   // (waves in the contraction keep the matrix pipe fed: ahead of waves that derive / group)
            while (todo) {
                const int ckey = __builtin_amdgcn_readlane(key, __builtin_ctzll(todo));
                const unsigned long long same = __ballot(key == ckey) & todo;
                todo &= ~same;
                // (two 32-bit counts: compared as one 64-bit count, the step tests below become vector instructions)
                const int s1 = s0 + __builtin_popcount((unsigned)same) + __builtin_popcount((unsigned)(same >> 32));
                const int nsteps = (s1 - s0 + 3) >> 2;   // (a cell has 1..64 particles: 1..16 steps)
                f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
                if (prof) { pc[4] += 1; pc[5] += (unsigned)nsteps; tq[2] = __builtin_readcyclecounter(); }
                // Operands of a step are fetched one step ahead (the first step's during the previous cell's epilogue), so
                // the LDS latency hides behind the MFMAs.  Three kinds of step: the first accumulates onto the inline
                // constant 0 (no eight moves to clear the accumulators of every cell), only the last one has rows of the
                // NEXT cell to mask (a cell's rows are contiguous: every row of an earlier step is the cell's own).
                // Per step: pz (two fused multiply-adds), both weights (one v_pk_mul_f32), two MFMAs.  The middle steps are
                // written out (<= 14 of them, each with a scalar exit to the shared last step): their operand reads take
                // the row offset from the cell's first row as an immediate, instead of advancing three lane addresses per
                // step.  (A `for` with a break is re-rolled into such a loop; with a guard per step, leaving walks the
                // remaining guards.)
                auto step = [&](int k, bool first_step, bool last_step) {   // k: step of the cell
                    const float pz = fmaf(fmaf(cz2, nfz, cz1), nfz, cz0);
                    const f32x2 w01 = nxy * f32x2{pz, pz};
                    float y = ny;
                    if (last_step && !(g4 < s1 - s0 - 4 * k)) y = 0.f;   // (weights of foreign rows are finite: 0 * w = 0)
                    if (first_step) {
                        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
                        acc0 = p2g_mfma(y, w01.x, zero);
                        acc1 = p2g_mfma(y, w01.y, zero);
                    } else {
                        acc0 = p2g_mfma(y, w01.x, acc0);
                        acc1 = p2g_mfma(y, w01.y, acc1);
                    }
                    // (after the MFMAs, which have read this step's operands: the next ones go to the same registers)
                    if (!last_step) load_ops(4 * (k + 1) * STG);
                };
                if (nsteps == 1) {
                    step(0, true, true);
                } else {
                    step(0, true, false);
#define MPM_P2G_MIDDLE(k) if (nsteps - 1 == k) goto last_step; step(k, false, false);
                    MPM_P2G_MIDDLE(1) MPM_P2G_MIDDLE(2) MPM_P2G_MIDDLE(3) MPM_P2G_MIDDLE(4) MPM_P2G_MIDDLE(5)
                    MPM_P2G_MIDDLE(6) MPM_P2G_MIDDLE(7) MPM_P2G_MIDDLE(8) MPM_P2G_MIDDLE(9) MPM_P2G_MIDDLE(10)
                    MPM_P2G_MIDDLE(11) MPM_P2G_MIDDLE(12) MPM_P2G_MIDDLE(13) MPM_P2G_MIDDLE(14)
#undef MPM_P2G_MIDDLE
                last_step:
                    step(nsteps - 1, false, true);
                }
                // the next cell's first step: rows s1 .. s1 + 3 <= 66 (a next cell starts at s1 <= 63; after the last one
                // the reads are not used, and an unconditional read leaves no old operands to carry over)
                cell_rows(min(s1, 63));
                if (prof) { asm volatile("" :: "v"(acc0), "v"(acc1)); const unsigned long long tm = __builtin_readcyclecounter(); pc[2] += tm - tq[2]; tq[2] = tm; }
                s0 = s1;
                const int crx = ckey >> 6, cry = (ckey >> 3) & 7, crz = ckey & 7;
                // the mask depends on (rx >> 1, ry >> 1, rz >> 1) only: 64 combinations, one per lane of `reach_of_lane`
                mymask |= (unsigned)__builtin_amdgcn_readlane((int)reach_of_lane, ((ckey >> 3) & 0x30) | ((ckey >> 2) & 0xC) | ((ckey >> 1) & 3));
                long long* tb = tile + ((crx * TILE_W + cry) * TILE_W + crz) * 4;
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const f32x4 a = t ? acc1 : acc0;
                    // The four terms of this lane's (node, component), x_r = a[r] * fac[r], summed in pairs: (x0 + x1) + (x2 + x3).
                    // Two of the products ride in fused multiply-adds, with the same bits as products and sums of their
                    // own: a factor is 0, 1 or 2 times the power of two of the scale, so x1 and x3 are EXACT (the scale is
                    // 1 here or, in fixed point, far above 1 for any total mass below 2^47: nothing is pushed into the
                    // subnormal range), and fma(a1, f1, x0) rounds the same real number x0 + x1 once, as the sum does.  A zero
                    // product keeps its sign inside the fma, so the sum of two zeros gets the sign the separate sum gives it;
                    // an infinite or NaN a[r] gives the same infinity or NaN either way (inf * 0 is NaN in both).  Only a
                    // product beyond the largest float differs -- infinity then, a finite sum now where x0 cancels it: node
                    // sums of ~1e38, or > 2^62 quanta, which fixed point reports either way (fix_worst).
                    // Without the scale fac[0] is 1 for every lane that stores (delta >= 0), and x0 is a[0] itself.
                    float val;
                    {
#pragma clang fp contract(off)
                        const float x0 = EXACT ? a[0] * fac[t][0] : a[0], x2 = a[2] * fac[t][2];
                        val = fmaf(a[1], fac[t][1], x0) + fmaf(a[3], fac[t][3], x2);
                    }
                    if (delta[t] >= 0 && !(diag_flags(p) & 16)) {
                        if (EXACT) lds_add_fixed(tb + delta[t], val, fix_worst);
                        else __hip_atomic_fetch_add(reinterpret_cast<double*>(tb + delta[t]), (double)val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    }
                }
                if (prof) pc[3] += __builtin_readcyclecounter() - tq[2];
            }
            if (prof) {
                const unsigned long long te = __builtin_readcyclecounter();
                pc[0] += tq[1] - tq[0];   // derive + group + stage
                pc[1] += te - tq[1];      // contraction phase
                pc[6] += 1;
            }
            __builtin_amdgcn_s_setprio(0);
            // the next group's staging writes must not overtake this group's reads
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
        if (prof) pc[7] = __builtin_readcyclecounter() - tb0;  // whole block, before the final barrier + slab
        if (prof && lane == 0)
            for (int q = 0; q < 8; ++q) atomicAdd(&p.dbgbuf[q], pc[q]);
        if (mymask && lane == 0) atomicOr(&s_mask, mymask);
        if (__ballot(out_worst > (unsigned)(TILE_W - 3)) && lane == 0) atomicOr(&ctl->error, ERR_DRIFT);
        if (EXACT && __ballot(fix_worst >= __float_as_uint(0x1p62f)) && lane == 0) atomicOr(&ctl->error, ERR_RANGE);
        if (p.dist.on && __ballot(halo_bad) && lane == 0) atomicOr(&ctl->error, ERR_HALO);
        __syncthreads();
        if (prof && lane == 0) atomicAdd(&p.dbgbuf[15], (unsigned long long)__builtin_readcyclecounter() - tb0 - pc[7]);   // wave 0 at the closing barrier
        float4* out = p.slab + (size_t)item * TILE_N;
        bool not_finite = false;
        for (int n = tid; n < TILE_N; n += P2G_THREADS) {
            const long long* q = tile + n * 4;
            float4 o;
            if (EXACT) {
                o = make_float4((float)((double)q[0] * p.unfix_p), (float)((double)q[1] * p.unfix_p),
                                (float)((double)q[2] * p.unfix_p), (float)((double)q[3] * p.unfix_m));
            } else {
                const double* d = reinterpret_cast<const double*>(q);
                o = make_float4((float)d[0], (float)d[1], (float)d[2], (float)d[3]);
                // (NaN or infinity in a sum: what the fixed-point conversion reports per contribution)
                not_finite |= !(fabsf(o.x) + fabsf(o.y) + fabsf(o.z) + fabsf(o.w) < __int_as_float(0x7F800000));
            }
            out[n] = o;
        }
        if (!EXACT && __ballot(not_finite) && lane == 0) atomicOr(&ctl->error, ERR_RANGE);
        if (tid == 0) p.slab_mask[item] = s_mask;
        if ((diag_flags(p) & 4) && tid == 0) {
            atomicAdd(&p.dbgbuf[12], (unsigned long long)__builtin_readcyclecounter() - tb0);
            atomicAdd(&p.dbgbuf[13], 1ull);
        }
    }
}

// ---------------------------------------------------------------------------
// Grid: per active block, sum the overlapping tiles (fixed order => the grid is
// a pure function of the slabs, no float atomics), then the explicit update.
// MODE 0: store raw sums (mvx,mvy,mvz,m): the state "after ParticleToGrid" (mpm_download_array)
//         and the payload of the multi-GPU halo exchange.
// MODE 1: gather + v = mv/m, walls, analytic colliders per mpm_bc, store v and v*.
// MODE 2: like 1 but starting from the raw sums already in gv (after neighbours' sums were added).
// ---------------------------------------------------------------------------
// Analytic colliders of the grid update: a runtime table in place of the reference's compile-time
// scenes (update_grid_kernel<T, MPM_BOUNDARY_CONDITION>, cuda_mpm_kernels.cuh:660-789).  The first
// collider of the list whose region contains the node decides (the reference's `else` / `break`
// chains, :694-734, :752-774).
struct GridCollider {       // mirrors mpm_grid_collider_t (include/mpm_hip.h)
    int shape;              // 0 sphere (centre p, radius), 1 half-space (inside: n . (x - p) < 0)
    int mode;               // 0 fixed, 1 slip while approaching (scene 0), 2 slip whenever inside (scene 2)
    float p[3], n[3], radius, v[3], friction;
};
constexpr int MAX_GRID_COLLIDERS = 16;
struct GridColliders {
    int n;
    GridCollider c[MAX_GRID_COLLIDERS];
};

constexpr int GRID_LIST = 160;   // slabs over one block: 27 neighbours x splits
MPM_DEV int __reduce_max_sync_i32(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d));
    return v;
}

template <int MODE>
__global__ __launch_bounds__(256) void k_grid(DP p, GridColliders gc) {
#define MPM_GRID_BODIES 0
#include "mpm_grid_update.inc"
#undef MPM_GRID_BODIES
}

// ---------------------------------------------------------------------------
// G2P
// ---------------------------------------------------------------------------
// Stage the (TILE_W)^3 node velocities around a home block into LDS.
constexpr int G2P_THREADS = 512, G2P_WAVES = 4;
constexpr int LOAD_TILE_NQ = (TILE_N + G2P_THREADS - 1) / G2P_THREADS;
MPM_DEV void load_tile(const DP& p, unsigned h, float4* tile, const float4* field, int nthreads, unsigned long long* stamps = nullptr) {
    const int* nbr = p.home_nbr_act + (size_t)h * 27;
    // NQ nodes per thread (TILE_N <= NQ * nthreads), branch-free and in three sweeps so that the
    // table loads and then the node loads of all are in flight together
    constexpr int NQ = LOAD_TILE_NQ;
    int a[NQ], cell[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int n = min((int)threadIdx.x + q * nthreads, TILE_N - 1);
        const int tx = n / (TILE_W * TILE_W), ty = (n / TILE_W) % TILE_W, tz = n % TILE_W;
        const int qx = tx - FREE_ZONE + 4, qy = ty - FREE_ZONE + 4, qz = tz - FREE_ZONE + 4;  // >= 2
        a[q] = nbr[(qx >> 2) * 9 + (qy >> 2) * 3 + (qz >> 2)];
        cell[q] = ((qx & 3) << 4) + ((qy & 3) << 2) + (qz & 3);
    }
    if (MPM_DIAG && stamps) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); stamps[0] = __builtin_readcyclecounter(); }
    float4 v[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) v[q] = field[(size_t)max(a[q], 0) * 64 + cell[q]];
    if (MPM_DIAG && stamps) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); stamps[1] = __builtin_readcyclecounter(); }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int n = (int)threadIdx.x + q * nthreads;
        if (n < TILE_N) tile[n] = a[q] >= 0 ? v[q] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// returns bit 0: the advected particle no longer fits the tile (re-sort needed); bit 1: partitioned
// domain, the stencil of a ghost copy reached nodes whose sums this rank does not have in full
MPM_DEV int g2p_particle(const DP& p, const PSet& S, const float4* tile, unsigned i, float x, float y, float z,
                            float vol, int ox, int oy, int oz, float dt) {
    const Stencil st = make_stencil(p, x, y, z, ox, oy, oz);
    int bits = 0;
    if (p.dist.on && vol < 0.f) {
        const int gx = ox + st.rx;
        if (gx < p.dist.own_lo - p.dist.zone_cells || gx + 2 >= p.dist.own_hi + p.dist.zone_cells) bits = 2;
    }
    float nv[3] = {0.f, 0.f, 0.f}, nC[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const float4* base = tile + ((st.rx * TILE_W + st.ry) * TILE_W + st.rz);
    // The stencil weight is a product w_i(x) w_j(y) w_k(z), so the 27-node sums
    //     v   = sum w v_n,      C[r][c] = sum w v_n[r] (n - fx)[c]
    // factorise: contract z along each row of 3 nodes, then y over the 3 rows of a plane, then x
    // over the 3 planes (279 multiply-adds instead of 27 x 14).  One z-row is loaded at a time:
    // keeping all 27 node loads in flight costs ~200 VGPRs.
    const float ez[3] = {st.wz[0] * (0.f - st.fx[2]), st.wz[1] * (1.f - st.fx[2]), st.wz[2] * (2.f - st.fx[2])};
    const float ey[3] = {st.wy[0] * (0.f - st.fx[1]), st.wy[1] * (1.f - st.fx[1]), st.wy[2] * (2.f - st.fx[1])};
    // Packed arithmetic (v_pk_fma_f32, two lanes of fused multiply-adds per issue slot): the z contraction
    // carries the pair (w_k, w_k (k - fz)) so that A and Az come out of one chain, and so do (B, Bz) and
    // (v, C[:,2]).  Fully unrolled: no selects for the row weights, constant LDS offsets.
    const f32x2 W0 = {st.wz[0], ez[0]}, W1 = {st.wz[1], ez[1]}, W2 = {st.wz[2], ez[2]};
    const f32x2 zero2 = {0.f, 0.f};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        f32x2 BB[3] = {zero2, zero2, zero2};   // (B, Bz)[r]
        float By[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const float4* row = base + (a * TILE_W + b) * TILE_W;
            const float4 g0 = row[0], g1 = row[1], g2 = row[2];
            const float wb = st.wy[b], eb = ey[b];
            const f32x2 wb2 = {wb, wb};
            const float c0[3] = {g0.x, g0.y, g0.z}, c1[3] = {g1.x, g1.y, g1.z}, c2[3] = {g2.x, g2.y, g2.z};
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                f32x2 AA;   // (A, Az)[r]
                if (r == 2) {
                    // the z components sit in the low halves of the (z, m) pairs of the three nodes: broadcast by the
                    // instruction's operand select instead of by a move each (the compiler loads 12 bytes per node and
                    // then has no pair to select from): 27 moves less per particle, k_g2p 21.85 -> 20.95 us
                    // (DESIGN_HISTORY.md section 3.2)
                    const f32x2 z0 = {g0.z, g0.w}, z1 = {g1.z, g1.w}, z2 = {g2.z, g2.w};
                    // (one block with its own wait states between the dependent packed operations: the compiler puts an
                    // s_nop between its own, and must not be relied on to know what is inside an asm statement)
                    asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[1,0]\n\ts_nop 0\n\t"
                        "v_pk_fma_f32 %0, %3, %4, %0 op_sel_hi:[1,0,1]\n\ts_nop 0\n\t"
                        "v_pk_fma_f32 %0, %5, %6, %0 op_sel_hi:[1,0,1]"
                        : "=&v"(AA) : "v"(W0), "v"(z0), "v"(W1), "v"(z1), "v"(W2), "v"(z2));
                } else {
                    const f32x2 s0 = {c0[r], c0[r]}, s1 = {c1[r], c1[r]}, s2 = {c2[r], c2[r]};
                    AA = __builtin_elementwise_fma(W2, s2, __builtin_elementwise_fma(W1, s1, W0 * s0));
                }
                BB[r] = __builtin_elementwise_fma(wb2, AA, BB[r]);
                By[r] = fmaf(eb, AA.x, By[r]);
            }
        }
        // plane a is complete
        const float wa = st.wx[a];
        const float ea = wa * ((float)a - st.fx[0]);
        const f32x2 wa2 = {wa, wa};
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            f32x2 vc = {nv[r], nC[r * 3 + 2]};
            vc = __builtin_elementwise_fma(wa2, BB[r], vc);
            nv[r] = vc.x;
            nC[r * 3 + 2] = vc.y;
            nC[r * 3 + 0] = fmaf(ea, BB[r].x, nC[r * 3 + 0]);
            nC[r * 3 + 1] = fmaf(wa, By[r], nC[r * 3 + 1]);
        }
    }
    if (diag_flags(p) & 256) {  // ablation: no stores
        if (nv[0] + nC[0] + nC[4] + nC[8] == 1.2345e30f) S.q[1][i].x = nv[0];
        return 0;
    }
    const float sc = 4.f * p.dxinv;
    const float ca = (p.M.V + 1.f) * .5f, cb = (p.M.V - 1.f) * .5f;
    float Cn[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        // (an explicit fused multiply-add: left to the compiler, WHICH of the two products is fused changes from build to
        // build with the scheduling of the code around it, and C with it in the last bit)
        for (int c = 0; c < 3; ++c) Cn[r * 3 + c] = fmaf(ca, sc * nC[r * 3 + c], cb * (sc * nC[c * 3 + r]));
    // up to four 16-byte stores per particle (in this order: it keeps the kernel within the registers of its occupancy
    // without scratch)
    const float xn = x + nv[0] * dt, yn = y + nv[1] * dt, zn = z + nv[2] * dt;
    // A face particle's position and velocity are only looked at from outside (downloads): CalcFemStateAndForce
    // replaces them by the means of the corners before anything in a substep reads them (the re-sort bins a face by
    // the same means), and takes C8 from the c8 plane.  Between the substeps of one mpm_run_substeps batch the two
    // records are therefore not written (DP::lean_g2p; the last substep of a batch and the phase-by-phase calls
    // write them): 36 instead of 68 bytes out per face.
    const bool is_face = i < (unsigned)p.Nf;
    const bool full = !(p.lean_g2p && is_face);
    // (in this order: another one costs the kernel its register budget)
    S.q[2][i] = make_float4(Cn[0], Cn[1], Cn[2], Cn[3]);
    S.q[3][i] = make_float4(Cn[4], Cn[5], Cn[6], Cn[7]);
    // A vertex between the substeps of a batch: the record this lane loaded -- the position this substep's k_fem gathered --
    // goes to PSet::xp, from which the next k_fem forms the in-plane columns of F that this substep's did not store
    // (Ctl::f_inplane_stale; before the advected position replaces it)
    if (p.lean_g2p && !is_face) S.xp[i - (unsigned)p.Nf] = make_float4(x, y, z, vol);
    if (full) {
        S.q[0][i] = make_float4(xn, yn, zn, vol);
        S.q[1][i] = make_float4(nv[0], nv[1], nv[2], Cn[8]);
    }
    if (is_face) S.c8[i] = Cn[8];
    // Does the advected particle still fit this block's tile?  Vertices are tested where the next
    // P2G will find them; a face is re-centred on its corners by the FEM kernel first, which moves
    // it by O(dt * velocity spread inside the face), hence the 1/8-cell guard band.
    const float guard = .125f, top = (float)(TILE_W - 2) - guard;
    const float tx = xn * p.dxinv - .5f - (float)ox, ty = yn * p.dxinv - .5f - (float)oy,
                tz = zn * p.dxinv - .5f - (float)oz;
    return bits | (int)!(tx >= guard && tx < top && ty >= guard && ty < top && tz >= guard && tz < top);
}

__global__ __launch_bounds__(G2P_THREADS) __attribute__((amdgpu_waves_per_eu(G2P_WAVES, G2P_WAVES))) void k_g2p(DP p, float dt) {
    __shared__ float4 tile[TILE_N];
    const Ctl* ctl = p.ctl;
    if (p.gated && ctl->skip_this) {   // (not need_rebuild itself: this kernel raises it while it runs)
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&p.ctl->skipped, 1u);
        return;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        p.ctl->time_since_resort += dt;   // (see Ctl::quiet_time)
        // what the next k_fem finds: this substep's did not store F's in-plane columns, and the vertex lanes below leave
        // the positions they are made of in PSet::xp -- or it did, and they do not
        p.ctl->f_inplane_stale = p.lean_g2p;
    }
    const PSet& S = p.set[ctl->cur];
    const unsigned n_items = ctl->n_items;
    for (unsigned q = blockIdx.x; q < n_items; q += gridDim.x) {
        __syncthreads();  // everybody is done with the previous tile
        const int4 fa = p.item_flat[2 * q];
        const unsigned h = (unsigned)fa.y;
        if (p.halo_cls >= 0) {   // split gather around the halo exchange (uniform over the workgroup)
            int hx, hy, hz;
            block_coords((uint32_t)fa.z, hx, hy, hz);
            if (!halo_item_selected(p, hx)) continue;
        }
        // (bit 2: every wave of every workgroup, which perturbs the kernel; bit 12: wave 0 of eight workgroups spread over
        // the heaviest-first order, which does not)
        const bool prof = (diag_flags(p) & 4) != 0 || ((diag_flags(p) & 4096) != 0 && (blockIdx.x & 63u) == 5u && threadIdx.x < 64);
        unsigned long long t0 = 0, t1 = 0;
        if (prof) t0 = __builtin_readcyclecounter();
        const int4 rg = p.item_rng[q];   // the item's particles: face slots [x, y), vertex slots [z, w)
        // faces then vertices as one index space: a single copy of the (large) particle body
        const int nfb = rg.y - rg.x, total = nfb + (rg.w - rg.z);
        auto slot_of = [&](int u) { return (unsigned)(u < nfb ? rg.x + u : rg.z + (u - nfb)); };
        // the first positions are requested before the tile is staged, later ones one iteration
        // ahead, so the HBM latency of the particle stream hides behind LDS work
        int u = (int)threadIdx.x;
        int left = 0;
        unsigned i = slot_of(u < total ? u : 0);
        float4 pq = S.q[0][i];
        unsigned long long ts[2] = {0, 0};
        load_tile(p, h, tile, p.gv, G2P_THREADS, prof ? ts : nullptr);
        __syncthreads();
        if (prof) t1 = __builtin_readcyclecounter();
        if (prof && (threadIdx.x & 63) == 0 && (diag_flags(p) & 4096)) {
            atomicAdd(&p.dbgbuf[12], ts[0] - t0);   // item descriptor + neighbour table arrived
            atomicAdd(&p.dbgbuf[13], ts[1] - ts[0]);   // node values arrived
        }
        int bx, by, bz;
        block_coords((uint32_t)fa.z, bx, by, bz);
        const int ox = bx * 4 - FREE_ZONE, oy = by * 4 - FREE_ZONE, oz = bz * 4 - FREE_ZONE;
#pragma unroll 1
        for (; u < total; u += G2P_THREADS) {
            const unsigned ci = i;
            const float4 c = pq;
            const int un = u + G2P_THREADS;
            if (un < total) {
                i = slot_of(un);
                pq = S.q[0][i];
            }
            left |= g2p_particle(p, S, tile, ci, c.x, c.y, c.z, c.w, ox, oy, oz, dt);
        }
        // a plain store: the flag only ever goes 0 -> 1 inside this kernel (same-address atomics
        // from thousands of waves would serialise at the memory side)
        if (__ballot(left & 1) && (threadIdx.x & 63) == 0) p.ctl->need_rebuild = 1;
        if (p.dist.on && __ballot(left & 2) && (threadIdx.x & 63) == 0) atomicOr(&p.ctl->error, ERR_HALO);
        if (prof && (threadIdx.x & 63) == 0) {
            const unsigned long long t2 = __builtin_readcyclecounter();
            atomicAdd(&p.dbgbuf[8], t1 - t0);
            atomicAdd(&p.dbgbuf[9], t2 - t1);
            atomicAdd(&p.dbgbuf[10], (unsigned long long)((total + G2P_THREADS - 1) / G2P_THREADS));
            atomicAdd(&p.dbgbuf[11], 1ull);
        }
    }
}

// ---------------------------------------------------------------------------
// Multi-GPU halo: ranks tile the domain along x, each with its own engine and local grid.  After
// the local gather (k_grid<0>) a rank packs the raw node sums of its active blocks in the layers
// next to a cut, relabelled into the neighbour's block coordinates; the neighbour adds them to
// its own sums (k_halo_add) and both then run the same grid update (k_grid<2>) on shared blocks.
// The buffers are zone exchange buffers with one vector per cell (mpm_zone_buffer.h).
// ---------------------------------------------------------------------------

// both zones / both received buffers of a chain rank in one launch each (blockIdx.y selects)
__global__ __launch_bounds__(256) void k_halo_pack2(DP p, Zones z, unsigned cap) {
    const int k = blockIdx.y;
    uint32_t* buf = z.buf[k];
    const unsigned n_active = p.ctl->n_active;
    for (unsigned a = blockIdx.x * 4 + (threadIdx.x >> 6); a < n_active; a += gridDim.x * 4) {
        int bx, by, bz;
        block_coords(p.act_block[a], bx, by, bz);
        if (bx < z.lo[k] || bx > z.hi[k]) continue;   // wave-uniform
        const int nbx = bx + z.shift[k];
        if (nbx < 0 || nbx >= p.nb) continue;
        const int slot = zbuf_claim(&buf[0], cap, p.ctl);
        if (slot < 0) continue;
        zbuf_store<1>(buf, cap, (unsigned)slot, block_id((uint32_t)nbx, (uint32_t)by, (uint32_t)bz), p.gv + (size_t)a * 64 + (threadIdx.x & 63));
    }
}

// ---- DIRECT halo (peer-to-peer stores + sequence flags) ---------------------------------------------------------------
// k_grid<0> of substep s has stored the zone sums into the neighbours' receive buffers (its halo_pbuf point into peer
// memory).  This one-thread kernel, behind it on the same stream, tells the neighbours: the kernel boundary in front of
// it has made those stores complete; publish_then_flag orders the flag behind them for an observer on another device.
// (Cross-device ordering cannot be observed on a box with one GPU: the protocol, not its memory model, is what the
// one-GPU tests exercise -- DESIGN.md section 5.)  cnt_* / hdr_*: the pack counted its entries in words of THIS device's
// memory (zbuf_claim); the counts go into the neighbours' buffer headers here, in front of the flags.
__global__ void k_halo_signal(uint32_t* flag_a, uint32_t* flag_b, uint32_t seq, const uint32_t* cnt_a, uint32_t* hdr_a,
                              const uint32_t* cnt_b, uint32_t* hdr_b, unsigned cap) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (hdr_a) __hip_atomic_store(hdr_a, min(*cnt_a, cap), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (hdr_b) __hip_atomic_store(hdr_b, min(*cnt_b, cap), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    publish_then_flag(2, seq, [&](int k) { return k == 0 ? flag_a : flag_b; });
}
// ... and this one, one thread, waits (wait_flag: bounded) until both neighbours have said so for substep `seq`; a
// neighbour that never arrives raises ERR_HALO.  The kernel boundary behind it is the acquire for k_grid<2>, which then
// reads the received sums (fine-grained memory: not held in this device's L2).
__global__ void k_halo_wait(const uint32_t* flag_a, const uint32_t* flag_b, uint32_t seq, unsigned long long timeout_ticks, Ctl* ctl) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const unsigned long long t0 = wall_clock64();
    bool ok = true;
    if (flag_a) ok &= wait_flag<20>(flag_a, seq, t0, timeout_ticks);
    if (flag_b) ok &= wait_flag<20>(flag_b, seq, t0, timeout_ticks);
    if (!ok) atomicOr(&ctl->error, ERR_HALO);
}
// (a block lies in one zone only, so the two buffers of a launch touch disjoint cells)
__global__ __launch_bounds__(256) void k_halo_add2(DP p, Zones z, unsigned cap) {
    const uint32_t* buf = z.buf[blockIdx.y];
    const unsigned n = zbuf_count(buf, cap);
    for (unsigned e = blockIdx.x * 4 + (threadIdx.x >> 6); e < n; e += gridDim.x * 4) {
        uint32_t id;
        const int a = zbuf_entry_block(p, buf, e, &id);
        if (a < 0) continue;
        if (p.halo_nz > 0) {  // with a split update only zone blocks are still raw sums
            int hx, hy, hz;
            block_coords(id, hx, hy, hz);
            if (!in_halo_zone(p, hx)) {
                if ((threadIdx.x & 63) == 0) atomicOr(&p.ctl->error, ERR_CAPACITY);
                continue;
            }
        }
        zbuf_add<1>(buf, cap, e, p.gv + (size_t)a * 64 + (threadIdx.x & 63));
    }
}

}  // namespace mpm
