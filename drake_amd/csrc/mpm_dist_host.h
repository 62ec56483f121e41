// Host side of the partitioned domain (mpm_dist_*): the slot space of a rank and its resize, the set-up, the band
// re-tuning and the migration -- what the entry points in mpm_engine.hip call once their arguments are checked.
// Included by mpm_engine.hip after mpm_host.h and mpm_dist.h.
#pragma once
#include <type_traits>

#include "mpm_dist.h"
#include "mpm_host.h"

// (with C linkage: the kernel keeps the symbol it has had since it was written inside mpm_engine.hip's extern "C" block,
// which the profiles and kernel tables name)
extern "C" {
namespace mpm {
// after the arrays have moved: vertex slots start at new_nf instead of old_nf
__global__ __launch_bounds__(256) void k_dist_shift_slots(DP p, int old_nf, int new_nf, int nfa) {
    const PSet& S = p.set[p.ctl->cur];
    const int gs = gridDim.x * 256, t0 = blockIdx.x * 256 + threadIdx.x;
    auto shifted = [&](int s) { return s >= old_nf ? s - old_nf + new_nf : s; };
    for (int i = t0; i < nfa; i += gs) {
        float4 f3 = S.fq[3][i];
        f3.y = __int_as_float(shifted(__float_as_int(f3.y)));
        f3.z = __int_as_float(shifted(__float_as_int(f3.z)));
        f3.w = __int_as_float(shifted(__float_as_int(f3.w)));
        S.fq[3][i] = f3;
    }
    for (int g = t0; g < p.NpG; g += gs) p.imap[g] = shifted(p.imap[g]);
}
}  // namespace mpm
}  // extern "C"

// Slot space of a partitioned rank.  The rank was finalised with the whole scene (every rank runs the same Finalize, so
// ghost copies start bit-identical to their owners'); the first partitioned re-sort has compacted what it keeps into
// slots [0, nfa) and [Nf, Nf + nva).  dist_resize re-allocates every array indexed by particle slot for `new_nf` face and
// `new_nv` vertex slots, copies the held ranges, shifts the slot references and asks for a re-sort (block tables, work
// items and wave groups hold slot ranges).  mpm_dist_init calls it once to SHRINK the rank to headroom x its share and
// to release the tables of the whole scene's topology (corner ids per face, adjacency CSR, Dm^-1 by original id: per
// slot the rank keeps the same information by original id, DP::fg / vg, and migration records carry it); a migration
// that would overflow the slot space calls it again to GROW (mpm_dist_migrate_apply: the stream is idle there).  What
// stays whole-scene sized is the id -> slot map and the slot-order bookkeeping (13 bytes per particle of the scene).
static size_t dist_slot_capacity(float headroom, size_t held, size_t all) {
    if (!(headroom > 0.f)) return all;   // (0: keep the whole scene's size)
    return std::min(all, std::max<size_t>((size_t)((double)held * std::max(1.f, headroom)) + 256, 1024));
}
// TWO-PHASE: phase 1 allocates every new array and touches nothing of the engine -- a failure there (device
// memory exhausted) frees what phase 1 got and returns with the engine exactly as it was, still usable at its old size;
// phase 2 (copies, swaps, frees) cannot fail for lack of memory.
static int dist_resize(mpm_engine* e, size_t new_nf, size_t new_nv, bool first) {
    DP& p = e->dp;
    HIP_TRY(hipStreamSynchronize(e->stream));
    Ctl c;
    D2H(e, &c, p.ctl, sizeof(Ctl));
    // (what a migration appended behind the active particles and the re-sort has not merged yet is kept too)
    REQUIRE(c.nfa >= 0 && c.nva >= 0 && c.add_f >= 0 && c.add_v >= 0, "dist_resize: corrupt control block");
    const size_t nfa = (size_t)c.nfa + (size_t)c.add_f, nva = (size_t)c.nva + (size_t)c.add_v;
    const size_t old_nf = (size_t)p.Nf;
    REQUIRE(nfa <= old_nf && nva <= (size_t)p.Nv, "dist_resize: the control block counts more particles than the slot space holds");
    REQUIRE(new_nf >= nfa && new_nv >= nva, "dist_resize: smaller than what the rank holds");
    REQUIRE(new_nf + new_nv < ((size_t)1 << 30), "dist_resize: too many particle slots");
    const size_t new_np = new_nf + new_nv;
    const int cur = c.cur & 1;
    const unsigned new_q_stride = (unsigned)((new_np + 63) & ~(size_t)63);

    // ---- phase 1: allocate ----------------------------------------------------------------------------------------
    struct Copy { size_t dst_off, src_off, bytes; };
    struct Plan {
        void** owner;             // where the engine keeps the allocation's base pointer
        void* fresh;              // its replacement
        std::vector<Copy> keep;   // byte ranges carried over (old base -> fresh)
    };
    std::vector<Plan> plans;
    plans.reserve(64);
    FreshArrays fresh_arrays(e);   // (freed again unless phase 1 gets all of them)
    int rc = 0;
    auto plan = [&](auto*& ptr, size_t n_new, std::vector<Copy> keep_elems) -> int {
        using T = std::remove_pointer_t<std::remove_reference_t<decltype(ptr)>>;
        T* fresh = nullptr;
        if (int r = fresh_arrays.alloc(&fresh, n_new, true)) return r;
        Plan pl;
        pl.owner = (void**)(&ptr);
        pl.fresh = (void*)fresh;
        for (Copy k : keep_elems)
            if (k.bytes) pl.keep.push_back(Copy{k.dst_off * sizeof(T), k.src_off * sizeof(T), k.bytes * sizeof(T)});
        plans.push_back(std::move(pl));
        return 0;
    };
    float4* q_base[2] = {p.set[0].q[0], p.set[1].q[0]};   // (the four planes of a set are one allocation)
    float* f_base = p.f[0];
    for (int s = 0; s < 2 && !rc; ++s) {
        PSet& S = p.set[s];
        const bool live = s == cur;
        std::vector<Copy> planes;
        if (live)
            for (int d = 0; d < 4; ++d) {
                planes.push_back(Copy{(size_t)d * new_q_stride, (size_t)d * p.q_stride, nfa});
                planes.push_back(Copy{(size_t)d * new_q_stride + new_nf, (size_t)d * p.q_stride + old_nf, nva});
            }
        rc = plan(q_base[s], 4 * (size_t)new_q_stride, planes);
        if (!rc) rc = plan(S.pid, new_np, live ? std::vector<Copy>{{0, 0, nfa}, {new_nf, old_nf, nva}} : std::vector<Copy>{});
        const std::vector<Copy> kf = live ? std::vector<Copy>{{0, 0, nfa}} : std::vector<Copy>{};
        const std::vector<Copy> kv = live ? std::vector<Copy>{{0, 0, nva}} : std::vector<Copy>{};
        for (int d = 0; d < 4 && !rc; ++d) rc = plan(S.fq[d], new_nf, kf);
        if (!rc) rc = plan(S.f8, new_nf, kf);
        if (!rc) rc = plan(S.c8, new_nf, kf);
        if (!rc) rc = plan(p.fg[s], new_nf, kf);
        for (int d = 0; d < 2 && !rc; ++d) rc = plan(p.vg[s][d], new_nv, kv);
    }
    // per-substep outputs and re-sort scratch: nothing to keep
    if (!rc) rc = plan(p.ta, new_nf, {});
    if (!rc) rc = plan(p.G3, 3 * new_nf, {});
    // (the vertices' rows of force triples: zero-filled; the re-sort that follows writes the zeros / marks of every held
    // vertex again and k_fem the rest before anything reads them)
    if (!rc) rc = plan(p.VF, 3 * vf_entry((unsigned)new_nv + VF_CHUNK, 0), {});
    if (!rc) rc = plan(f_base, 3 * (size_t)new_q_stride, {});
    if (!rc) rc = plan(p.pkey, new_np, {});
    if (!rc) rc = plan(p.prank, new_np, {});
    if (!rc) rc = plan(p.src_of, new_np, {});
    if (!rc) rc = plan(p.dst_of, new_np, {});
    if (!rc) rc = plan(p.home_groups, new_np / 64 + p.capH + 2, {});
    if (rc) {
        const std::string why = g_last_error;
        (void)hipStreamSynchronize(e->stream);
        return fail(rc, "dist_resize: " + why + " -- the rank keeps its slot space of " + std::to_string(p.Nf) + " + " +
                            std::to_string(p.Nv) + " slots and stays usable");
    }

    // ---- phase 2: copy, swap, free (no allocation from here on) ------------------------------------------------------
    fresh_arrays.commit();
    for (Plan& pl : plans)
        for (const Copy& k : pl.keep)
            HIP_TRY(hipMemcpyAsync((char*)pl.fresh + k.dst_off, (const char*)*pl.owner + k.src_off, k.bytes,
                                   hipMemcpyDeviceToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    for (Plan& pl : plans) {
        void* old = *pl.owner;
        e->dfree(old);
        *pl.owner = pl.fresh;
    }
    for (int s = 0; s < 2; ++s)
        for (int d = 0; d < 4; ++d) p.set[s].q[d] = q_base[s] + (size_t)d * new_q_stride;
    for (int d = 0; d < 3; ++d) p.f[d] = f_base + (size_t)d * new_q_stride;
    if (first) {
        // (a partitioned domain runs no lean substeps: nothing writes or reads PSet::xp, DP::lean_g2p)
        for (int s = 0; s < 2; ++s) e->dfree(p.set[s].xp);
        // the whole scene's topology tables
        for (int d = 0; d < 3; ++d) {
            int* t = const_cast<int*>(p.idx_orig[d]);
            e->dfree(t);
            p.idx_orig[d] = nullptr;
        }
        float4* dm = const_cast<float4*>(p.dm_orig);
        e->dfree(dm);
        p.dm_orig = nullptr;
        if (e->max_valence <= 8) {
            int* a = const_cast<int*>(p.adj_off);
            int* b = const_cast<int*>(p.adj_fc);
            e->dfree(a); e->dfree(b);
            p.adj_off = nullptr; p.adj_fc = nullptr;
        }
        // (a mesh with a vertex of more than eight faces keeps the scene's adjacency -- 4 bytes per vertex and 12 per face
        // on every rank: such a vertex's record holds a mark instead of face ids, and its force walks the adjacency by
        // original id through the id -> slot map, wherever the vertex migrates: vertex_force_csr)
    }
    p.Np = (int)new_np; p.Nf = (int)new_nf; p.Nv = (int)new_nv;
    p.q_stride = new_q_stride;
    p.f_stride = new_q_stride;
    hipLaunchKernelGGL(k_dist_shift_slots, dim3(1024), dim3(256), 0, e->stream, p, (int)old_nf, (int)new_nf, (int)nfa);
    // block tables, work items and wave groups hold slot ranges: rebuild them on the new slot space
    const int one = 1;
    H2D(e, &p.ctl->need_rebuild, &one, sizeof(int));
    e->dist_resizes += 1;
    if (!first) return 0;   // (a migration follows, and the re-sort that merges what it brings)
    launch_rebuild(e, e->dp);
    D2H(e, &c, p.ctl, sizeof(Ctl));
    return recover_slab_overflow(e, c);
}

static int dist_init(mpm_engine* e, const mpm_dist_config_t* cfg) {
    const int nb = e->dp.nb;
    REQUIRE(cfg->world >= 1 && cfg->rank >= 0 && cfg->rank < cfg->world, "bad rank / world");
    REQUIRE(cfg->own_lo_block >= 0 && cfg->own_lo_block < cfg->own_hi_block && cfg->own_hi_block <= nb,
            "bad slab: need 0 <= own_lo_block < own_hi_block <= blocks per axis");
    const bool auto_bands = cfg->ghost_cells == 0 && cfg->ghost_margin_cells == 0;
    REQUIRE(cfg->zone_blocks >= 1 && (auto_bands || (cfg->ghost_cells >= 1 && cfg->ghost_margin_cells >= 1)),
            "zone_blocks must be positive; ghost_cells and ghost_margin_cells both positive, or both 0 (bands from the mesh)");
    // a ghost vertex may sit ghost_cells + ghost_margin_cells beyond the cut and its stencil reaches 2 nodes further
    REQUIRE(auto_bands || cfg->zone_blocks * 4 >= cfg->ghost_cells + cfg->ghost_margin_cells + 2,
            "zone too shallow for the ghost band: need 4 * zone_blocks >= ghost_cells + ghost_margin_cells + 2");
    // Reach of a face: how far a corner vertex can be from the face particle (the centroid), in cells -- 2/3 of a
    // median, bounded by 0.75 x the longest edge of the mesh as it was handed over (a cloth stretches by per cent).
    float longest_edge = 0.f;
    for (size_t f = 0; f < e->nf; ++f)
        for (int k = 0; k < 3; ++k) {
            const float* A = &e->h_pos[(size_t)e->h_idx[f * 3 + k] * 3];
            const float* B = &e->h_pos[(size_t)e->h_idx[f * 3 + (k + 1) % 3] * 3];
            longest_edge = std::max(longest_edge, std::sqrt((A[0] - B[0]) * (A[0] - B[0]) + (A[1] - B[1]) * (A[1] - B[1]) +
                                                            (A[2] - B[2]) * (A[2] - B[2])));
        }
    longest_edge *= e->dp.dxinv;
    const float reach = .75f * longest_edge;
    // Drift budget.  Between two migrations nothing joins or leaves a rank, so what a rank holds must cover what its
    // owned particles need even after every particle has drifted `delta` cells along x:
    //   an owned vertex needs its adjacent faces:  ghost_w >= reach + 2 delta   (both may have moved)
    //   a face needs its corners:                  vert_w  >= ghost_w + reach   (holds at the migration, nothing leaves after)
    //   a ghost's stencil stays inside the zone:   vert_w + delta <= 4 zone_blocks - 2
    //   an owned particle's stencil does:          delta <= 4 zone_blocks - 3
    // bands from the mesh (ghost_cells = ghost_margin_cells = 0): the widths that make delta largest; given widths:
    // the delta they allow (0: migrate with every substep).
    // (with the hysteresis h of ownership and band membership, Dist::hyst: an owned particle may sit h beyond a cut and a
    // held ghost h beyond its band when the drift starts)
    //   ghost_w >= reach + 2 delta + h;  vert_w >= ghost_w + reach;  vert_w + h + delta <= 4 zone_blocks - 2;
    //   h + delta <= 4 zone_blocks - 3
    const float zone_room = (float)(4 * cfg->zone_blocks - 2);
    float ghost_w, vert_w, delta, hyst = .125f;
    if (auto_bands) {
        // (as much drift as the zone allows, but no more than dist_drift_target: every cell of band is a cell of ghost
        // particles that FEM and GridToParticle advance with every substep -- with slabs of 16 cells the widest bands
        // of a two-block zone, 3.8 / 4.3 cells, are half as many ghosts as owned particles)
        delta = std::min({(zone_room - 2.f * reach - 2.f * hyst) / 3.f, zone_room - 1.f - hyst, e->dist_drift_target});
        REQUIRE(delta > .05f, "mpm_dist_init: the exchanged zone is too shallow for this mesh (4 zone_blocks - 2 must exceed 1.5 x "
                              "the longest mesh edge in cells): use more zone_blocks or a finer mesh");
        ghost_w = reach + 2.f * delta + hyst;
        vert_w = ghost_w + reach;
    } else {
        ghost_w = (float)cfg->ghost_cells;
        vert_w = (float)(cfg->ghost_cells + cfg->ghost_margin_cells);
        if (zone_room - vert_w < 2.f * hyst) hyst = 0.f;   // (bands that fill the zone: no room for it)
        delta = std::max(0.f, std::min({(ghost_w - reach - hyst) * .5f, zone_room - vert_w - hyst, zone_room - 1.f - hyst}));
    }
    const bool has_left = cfg->rank > 0, has_right = cfg->rank < cfg->world - 1;
    // the zones of the two cuts must not overlap (a block is shared by at most two ranks)
    REQUIRE(!(has_left && has_right) || cfg->own_hi_block - cfg->own_lo_block >= 2 * cfg->zone_blocks,
            "slab narrower than two zones: use fewer ranks or zone_blocks = 1");
    REQUIRE(!has_left || (cfg->left_lo_block >= 0 && cfg->left_lo_block < cfg->own_lo_block), "bad left neighbour range");
    REQUIRE(!has_right || (cfg->right_hi_block > cfg->own_hi_block && cfg->right_hi_block <= nb), "bad right neighbour range");
    Dist d{};
    d.on = 1;
    d.rank = cfg->rank; d.world = cfg->world;
    d.own_lo = has_left ? cfg->own_lo_block * 4 : 0;
    d.own_hi = has_right ? cfg->own_hi_block * 4 : nb * 4;
    d.nbr_lo = has_left ? (cfg->rank > 1 ? cfg->left_lo_block * 4 : 0) : 0;
    d.nbr_hi = has_right ? (cfg->rank < cfg->world - 2 ? cfg->right_hi_block * 4 : nb * 4) : nb * 4;
    d.has_left = has_left; d.has_right = has_right;
    d.ghost_w = ghost_w;
    d.vert_w = vert_w;
    d.hyst = hyst;
    d.zone_cells = cfg->zone_blocks * 4;
    d.mig_delta = delta;
    d.mig_reach = vert_w + 2.f * reach + 1.f;
    e->dist_longest_edge = longest_edge;
    e->dist_auto = auto_bands;
    e->dist_reach = reach;
    e->dist_hyst = hyst;
    e->dist_delta_max = std::min((zone_room - 2.f * reach - 2.f * hyst) / 3.f, zone_room - 1.f - hyst);
    if (int rc = e->dalloc(&d.prev, e->np, true)) return rc;
    if (int rc = e->dalloc(&d.mig_min, 32 * 32, true)) return rc;
    // per-slot topology by original id, for every particle at first (nobody has been released yet)
    for (int s = 0; s < 2; ++s) {
        if (int rc = e->dalloc(&e->dp.fg[s], e->nf, false)) return rc;
        for (int k = 0; k < 2; ++k)
            if (int rc = e->dalloc(&e->dp.vg[s][k], e->nv, false)) return rc;
    }
    hipLaunchKernelGGL(k_dist_build_topology, dim3(std::min(e->g_np, 2048u)), dim3(256), 0, e->stream, e->dp);
    e->dp.dist = d;
    hipLaunchKernelGGL(k_dist_init_roles, dim3(e->g_np), dim3(256), 0, e->stream, e->dp);
    int one = 1;
    H2D(e, &e->dp.ctl->need_rebuild, &one, sizeof(int));
    launch_rebuild(e, e->dp);
    {
        Ctl c;
        D2H(e, &c, e->dp.ctl, sizeof(Ctl));
        if (int rc = recover_slab_overflow(e, c)) return rc;
    }
    // the rank keeps its share: the particle arrays shrink to it, the whole scene's topology tables go
    {
        Ctl c;
        D2H(e, &c, e->dp.ctl, sizeof(Ctl));
        if (int rc = dist_resize(e, dist_slot_capacity(e->dist_headroom, (size_t)c.nfa, (size_t)e->dp.Nf),
                                 dist_slot_capacity(e->dist_headroom, (size_t)c.nva, (size_t)e->dp.Nv), true))
            return rc;
    }
    return mpm_sync(e);
}

static int dist_get_geometry(const mpm_engine* e, mpm_dist_geometry_t* out) {
    const Dist& d = e->dp.dist;
    out->face_band_cells = d.ghost_w;
    out->vertex_band_cells = d.vert_w;
    out->drift_budget_cells = d.mig_delta;
    out->longest_edge_cells = e->dist_longest_edge;
    out->slot_resizes = e->dist_resizes;
    out->migrations = e->dist_migrations;
    out->retunes = e->dist_retunes;
    return 0;
}

static int dist_retune(mpm_engine* e, float quiet_time_all, float dt, int* changed_out) {
    if (changed_out) *changed_out = 0;
    if (!e->dist_auto || !e->dist_retune || !(dt > 0.f)) return 0;
    Dist& d = e->dp.dist;
    // The ranks' common estimate says the fastest relevant particle uses up the CURRENT budget in quiet_time_all: that
    // is a speed.  The budget that makes a migration due every dist_target_interval substeps at that speed (half of
    // the estimate is trusted), in steps of an eighth of a cell so that it does not flutter, within what the zone allows:
    float want = e->dist_delta_max;   // (an estimate of 0 or NaN: as wide as the zone allows)
    if (quiet_time_all > 0.f && std::isfinite(quiet_time_all)) {
        const float speed = d.mig_delta / quiet_time_all;   // cells per second
        want = speed * dt * e->dist_target_interval / e->mig_safety;
        want = std::ceil(want * 8.f) * .125f;
    } else if (quiet_time_all > 0.f) {
        want = .125f;   // (an infinite estimate -- nothing moves along x --: the narrowest bands)
    }
    want = std::min(std::max(want, .125f), e->dist_delta_max);
    if (!(want > .05f) || std::fabs(want - d.mig_delta) < .06f) return 0;
    // Every rank computes this from the same numbers at the same migration, so all switch together.  The new widths
    // take effect at the NEXT migration's classification (particles newly inside a wider band are sent then, ghosts
    // outside a narrower one are released then); the interval up to it was budgeted with the old widths.
    d.mig_delta = want;
    d.ghost_w = e->dist_reach + 2.f * want + e->dist_hyst;
    d.vert_w = d.ghost_w + e->dist_reach;
    d.mig_reach = d.vert_w + 2.f * e->dist_reach + 1.f;
    e->dist_retunes += 1;
    if (changed_out) *changed_out = 1;
    return 0;
}

static int dist_migrate_pack(mpm_engine* e, void* send_left, void* send_right, size_t capacity_particles) {
    HIP_TRY(hipMemsetAsync(send_left, 0, 16, e->stream));
    HIP_TRY(hipMemsetAsync(send_right, 0, 16, e->stream));
    hipLaunchKernelGGL(k_dist_classify, dim3(std::min(e->g_np, 2048u)), dim3(256), 0, e->stream, e->dp,
                       static_cast<float4*>(send_left), static_cast<float4*>(send_right), (unsigned)capacity_particles);
    // (the time until the next migration is due, as far as this rank can tell: Ctl::mig_quiet)
    hipLaunchKernelGGL(k_dist_mig_reduce, dim3(1), dim3(64), 0, e->stream, e->dp);
    e->dist_migrations += 1;
    return 0;
}

// What a migration brings, from the two 16-byte headers of the received buffers ([0] records, [1] how many of them are
// faces, [2..3] zero), and the slot space it needs.  Host arithmetic on numbers that came out of BUFFERS (another rank
// wrote them, a transport carried them): nothing is sized from them before they have been checked against the
// buffers' capacity and against the scene -- a header that fails the checks is an error code, never an allocation.
struct MigrationPlan {
    size_t in_f = 0, in_v = 0;       // arriving records: faces, vertices
    size_t need_f = 0, need_v = 0;   // slots the rank must have before k_dist_apply runs
    size_t want_f = 0, want_v = 0;   // slot space to re-allocate to (= the current one when it suffices)
};
static int plan_migration(const uint32_t* hdr_left, const uint32_t* hdr_right, size_t capacity, size_t scene_f, size_t scene_v,
                          size_t held_f, size_t held_v, size_t slots_f, size_t slots_v, float headroom, MigrationPlan* out) {
    REQUIRE(capacity > 0 && capacity < ((size_t)1 << 28), "migration: bad buffer capacity");
    REQUIRE(scene_f + scene_v < ((size_t)1 << 30), "migration: bad scene size");
    if (held_f > slots_f || held_v > slots_v || slots_f > scene_f || slots_v > scene_v)
        return fail(MPM_ERR_INTERNAL, "migration: the rank's own counts are inconsistent (holds " + std::to_string(held_f) + " + " +
                                          std::to_string(held_v) + " particles in " + std::to_string(slots_f) + " + " +
                                          std::to_string(slots_v) + " slots of a scene of " + std::to_string(scene_f) + " + " +
                                          std::to_string(scene_v) + ")");
    MigrationPlan m;
    const uint32_t* hdrs[2] = {hdr_left, hdr_right};
    for (int k = 0; k < 2; ++k) {
        const uint32_t* h = hdrs[k];
        if (!h) continue;
        const char* side = k ? "right" : "left";
        // (a sender whose buffer overflowed keeps counting: it raises MPM_ERR_CAPACITY on its side, and the records
        // beyond the capacity were never written -- applying the rest would lose particles silently)
        if (h[0] > capacity)
            return fail(MPM_ERR_CAPACITY, std::string("migration: the ") + side + " neighbour packed " + std::to_string(h[0]) +
                                              " records into buffers of " + std::to_string(capacity) +
                                              " (mpm_chain_enable_migration / DomainChain: raise capacity_particles)");
        if (h[1] > h[0] || h[2] != 0 || h[3] != 0)
            return fail(MPM_ERR_INVALID, std::string("migration: corrupt header from the ") + side + " neighbour (" +
                                             std::to_string(h[0]) + " records, " + std::to_string(h[1]) + " faces, " +
                                             std::to_string(h[2]) + ", " + std::to_string(h[3]) + ")");
        m.in_f += h[1];
        m.in_v += h[0] - h[1];
    }
    // (every arriving record counted as a new particle -- promotions of ghosts the rank already holds need no slot --,
    // but never more than the scene has: a particle has one slot)
    m.need_f = std::min(scene_f, held_f + m.in_f);
    m.need_v = std::min(scene_v, held_v + m.in_v);
    m.want_f = slots_f;
    m.want_v = slots_v;
    if (m.need_f > slots_f || m.need_v > slots_v) {
        m.want_f = std::max(slots_f, dist_slot_capacity(headroom, m.need_f, scene_f));
        m.want_v = std::max(slots_v, dist_slot_capacity(headroom, m.need_v, scene_v));
    }
    *out = m;
    return 0;
}

static int dist_migrate_apply(mpm_engine* e, const void* recv_left, const void* recv_right, size_t capacity_particles) {
    // A migration is a synchronisation point: the host reads how many particles arrive and what the rank holds, and
    // re-allocates the slot space first if they would not fit (a cloth that slides across a cut, an uneven split).
    {
        DP& p = e->dp;
        uint32_t hdr[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
        // (pinned landing places are not needed: the copies are followed by a synchronisation at once)
        Ctl c;
        HIP_TRY(hipMemcpyAsync(&c, p.ctl, sizeof(Ctl), hipMemcpyDeviceToHost, e->stream));
        const void* bufs[2] = {recv_left, recv_right};
        for (int k = 0; k < 2; ++k)
            if (bufs[k]) HIP_TRY(hipMemcpyAsync(hdr[k], bufs[k], 16, hipMemcpyDeviceToHost, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        REQUIRE(c.nfa >= 0 && c.nva >= 0 && c.add_f >= 0 && c.add_v >= 0, "migration: corrupt control block");
        MigrationPlan m;
        if (int rc = plan_migration(recv_left ? hdr[0] : nullptr, recv_right ? hdr[1] : nullptr, capacity_particles, e->nf, e->nv,
                                    (size_t)c.nfa + (size_t)c.add_f, (size_t)c.nva + (size_t)c.add_v, (size_t)p.Nf, (size_t)p.Nv,
                                    e->dist_headroom, &m))
            return rc;
        if (m.want_f != (size_t)p.Nf || m.want_v != (size_t)p.Nv)
            if (int rc = dist_resize(e, m.want_f, m.want_v, false)) return rc;
    }
    for (const void* b : {recv_left, recv_right})
        if (b)
            hipLaunchKernelGGL(k_dist_apply, dim3(256), dim3(256), 0, e->stream, e->dp, static_cast<const float4*>(b),
                               (unsigned)capacity_particles);
    return 0;
}

static int dist_roles(mpm_engine* e, uint8_t* out) {
    if (int rc = e->stage(e->np)) return rc;
    hipLaunchKernelGGL(k_dist_roles, dim3(e->g_np), dim3(256), 0, e->stream, e->dp, (const int*)e->d_pids_api,
                       (unsigned char*)e->d_stage);
    HIP_TRY(hipMemcpyAsync(out, e->d_stage, e->np, hipMemcpyDeviceToHost, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return 0;
}
