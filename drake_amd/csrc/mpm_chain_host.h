// Host side of the native chain (mpm_chain_*), of its direct halo (mpm_chain_direct_*) and of the team transport's
// set-up (mpm_team_prepare, mpm_team_connect): what the entry points in mpm_engine.hip call once their arguments are
// checked.  Included by mpm_engine.hip after mpm_host.h, mpm_chain.h and mpm_dist.h.
#pragma once
#include "mpm_chain.h"
#include "mpm_host.h"

// the halo substeps of mpm_engine.hip that a chain substep is made of
static int substep_begin_halo(mpm_handle_t e, float dt, int n, const int* bx_lo, const int* bx_hi, const int* shift_bx,
                              void* const* send_bufs, size_t cap, uint32_t* const* counters, bool lean);
static int substep_end_halo(mpm_handle_t e, float dt, int bc, int n, const void* const* recv_bufs, size_t cap, bool with_g2p,
                            bool lean);

// ---- the chain over RCCL (mpm_chain_unique_id, mpm_chain_init, mpm_chain_destroy, mpm_chain_enable_migration) -----------
// RCCL's id of a new communicator: one rank makes it, all ranks hand it to mpm_chain_init
static int chain_unique_id(char id_out[128]) {
    const rccl_rt::Api* a = rccl_rt::api();
    if (!a) return fail(MPM_ERR_HIP, "RCCL (librccl.so) is not available in this process");
    rccl_rt::UniqueId id;
    RCCL_TRY(a->get_unique_id(&id));
    std::memcpy(id_out, id.internal, rccl_rt::kIdBytes);
    return 0;
}

// the neighbours' regions of the direct halo, unmapped (a ring of two maps one region for both sides)
static void chain_unmap_peers(mpm_engine::Chain& c) {
    for (int k = 0; k < 2; ++k)
        if (c.peer_mapped[k] && c.peer_base[k] && !(k == 1 && c.peer_base[1] == c.peer_base[0])) (void)hipIpcCloseMemHandle(c.peer_base[k]);
    c.peer_mapped[0] = c.peer_mapped[1] = false;
    c.peer_base[0] = c.peer_base[1] = nullptr;
}

// everything mpm_chain_* and mpm_team_* hold: communicator, buffers, mapped regions (also mpm_destroy and chain_init)
static int chain_destroy(mpm_engine* e) {
    mpm_engine::Chain& c = e->chain;
    if (int rc = use(e)) return rc;
    (void)hipStreamSynchronize(e->stream);
    if (c.comm) {   // (RCCL is only looked up by engines that use it)
        const rccl_rt::Api* a = rccl_rt::api();
        if (a) (void)a->comm_destroy(c.comm);
    }
    for (void* q : {c.send_l, c.send_r, c.recv_l, c.recv_r, c.mig_send_l, c.mig_send_r, c.mig_recv_l, c.mig_recv_r,
                    (void*)c.mig_quiet_all})
        if (q) (void)hipFree(q);
    chain_unmap_peers(c);
    if (c.direct_base) (void)hipFree(c.direct_base);
    if (c.direct_cnt) (void)hipFree(c.direct_cnt);
    c = mpm_engine::Chain();
    {
        mpm_engine::Team& t = e->team;
        for (int r = 0; r < TEAM_MAX; ++r)
            if (t.mapped[r] && t.peer[r]) (void)hipIpcCloseMemHandle(t.peer[r]);
        if (t.base) (void)hipFree(t.base);
        if (t.ts) (void)hipFree(t.ts);
        t = mpm_engine::Team();
    }
    return 0;
}

// the migration buffers of a partitioned domain's chain and its cadence (every = 0: adaptive, see chain_substeps)
static int chain_enable_migration(mpm_engine* e, int every, size_t capacity_particles) {
    mpm_engine::Chain& c = e->chain;
    REQUIRE(c.comm, "mpm_chain_init first");
    REQUIRE(e->dp.dist.on, "mpm_dist_init first");
    REQUIRE(c.pitch == 0 && c.rank == e->dp.dist.rank && c.world == e->dp.dist.world,
            "the chain of a partitioned domain has pitch 0 and the rank / world given to mpm_dist_init");
    REQUIRE(every >= 0 && capacity_particles > 0 && capacity_particles < (1u << 28), "bad migration parameters");
    REQUIRE(every > 0 || rccl_rt::api()->all_reduce, "adaptive migration (every = 0) needs ncclAllReduce");
    for (void** q : {&c.mig_send_l, &c.mig_send_r, &c.mig_recv_l, &c.mig_recv_r, (void**)&c.mig_quiet_all}) {
        if (*q) (void)hipFree(*q);
        *q = nullptr;
    }
    HIP_TRY(hipMalloc((void**)&c.mig_quiet_all, 16));
    c.mig_budget = 0.f;    // (the first substep starts with a migration: it yields the first estimate)
    c.mig_elapsed = 0.f;
    c.mig_every = every;
    c.mig_cap = capacity_particles;
    c.mig_bytes = mpm_dist_migration_buffer_bytes(capacity_particles);
    for (void** q : {&c.mig_send_l, &c.mig_send_r, &c.mig_recv_l, &c.mig_recv_r}) {
        HIP_TRY(hipMalloc(q, c.mig_bytes));
        HIP_TRY(hipMemsetAsync(*q, 0, c.mig_bytes, e->stream));
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    return 0;
}

// a rank's place in the chain: neighbours, the zones around its two cuts, send / receive buffers, the communicator
static int chain_init(mpm_engine* e, const char id[128], int rank, int world, int cut_lo_block, int cut_hi_block,
                      int pitch_blocks, int zone_blocks, size_t capacity_blocks, int periodic) {
    // (id == NULL: the geometry only, no RCCL communicator -- for the direct transport, mpm_chain_direct_prepare)
    const rccl_rt::Api* a = id ? rccl_rt::api() : nullptr;
    if (id && !a) return fail(MPM_ERR_HIP, "RCCL (librccl.so) is not available in this process");
    if (int rc = mpm_chain_destroy(e)) return rc;
    mpm_engine::Chain& c = e->chain;
    c.rank = rank; c.world = world; c.pitch = pitch_blocks; c.cap = capacity_blocks;
    c.left = rank > 0 ? rank - 1 : (periodic ? world - 1 : -1);
    c.right = rank < world - 1 ? rank + 1 : (periodic ? 0 : -1);
    c.zone_lo[0] = cut_lo_block - zone_blocks; c.zone_hi[0] = cut_lo_block + zone_blocks - 1;
    c.zone_lo[1] = cut_hi_block - zone_blocks; c.zone_hi[1] = cut_hi_block + zone_blocks - 1;
    c.bytes = mpm_halo_buffer_bytes(capacity_blocks);
    for (void** q : {&c.send_l, &c.send_r, &c.recv_l, &c.recv_r}) {
        HIP_TRY(hipMalloc(q, c.bytes));
        HIP_TRY(hipMemsetAsync(*q, 0, c.bytes, e->stream));
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (id) {
        rccl_rt::UniqueId uid;
        std::memcpy(uid.internal, id, rccl_rt::kIdBytes);
        RCCL_TRY(a->comm_init_rank(&c.comm, world, uid, rank));
    }
    return 0;
}

// ---- direct halo: peer-to-peer stores + sequence flags -------------------------------------------
static size_t direct_slot_bytes(const mpm_engine::Chain& c) { return (c.bytes + 255) & ~(size_t)255; }
static size_t direct_total_bytes(const mpm_engine::Chain& c) { return 4 * direct_slot_bytes(c) + 256; }
// [side 0 = from the left neighbour, 1 = from the right][parity] inside an allocation laid out as above
static void* direct_buffer(const mpm_engine::Chain& c, void* base, int side, int parity) {
    return (char*)base + (size_t)(side * 2 + parity) * direct_slot_bytes(c);
}
static uint32_t* direct_flag(const mpm_engine::Chain& c, void* base, int side) {
    return reinterpret_cast<uint32_t*>((char*)base + 4 * direct_slot_bytes(c)) + side * 16;   // (64 bytes apart)
}

// this rank's region (made at the first call) and its IPC handle for the neighbours
static int chain_direct_prepare(mpm_engine* e, char handle_out[64]) {
    mpm_engine::Chain& c = e->chain;
    REQUIRE(handle_out, "null argument");
    REQUIRE(c.cap > 0, "mpm_chain_init first (with a NULL id for the geometry alone)");
    static_assert(sizeof(hipIpcMemHandle_t) == 64, "IPC handle size");
    if (!c.direct_base) {
        const size_t bytes = direct_total_bytes(c);
        // FINE-GRAINED, or not at all: the protocol's consumer (k_grid<2>) reads the count, the ids and the sums with plain
        // loads and relies on a peer's stores not being shadowed by stale lines of this device's L2.  A coarse-grained
        // region would add stale halo sums without any error flag, so a refused allocation is an error of
        // this call -- the caller stays on RCCL (the connect protocol allows that: mpm_chain_direct_connect(NULL, NULL)).
        // MPM_DIRECT_COARSE_OK=1 accepts plain device memory for rehearsals on ONE device, where both ends share the L2.
        const hipError_t fg = hipExtMallocWithFlags(&c.direct_base, bytes, hipDeviceMallocFinegrained);
        if (fg != hipSuccess) {
            (void)hipGetLastError();
            c.direct_base = nullptr;
            if (!getenv("MPM_DIRECT_COARSE_OK"))
                return fail(MPM_ERR_HIP, std::string("mpm_chain_direct_prepare: fine-grained device memory is not available (") +
                                             hipGetErrorString(fg) + "): the direct halo exchange needs it; stay on the RCCL transport");
            HIP_TRY(hipMalloc(&c.direct_base, bytes));
        }
        HIP_TRY(hipMemsetAsync(c.direct_base, 0, bytes, e->stream));
        if (!c.direct_cnt) {
            HIP_TRY(hipMalloc((void**)&c.direct_cnt, 64));
            HIP_TRY(hipMemsetAsync(c.direct_cnt, 0, 64, e->stream));
        }
        HIP_TRY(hipStreamSynchronize(e->stream));
    }
    hipIpcMemHandle_t h;
    HIP_TRY(hipIpcGetMemHandle(&h, c.direct_base));
    std::memcpy(handle_out, &h, 64);
    if (const char* t = getenv("MPM_HALO_TIMEOUT_S")) c.direct_timeout_s = std::max(.001f, (float)atof(t));
    c.direct_mute = getenv("MPM_HALO_DEBUG_MUTE") != nullptr;   // (tests: this rank never signals)
    return 0;
}

// the neighbours' regions mapped through their IPC handles (both NULL: the direct transport switched off again)
static int chain_direct_connect(mpm_engine* e, const char left_handle[64], const char right_handle[64]) {
    mpm_engine::Chain& c = e->chain;
    REQUIRE(c.direct_base, "mpm_chain_direct_prepare first");
    const char* hs[2] = {left_handle, right_handle};
    const int nbr[2] = {c.left, c.right};
    chain_unmap_peers(c);
    const bool foreign = (c.left >= 0 && c.left != c.rank) || (c.right >= 0 && c.right != c.rank);
    if (foreign && !left_handle && !right_handle) {   // switched off again: the chain is RCCL's (or nobody's) once more
        c.direct = false;
        return 0;
    }
    for (int k = 0; k < 2; ++k) {
        if (nbr[k] < 0) continue;
        if (nbr[k] == c.rank) {   // a ring of one: the neighbour is this rank, no mapping
            c.peer_base[k] = c.direct_base;
            continue;
        }
        REQUIRE(hs[k], "missing IPC handle of a neighbour");
        if (k == 1 && c.left == c.right && c.peer_base[0]) {   // a ring of two: both neighbours are the same rank
            c.peer_base[1] = c.peer_base[0];
            c.peer_mapped[1] = c.peer_mapped[0];
            continue;
        }
        hipIpcMemHandle_t h;
        std::memcpy(&h, hs[k], 64);
        const hipError_t err = hipIpcOpenMemHandle(&c.peer_base[k], h, hipIpcMemLazyEnablePeerAccess);
        if (err != hipSuccess) {
            (void)hipGetLastError();   // (not sticky: the engine stays usable, with RCCL or without neighbours)
            c.peer_base[k] = nullptr;
            return fail(MPM_ERR_HIP, std::string("hipIpcOpenMemHandle: ") + hipGetErrorString(err) +
                                         " (the neighbour's buffers cannot be mapped: another node, or a handle of this very process)");
        }
        c.peer_mapped[k] = true;
    }
    c.direct = true;
    return 0;
}

// ... of neighbours in this process, named by pointer (mpm_chain_direct_base)
static int chain_direct_connect_local(mpm_engine* e, void* left_base, void* right_base) {
    mpm_engine::Chain& c = e->chain;
    REQUIRE(c.direct_base, "mpm_chain_direct_prepare first");
    REQUIRE((c.left < 0 || left_base) && (c.right < 0 || right_base), "missing region of a neighbour");
    chain_unmap_peers(c);
    c.peer_base[0] = c.left >= 0 ? left_base : nullptr;
    c.peer_base[1] = c.right >= 0 ? right_base : nullptr;
    c.direct = true;
    return 0;
}

// ---- TEAM transport of the distributed contact solve (mpm_team.h) --------------------------------------------------------
// this rank's region and exchange counters (made at the first call), its IPC handle and / or its pointer
static int team_prepare(mpm_engine* e, size_t zone_capacity_blocks, char handle_out[64], void** base_out) {
    mpm_engine::Team& t = e->team;
    REQUIRE(!t.on, "mpm_team_prepare after mpm_team_connect");
    if (!t.base) {
        t.rank = e->dp.dist.rank;
        t.world = e->dp.dist.world;
        t.zone_cap = zone_capacity_blocks;
        t.zone_bytes = team_zone_slot_bytes(zone_capacity_blocks);
        const size_t bytes = team_region_bytes(t.zone_bytes);
        // fine-grained or not at all, as for the direct halo (mpm_chain_direct_prepare)
        const hipError_t fg = hipExtMallocWithFlags(&t.base, bytes, hipDeviceMallocFinegrained);
        if (fg != hipSuccess) {
            (void)hipGetLastError();
            t.base = nullptr;
            if (!getenv("MPM_DIRECT_COARSE_OK"))
                return fail(MPM_ERR_HIP, std::string("mpm_team_prepare: fine-grained device memory is not available (") + hipGetErrorString(fg) +
                                             "): the team transport needs it; the solve stays on the host-driven transports");
            HIP_TRY(hipMalloc(&t.base, bytes));
        }
        HIP_TRY(hipMemsetAsync(t.base, 0, bytes, e->stream));
        HIP_TRY(hipMalloc((void**)&t.ts, sizeof(TeamState)));
        HIP_TRY(hipMemsetAsync(t.ts, 0, sizeof(TeamState), e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        if (const char* s2 = getenv("MPM_HALO_TIMEOUT_S")) t.timeout_s = std::max(.001f, (float)atof(s2));
    }
    if (handle_out) {
        hipIpcMemHandle_t h;
        HIP_TRY(hipIpcGetMemHandle(&h, t.base));
        std::memcpy(handle_out, &h, 64);
    }
    if (base_out) *base_out = t.base;
    return 0;
}

// every other rank's region, by pointer (a rank of this process) or mapped through its handle; switches the team on
static int team_connect(mpm_engine* e, const char* handles, void* const* local_bases) {
    mpm_engine::Team& t = e->team;
    REQUIRE(t.base, "mpm_team_prepare first");
    for (int r = 0; r < t.world; ++r) {
        if (r == t.rank) {
            t.peer[r] = t.base;
            continue;
        }
        if (t.mapped[r] && t.peer[r]) (void)hipIpcCloseMemHandle(t.peer[r]);
        t.mapped[r] = false;
        t.peer[r] = nullptr;
        if (local_bases && local_bases[r]) {
            t.peer[r] = local_bases[r];
            continue;
        }
        REQUIRE(handles, "missing IPC handle of a rank");
        hipIpcMemHandle_t h;
        std::memcpy(&h, handles + (size_t)r * 64, 64);
        const hipError_t err = hipIpcOpenMemHandle(&t.peer[r], h, hipIpcMemLazyEnablePeerAccess);
        if (err != hipSuccess) {
            (void)hipGetLastError();
            t.peer[r] = nullptr;
            return fail(MPM_ERR_HIP, std::string("mpm_team_connect: hipIpcOpenMemHandle: ") + hipGetErrorString(err) +
                                         " (a rank's region cannot be mapped: another node, or a handle of this very process)");
        }
        t.mapped[r] = true;
    }
    t.on = true;
    return 0;
}

// The two halves of a chain substep over the DIRECT transport (see mpm_chain_substeps): begin = re-sort checks, FEM,
// ParticleToGrid, raw sums packed into the neighbours' slots of this substep's parity, signal; end = wait, add + grid
// update (+ GridToParticle).  Between them a coupled substep runs nothing that touches the grid.
static int chain_zones(const mpm_engine::Chain& c, int* lo, int* hi, int* sh) {
    int nz = 0;
    if (c.left >= 0) { lo[nz] = c.zone_lo[0]; hi[nz] = c.zone_hi[0]; sh[nz] = +c.pitch; ++nz; }
    if (c.right >= 0) { lo[nz] = c.zone_lo[1]; hi[nz] = c.zone_hi[1]; sh[nz] = -c.pitch; ++nz; }
    return nz;
}
// ... and a (left, right) pair of buffers in the same order
static void chain_sides(const mpm_engine::Chain& c, void* left, void* right, void** out) {
    int k = 0;
    if (c.left >= 0) out[k++] = left;
    if (c.right >= 0) out[k++] = right;
}
// One RCCL group with both neighbours: out_l / out_r bytes from send_l / send_r, in_l / in_r bytes into recv_l / recv_r (a
// size of 0 leaves the call out).  What goes to the left arrives "from the right" over there: when both neighbours are the
// same rank (a ring of one or two) the k-th send pairs with the k-th receive, so the receives are posted right-then-left
// against sends left-then-right.
static int chain_exchange(mpm_engine* e, const rccl_rt::Api* a, void* send_l, size_t out_l, void* send_r, size_t out_r, void* recv_l,
                          size_t in_l, void* recv_r, size_t in_r) {
    const mpm_engine::Chain& c = e->chain;
    RCCL_TRY(a->group_start());
    int rc_g = 0;
    if (!rc_g && c.left >= 0 && out_l) rc_g = a->send(send_l, out_l, 0 /* ncclChar */, c.left, c.comm, e->stream);
    if (!rc_g && c.right >= 0 && out_r) rc_g = a->send(send_r, out_r, 0, c.right, c.comm, e->stream);
    if (!rc_g && c.right >= 0 && in_r) rc_g = a->recv(recv_r, in_r, 0, c.right, c.comm, e->stream);
    if (!rc_g && c.left >= 0 && in_l) rc_g = a->recv(recv_l, in_l, 0, c.left, c.comm, e->stream);
    const int rc_e = a->group_end();   // (always closes the group, also after a failed call)
    RCCL_TRY(rc_g);
    RCCL_TRY(rc_e);
    return 0;
}
// lean: another substep of the same batch follows (see substep_begin_halo)
static int chain_direct_begin(mpm_engine* e, float dt, bool lean) {
    mpm_engine::Chain& c = e->chain;
    REQUIRE(c.direct, "mpm_chain_direct_connect first");
    int lo[2], hi[2], sh[2];
    const int nz = chain_zones(c, lo, hi, sh);
    c.mig_elapsed += dt;
    c.steps += 1;
    const int parity = (int)(c.steps & 1u);
    const uint32_t seq = (uint32_t)c.steps;
    void* dsb[2] = {nullptr, nullptr};
    uint32_t *sig[2] = {nullptr, nullptr}, *cnt[2] = {nullptr, nullptr}, *hdr[2] = {nullptr, nullptr}, *counters[2] = {nullptr, nullptr};
    int k = 0;
    if (c.left >= 0) {   // my left zone goes to the left neighbour's "from the right" buffer
        dsb[k] = direct_buffer(c, c.peer_base[0], 1, parity);
        sig[0] = direct_flag(c, c.peer_base[0], 1);
        cnt[0] = c.direct_cnt; hdr[0] = static_cast<uint32_t*>(dsb[k]);
        counters[k] = cnt[0];
        ++k;
    }
    if (c.right >= 0) {
        dsb[k] = direct_buffer(c, c.peer_base[1], 0, parity);
        sig[1] = direct_flag(c, c.peer_base[1], 0);
        cnt[1] = c.direct_cnt + 8; hdr[1] = static_cast<uint32_t*>(dsb[k]);
        counters[k] = cnt[1];
        ++k;
    }
    if (int rc = substep_begin_halo(e, dt, nz, lo, hi, sh, dsb, c.cap, counters, lean)) return rc;
    if (!c.direct_mute && nz > 0)
        hipLaunchKernelGGL(k_halo_signal, dim3(1), dim3(64), 0, e->stream, sig[0], sig[1], seq, (const uint32_t*)cnt[0], hdr[0],
                           (const uint32_t*)cnt[1], hdr[1], (unsigned)c.cap);
    return 0;
}
static int chain_direct_end(mpm_engine* e, float dt, int bc, bool with_g2p, bool lean) {
    mpm_engine::Chain& c = e->chain;
    int lo[2], hi[2], sh[2];
    const int nz = chain_zones(c, lo, hi, sh);
    const int parity = (int)(c.steps & 1u);
    const uint32_t seq = (uint32_t)c.steps;
    void* drb[2] = {nullptr, nullptr};
    uint32_t* mine[2] = {nullptr, nullptr};
    int k = 0;
    if (c.left >= 0) { drb[k++] = direct_buffer(c, c.direct_base, 0, parity); mine[0] = direct_flag(c, c.direct_base, 0); }
    if (c.right >= 0) { drb[k++] = direct_buffer(c, c.direct_base, 1, parity); mine[1] = direct_flag(c, c.direct_base, 1); }
    if (nz > 0)
        hipLaunchKernelGGL(k_halo_wait, dim3(1), dim3(64), 0, e->stream, (const uint32_t*)mine[0], (const uint32_t*)mine[1], seq,
                           (unsigned long long)((double)c.direct_timeout_s * 1e8), e->dp.ctl);
    return substep_end_halo(e, dt, bc, nz, drb, c.cap, with_g2p, lean);
}

// mpm_chain_substeps: n contact-free substeps of this rank, each with its halo exchange (direct or RCCL), and the
// migrations that fall due between them
static int chain_substeps(mpm_engine* e, int n, float dt, int bc) {
    mpm_engine::Chain& c = e->chain;
    REQUIRE(c.comm || c.direct, "mpm_chain_init first");
    const rccl_rt::Api* a = c.comm ? rccl_rt::api() : nullptr;
    REQUIRE(c.comm || c.mig_cap == 0, "migration needs the RCCL communicator (mpm_chain_init with an id)");
    // zones / buffers in the order (left, right), leaving out a missing neighbour
    int lo[2], hi[2], sh[2];
    const int nz = chain_zones(c, lo, hi, sh);
    void *sb[2], *rb[2];
    chain_sides(c, c.send_l, c.send_r, sb);
    chain_sides(c, c.recv_l, c.recv_r, rb);
    for (int s = 0; s < n; ++s) {
        // Migration: every mig_every substeps, or (mig_every = 0, adaptive) when half of the time has passed in which,
        // by the ranks' common estimate, no particle can have drifted further than the bands allow (Dist::mig_delta).
        bool due = false;
        if (c.mig_cap > 0 && nz > 0) {
            if (c.mig_every > 0) due = c.steps > 0 && c.steps % (uint64_t)c.mig_every == 0;
            else due = !(c.mig_elapsed + dt <= c.mig_budget);
        }
        if (due) {
            // particles change hands (mpm_dist.h): records to / from both neighbours, same pairing as below.  In two
            // rounds: the 16-byte headers first (record counts), then exactly the records that exist -- a RCCL
            // send needs its size when it is enqueued, and the buffers are sized for the worst case (9 MB for 65536
            // records) while a migration of a cloth at rest moves none.  The host reads the counts in between; a
            // migration is a synchronisation point anyway (mpm_dist_migrate_apply).
            if (int rc = mpm_dist_migrate_pack(e, c.mig_send_l, c.mig_send_r, c.mig_cap)) return rc;
            auto exchange = [&](size_t out_l, size_t out_r, size_t in_l, size_t in_r, size_t offset) -> int {
                return chain_exchange(e, a, (char*)c.mig_send_l + offset, out_l, (char*)c.mig_send_r + offset, out_r,
                                      (char*)c.mig_recv_l + offset, in_l, (char*)c.mig_recv_r + offset, in_r);
            };
            if (int rc = exchange(16, 16, 16, 16, 0)) return rc;
            if (c.mig_every == 0) {
                // the ranks agree on the smallest estimate (one float, ncclMin), read back with the headers
                RCCL_TRY(a->all_reduce(&e->dp.ctl->mig_quiet, c.mig_quiet_all, 1, 7 /* ncclFloat32 */, 3 /* ncclMin */, c.comm,
                                       e->stream));
            }
            {
                uint32_t h[4][4] = {};
                void* bufs[4] = {c.mig_send_l, c.mig_send_r, c.mig_recv_l, c.mig_recv_r};
                for (int k = 0; k < 4; ++k) HIP_TRY(hipMemcpyAsync(h[k], bufs[k], 16, hipMemcpyDeviceToHost, e->stream));
                HIP_TRY(hipStreamSynchronize(e->stream));
                auto bytes = [&](int k, bool there) {
                    return there ? (size_t)std::min<size_t>(h[k][0], c.mig_cap) * DIST_REC_F4 * 16 : (size_t)0;
                };
                // (a ring of one or two ranks pairs the k-th send with the k-th receive: what goes left arrives "from the
                // right" over there -- the received headers say how much comes from each side)
                if (int rc = exchange(bytes(0, c.left >= 0), bytes(1, c.right >= 0), bytes(2, c.left >= 0), bytes(3, c.right >= 0), 16))
                    return rc;
            }
            if (int rc = mpm_dist_migrate_apply(e, c.left >= 0 ? c.mig_recv_l : nullptr, c.right >= 0 ? c.mig_recv_r : nullptr,
                                                c.mig_cap))
                return rc;
            if (c.mig_every == 0) {
                float t = 0.f;
                D2H(e, &t, c.mig_quiet_all, sizeof(float));   // (the stream is idle: apply has just synchronised it)
                // (the estimate is ballistic: forces can speed particles up before the next look.  The interval may at
                // most double from one migration to the next -- 4 substeps after the first --, so a change of the
                // velocities is seen after at most as long as they have been watched)
                const float t_est = e->mig_safety * (t >= 0.f ? t : 0.f);   // (NaN -> 0: migrate again next substep)
                c.mig_budget = std::min(t_est, std::max(4.f * dt, 2.f * c.mig_elapsed));
                c.mig_elapsed = 0.f;
                if (int rc = mpm_dist_retune(e, t, dt, nullptr)) return rc;   // (band widths for the migrations to come)
            }
        }
        const bool lean = s + 1 < n;
        if (c.direct && nz > 0) {
            // DIRECT: the pack kernel stores into the neighbours' receive buffers of this substep's parity (two in
            // rotation: a neighbour may still be reading the other one -- it cannot be reading this one: its read of
            // substep s - 2 precedes its signal of s - 1, which this rank's update of s - 1 has waited for), a one-thread
            // kernel raises the flags over there, a one-wave kernel waits for this rank's.
            if (int rc = chain_direct_begin(e, dt, lean)) return rc;
            if (int rc = chain_direct_end(e, dt, bc, true, lean)) return rc;
            continue;
        }
        c.mig_elapsed += dt;
        c.steps += 1;
        if (int rc = substep_begin_halo(e, dt, nz, lo, hi, sh, sb, c.cap, nullptr, lean)) return rc;
        if (nz > 0)
            if (int rc = chain_exchange(e, a, c.send_l, c.bytes, c.send_r, c.bytes, c.recv_l, c.bytes, c.recv_r, c.bytes)) return rc;
        if (int rc = substep_end_halo(e, dt, bc, nz, rb, c.cap, true, lean)) return rc;
    }
    HIP_TRY(hipGetLastError());
    return 0;
}
