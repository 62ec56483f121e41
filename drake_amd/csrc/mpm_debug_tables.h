// Test-only views of what no public array shows: the tables of the last conditional re-sort (mpm_rebuild.h) and the
// radix sort of mpm_sort.h on caller-made pairs.  Host code around existing kernels plus copies; no kernel of its own.
#pragma once
#include <cstring>
#include <vector>

#include "mpm_host.h"
#include "mpm_sort.h"

// mpm_debug_resort_tables: every table is an array of 4-byte words (int4 / int2 records flattened)
static int debug_resort_table(mpm_engine* e, int which, void* out, size_t capacity_bytes, size_t* count_out) {
    const DP& p = e->dp;
    HIP_TRY(hipStreamSynchronize(e->stream));
    Ctl c;
    D2H(e, &c, p.ctl, sizeof(Ctl));
    auto give = [&](const void* host, size_t words) -> int {
        if (count_out) *count_out = words;
        REQUIRE(capacity_bytes >= words * 4, "output buffer too small");
        if (words) std::memcpy(out, host, words * 4);
        return 0;
    };
    auto copy = [&](const void* dev, size_t words) -> int {
        if (count_out) *count_out = words;
        REQUIRE(capacity_bytes >= words * 4, "output buffer too small");
        if (words) D2H(e, out, dev, words * 4);
        return 0;
    };
    auto bits_of = [](float f) {
        int32_t v;
        std::memcpy(&v, &f, 4);
        return v;
    };
    const size_t np = (size_t)p.Np, nh = c.n_home, na = c.n_active, ni = c.n_items;
    switch (which) {
        case MPM_RT_CTL: {
            const int32_t rec[14] = {c.cur, c.need_rebuild, (int32_t)c.rebuilds, c.nfa, c.nva, c.add_f, c.add_v,
                                     (int32_t)c.n_home, (int32_t)c.n_active, (int32_t)c.n_items, (int32_t)c.n_items_wanted,
                                     (int32_t)c.error, bits_of(c.quiet_time), (int32_t)c.ticket};
            return give(rec, 14);
        }
        case MPM_RT_PARAMS: {
            const int32_t rec[16] = {p.Nf, p.Np, p.bits, p.nb, (int32_t)p.nblocks, (int32_t)p.capH, (int32_t)p.capA,
                                     (int32_t)p.capI, (int32_t)p.capS, p.item_groups, p.item_groups_small, p.item_small_below,
                                     bits_of(e->anticipation()),   // (as launch_rebuild sets DP::anticip)
                                     p.fem_fast, p.dist.on, p.NpG};
            return give(rec, 16);
        }
        case MPM_RT_PKEY: return copy(p.pkey, np);
        case MPM_RT_PRANK: return copy(p.prank, np);
        case MPM_RT_SRC_OF: return copy(p.src_of, np);
        case MPM_RT_DST_OF: return copy(p.dst_of, np);
        case MPM_RT_IMAP: return copy(p.imap, (size_t)p.NpG);
        case MPM_RT_PID: return copy(p.set[c.cur & 1].pid, np);
        case MPM_RT_HOME_BLOCK: return copy(p.home_block, nh);
        case MPM_RT_HOME_RANGE: return copy(p.home_range, nh * 4);
        case MPM_RT_HOME_ITEMS: return copy(p.home_items, nh * 2);
        case MPM_RT_HOME_NGROUPS: return copy(p.home_ngroups, nh);
        case MPM_RT_HOME_GROUPS: return copy(p.home_groups, (np / 64 + p.capH + 2) * 4);
        case MPM_RT_HOME_NBR_ACT: return copy(p.home_nbr_act, nh * 27);
        case MPM_RT_ACT_BLOCK: return copy(p.act_block, na);
        case MPM_RT_ACT_NBR_HOME: return copy(p.act_nbr_home, na * 27);
        case MPM_RT_ACT_NBR_ITEMS: return copy(p.act_nbr_items, na * 27);
        case MPM_RT_LUT_HOME: return copy(p.lut_home, p.nblocks);
        case MPM_RT_LUT_ACT: return copy(p.lut_act, p.nblocks);
        case MPM_RT_ITEM_DESC: return copy(p.item_desc, ni * 4);
        case MPM_RT_ITEM_ORDER: return copy(p.item_order, ni);
        case MPM_RT_ITEM_POS: return copy(p.item_pos, ni);
        case MPM_RT_ITEM_FLAT: return copy(p.item_flat, ni * 8);
        case MPM_RT_ITEM_RNG: return copy(p.item_rng, ni * 4);
        case MPM_RT_BLKSTART0: return copy(p.blkstart[0], p.nblocks);
        case MPM_RT_BLKSTART1: return copy(p.blkstart[1], p.nblocks);
        case MPM_RT_BLKCNT0: return copy(p.blkcnt[0], p.nblocks);
        case MPM_RT_BLKCNT1: return copy(p.blkcnt[1], p.nblocks);
        case MPM_RT_CELLCNT0: return copy(p.cellcnt[0], p.ncells);
        case MPM_RT_CELLCNT1: return copy(p.cellcnt[1], p.ncells);
        case MPM_RT_HOME_BITS: return copy(p.home_bits, (size_t)p.nblocks / 32 + 1);
        case MPM_RT_TICKETS: return copy(p.tickets, 32 * 32);
        case MPM_RT_FACE_REFS: return copy(p.set[c.cur & 1].fq[3], (size_t)p.Nf * 4);
        default: return fail(MPM_ERR_INVALID, "unknown re-sort table id");
    }
}

// mpm_debug_sort_pairs: radix_sort_pairs on buffers of exactly n pairs, both pairs downloaded in full
static int debug_sort_pairs(mpm_engine* e, const uint32_t* keys, const uint32_t* vals, size_t n, int bits, int device_count,
                            int want_in_place, uint32_t* keys_out, uint32_t* vals_out, int info_out[4]) {
    REQUIRE(n > 0 && n < ((size_t)1 << 30), "pair count out of range");
    REQUIRE(bits >= 0 && bits <= 32, "key bits out of range");
    REQUIRE(device_count < 0 || (size_t)device_count <= n, "device count above the launch bound");
    REQUIRE(keys && vals && keys_out && vals_out && info_out, "null pointer");
    HIP_TRY(hipStreamSynchronize(e->stream));
    uint32_t* buf[4] = {nullptr, nullptr, nullptr, nullptr};   // keys a, vals a, keys b, vals b
    int *hist = nullptr, *n_dev = nullptr;
    auto body = [&]() -> int {
        static const int fill[4] = {0xA5, 0x5A, 0xB6, 0x6B};
        for (int k = 0; k < 4; ++k) {
            HIP_TRY(hipMalloc((void**)&buf[k], n * 4));
            HIP_TRY(hipMemsetAsync(buf[k], fill[k], n * 4, e->stream));
        }
        HIP_TRY(hipMalloc((void**)&hist, sort_hist_ints_upto(n) * sizeof(int)));
        const size_t used = device_count >= 0 ? (size_t)device_count : n;
        if (used) {
            H2D(e, buf[0], keys, used * 4);
            H2D(e, buf[1], vals, used * 4);
        }
        if (device_count >= 0) {
            HIP_TRY(hipMalloc((void**)&n_dev, sizeof(int)));
            H2D(e, n_dev, &device_count, sizeof(int));
        }
        bool in_b = false;
        if (radix_sort_pairs(e->stream, buf[0], buf[1], buf[2], buf[3], hist, n, bits, want_in_place ? nullptr : &in_b, n_dev))
            return fail(MPM_ERR_HIP, "radix_sort_pairs failed");
        HIP_TRY(hipGetLastError());
        for (int k = 0; k < 4; ++k) D2H(e, ((k & 1) ? vals_out : keys_out) + (k >> 1) * n, buf[k], n * 4);
        const bool ran = n >= 2 && bits > 0;
        const SortPlan pl = sort_plan(n, bits);
        info_out[0] = ran ? pl.digit_bits : 0;
        info_out[1] = ran ? pl.passes : 0;
        info_out[2] = ran ? pl.ntiles : 0;
        info_out[3] = in_b ? 1 : 0;
        return 0;
    };
    const int rc = body();
    (void)hipStreamSynchronize(e->stream);
    for (int k = 0; k < 4; ++k)
        if (buf[k]) (void)hipFree(buf[k]);
    if (hist) (void)hipFree(hist);
    if (n_dev) (void)hipFree(n_dev);
    return rc;
}
