// Zone exchange buffers: the one format in which ranks hand each other per-node data of the blocks next to a cut -- the
// grid sums of a chain substep (mpm_step.h, mpm_grid_update.inc; NV = 1) and the contact solve's (H, G) sums and node
// flags (mpm_contact_dev.h, mpm_team.h; NV = 3), on the RCCL, staged, direct and team transports alike -- and the flag
// protocol of the transports that store into a peer's memory.  Nothing outside this header knows either.
//
// Layout, in uint32 words:  [0] the number of blocks listed; [1..3] unused; [4 .. 4 + cap) their block ids, in the order
// the sender's atomics fell; then, from the next 16-byte boundary, cap * 64 * NV float4: block-major, cell, vector.
// Entries are only copied or added component-wise: there is no multiply here for the compiler to contract.
#pragma once
#include "mpm_device.h"

namespace mpm {

// ---- layout (host and device) -------------------------------------------------------------------------------------
__host__ __device__ inline size_t zbuf_ids_offset() { return 4; }                                             // uint32 units
__host__ __device__ inline size_t zbuf_data_offset(size_t cap) { return ((zbuf_ids_offset() + cap) * 4 + 15) / 16; }  // float4 units
__host__ __device__ inline size_t zone_buffer_bytes(size_t cap, int nv) { return (zbuf_data_offset(cap) + cap * 64 * nv) * 16; }

MPM_DEV const float4* zbuf_cell(const uint32_t* buf, unsigned cap, unsigned entry, int nv) {   // this lane's vectors of an entry
    return reinterpret_cast<const float4*>(buf) + zbuf_data_offset(cap) + ((size_t)entry * 64 + (threadIdx.x & 63)) * nv;
}

// up to two zones of a launch (blockIdx.y selects): x-block range [lo, hi], the shift into the receiver's block
// coordinates where the sender relabels, and the buffer packed into or added from
struct Zones {
    int lo[2], hi[2], shift[2];
    uint32_t* buf[2];
};

// ---- writer: one wave per block ---------------------------------------------------------------------------------------
// Claims the next entry for the wave: the wave-uniform slot, or -1 when the buffer is full (ERR_CAPACITY is raised).
// `counter` is word 0 of the buffer itself where the buffer lies in this device's memory (RCCL, staged transports).  The
// direct and team transports pack straight into the NEIGHBOUR's memory and count in a word of their own device -- a
// returning atomic on a peer's memory is not something every interconnect guarantees --; their signal kernel
// stores the final count into the neighbour's word 0 behind the pack's kernel boundary.
MPM_DEV int zbuf_claim(uint32_t* counter, unsigned cap, Ctl* ctl) {
    const bool lane0 = (threadIdx.x & 63) == 0;
    unsigned slot = 0;
    if (lane0) slot = atomicAdd(counter, 1u);
    slot = __builtin_amdgcn_readfirstlane(slot);
    if (slot >= cap) {
        if (lane0) atomicOr(&ctl->error, ERR_CAPACITY);
        return -1;
    }
    return (int)slot;
}
// lane 0 stores the id, every lane its cell's NV vectors
template <int NV>
MPM_DEV void zbuf_store(uint32_t* buf, unsigned cap, unsigned slot, uint32_t id, const float4* src) {
    if ((threadIdx.x & 63) == 0) buf[zbuf_ids_offset() + slot] = id;
    float4* dst = const_cast<float4*>(zbuf_cell(buf, cap, slot, NV));
#pragma unroll
    for (int v = 0; v < NV; ++v) dst[v] = src[v];
}

// ---- reader -----------------------------------------------------------------------------------------------------------
MPM_DEV unsigned zbuf_count(const uint32_t* buf, unsigned cap) { return min(buf[0], cap); }
// entry e -> this rank's active block, or why it is not ours: nothing of this rank reaches that block (FOREIGN), or the
// id is no block of this grid (BAD_ID: no sender writes such an id); *id_out: the block id as listed
constexpr int ZBUF_FOREIGN = -1, ZBUF_BAD_ID = -2;
MPM_DEV int zbuf_entry_block(const DP& p, const uint32_t* buf, unsigned e, uint32_t* id_out = nullptr) {
    const uint32_t id = buf[zbuf_ids_offset() + e];
    if (id_out) *id_out = id;
    if (id >= p.nblocks) return ZBUF_BAD_ID;
    const int a = p.lut_act[id];
    return a < 0 ? ZBUF_FOREIGN : a;
}
// adds this lane's NV vectors of entry e to those at dst
template <int NV>
MPM_DEV void zbuf_add(const uint32_t* buf, unsigned cap, unsigned e, float4* dst) {
    const float4* src = zbuf_cell(buf, cap, e, NV);
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        const float4 r = src[v];
        float4 q = dst[v];
        q.x += r.x; q.y += r.y; q.z += r.z; q.w += r.w;
        dst[v] = q;
    }
}
// the entry among the first n that lists block `id`, or -1 (wave-uniform): the wave scans the ids, 64 per step
MPM_DEV int zbuf_find(const uint32_t* buf, unsigned n, uint32_t id) {
    const unsigned lane = threadIdx.x & 63;
    for (unsigned base = 0; base < n; base += 64) {
        const uint32_t listed = base + lane < n ? buf[zbuf_ids_offset() + base + lane] : 0xFFFFFFFFu;
        const unsigned long long m = __ballot(listed == id);
        if (m) return (int)base + __builtin_ctzll(m);
    }
    return -1;
}

// ---- flags of the transports that store into a peer's memory ------------------------------------------------------------
// "My stores are complete, system-wide; now the flags": a system-scope fence, then a system-scope RELEASE store of `seq`
// into each of the n flags flag_of(i) (null: none).  For stores of other waves the caller runs behind their kernel
// boundary; the fence is the calling wave's and covers every lane's own stores.
template <class F>
MPM_DEV void publish_then_flag(int n, uint32_t seq, F flag_of) {
    __threadfence_system();
    // (MI355X_MICROARCH.md, "Compiler hazard": the wait behind the write-back may be dropped when the wave's vmcnt is
    // provably empty -- the flag could then overtake the data; an inline-asm wait is invisible to that pass)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    for (int i = 0; i < n; ++i)
        if (uint32_t* flag = flag_of(i)) __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
// Bounded wait for `flag >= seq` (sequence numbers only grow: signed difference), with system-scope ACQUIRE loads SLEEP
// apart: false once more than `timeout_ticks` of the 100 MHz wall clock have passed since t0, so that a peer that never
// arrives becomes an error code of the caller's, not a hung device.
template <int SLEEP>
MPM_DEV bool wait_flag(const uint32_t* flag, uint32_t seq, unsigned long long t0, unsigned long long timeout_ticks) {
    while (true) {
        if ((int)(__hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) - seq) >= 0) return true;
        if (wall_clock64() - t0 > timeout_ticks) return false;
        __builtin_amdgcn_s_sleep(SLEEP);
    }
}

}  // namespace mpm
