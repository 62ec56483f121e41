// The body of the grid kernels: k_grid<MODE> (mpm_step.h, MPM_GRID_BODIES 0) and k_grid_bodies<KINDS> (mpm_grid_bodies.h,
// MPM_GRID_BODIES 1, MODE == 1), which share the gather, the division and the walls and differ in what acts on a node
// afterwards: the table of spheres and half-spaces, or the rigid bodies of mpm_set_grid_bodies with their reaction.
    __shared__ int2 s_list[4][GRID_LIST];   // (item, offset index)
    const Ctl* ctl = p.ctl;
    {
        const bool out = gated_out(p);
        if (blockIdx.x == 0 && threadIdx.x == 0) p.ctl->skip_this = out;
        if (out) return;
    }
#if MPM_GRID_BODIES
    // the reaction on the bodies: pre-summed per workgroup here, one global add per body and component at the end
    __shared__ unsigned long long s_acc[CT_LDS_BODIES][6];
    for (int q = threadIdx.x; q < CT_LDS_BODIES * 6; q += 256) (&s_acc[0][0])[q] = 0ull;
    __syncthreads();
    bool bad = false;
#endif
    const unsigned n_active = ctl->n_active;
    const int tid = threadIdx.x;
    const int cell = tid & 63;
    const int cx = cell >> 4, cy = (cell >> 2) & 3, cz = cell & 3;
    // the multi-GPU path packs halo buffers right after this kernel: reset their entry counters here
    if (MODE == 0 && blockIdx.x == 0 && tid < 2 && p.halo_hdr[tid]) p.halo_hdr[tid][0] = 0u;
    if (MODE == 2 && p.halo_pn > 0 && tid < 64 && blockIdx.x * 64u < p.halo_pcap) {
        // Diagnostics of the received lists (what k_halo_add2 reports for the public mpm_halo_add; ADVICE r4): the add
        // below looks a zone block up in ITS zone's buffer, so a received block that lies in this rank's grid but outside
        // the zone its buffer belongs to would be dropped without a trace.  The first few workgroups look at 64 ids each.
        for (int k = 0; k < p.halo_pn; ++k) {
            const uint32_t* buf = p.halo_pbuf[k];
            const unsigned n = zbuf_count(buf, p.halo_pcap);
            for (unsigned e = blockIdx.x * 64u + (unsigned)tid; e < n; e += gridDim.x * 64u) {
                uint32_t id;
                const int a = zbuf_entry_block(p, buf, e, &id);
                if (a == ZBUF_BAD_ID) atomicOr(&p.ctl->error, ERR_HALO);   // (the buffer is not a halo buffer of this grid)
                if (a < 0) continue;
                int hx, hy, hz;
                block_coords(id, hx, hy, hz);
                if (hx < p.halo_plo[k] || hx > p.halo_phi[k]) atomicOr(&p.ctl->error, ERR_CAPACITY);
            }
        }
    }
    for (unsigned a = blockIdx.x * 4 + (tid >> 6); a < n_active; a += gridDim.x * 4) {
        if (MODE == 2 && p.halo_cls >= 0) {   // split update around the halo exchange (wave-uniform)
            int hx, hy, hz;
            block_coords(p.act_block[a], hx, hy, hz);
            if (!halo_block_selected(p, hx)) continue;
        }
        const int* nbr = p.act_nbr_items + (size_t)a * 27;
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        if (MODE == 2) {
            s = p.gv[(size_t)a * 64 + cell];
            if (p.halo_pn > 0) {
                // chain substep: the neighbour's sums for this block, straight from the received buffer (what k_halo_add2
                // does as a launch of its own for the public mpm_halo_add).  The buffer lists its blocks in the order its
                // sender's atomics fell: the wave scans the ids, 64 per step (a zone holds a few hundred blocks).  own +
                // received is the same pair of numbers on both ranks, so both compute identical node values.
                const uint32_t myid = p.act_block[a];
                int bx, by, bz;
                block_coords(myid, bx, by, bz);
                for (int k = 0; k < p.halo_pn; ++k) {
                    if (bx < p.halo_plo[k] || bx > p.halo_phi[k]) continue;   // wave-uniform
                    const uint32_t* buf = p.halo_pbuf[k];
                    const int found = zbuf_find(buf, zbuf_count(buf, p.halo_pcap), myid);
                    if (found >= 0) zbuf_add<1>(buf, p.halo_pcap, (unsigned)found, &s);
                }
            }
        }
        if (MODE != 2) {
            // Phase 1: lanes 0..26 look at one neighbour home block each and list the slabs (one per
            // work item of that block) whose stencils reached this block, in a fixed order
            // (split index, then offset).  Phase 2 streams through the list: all table walks are
            // done, the slab reads are independent and overlap.
            int2* list = s_list[tid >> 6];
            const int packed = cell < 27 ? nbr[cell] : -1;
            const int it0 = packed & 0xFFFFFF, ni = packed < 0 ? 0 : (packed >> 24);
            int cnt = 0;
            const int nimax = __reduce_max_sync_i32(ni);
            for (int k = 0; k < nimax; ++k) {
                // this block seen from the home block is at offset -o
                const bool hit = k < ni && ((p.slab_mask[it0 + k] >> (26 - cell)) & 1u);
                const unsigned long long m = __ballot(hit);
                if (hit) {
                    const int at = cnt + (int)__popcll(m & ((1ull << cell) - 1ull));
                    if (at < GRID_LIST) list[at] = make_int2(it0 + k, cell);
                }
                cnt += (int)__popcll(m);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            if (cnt > GRID_LIST) {   // > 160 slabs over one block (dozens of split, very heavy neighbours)
                if (cell == 0) atomicOr(&p.ctl->error, ERR_CAPACITY);
                cnt = GRID_LIST;
            }
#pragma unroll 4
            for (int e = 0; e < cnt; ++e) {
                const int2 en = list[e];
                const int it = en.x, o = en.y;
                const int tx = cx - 4 * (o / 9 - 1) + FREE_ZONE;
                const int ty = cy - 4 * ((o / 3) % 3 - 1) + FREE_ZONE;
                const int tz = cz - 4 * (o % 3 - 1) + FREE_ZONE;
                // branch-free so that the unrolled loads are issued back to back: lanes outside the
                // slab read its node 0 and add nothing
                const bool in_tile = !(tx < 0 || ty < 0 || tz < 0 || tx >= TILE_W || ty >= TILE_W || tz >= TILE_W);
                const int node = in_tile ? (tx * TILE_W + ty) * TILE_W + tz : 0;
                const float4 t = p.slab[(size_t)it * TILE_N + node];
                s.x += in_tile ? t.x : 0.f; s.y += in_tile ? t.y : 0.f;
                s.z += in_tile ? t.z : 0.f; s.w += in_tile ? t.w : 0.f;
            }
            __builtin_amdgcn_wave_barrier();   // the list is reused by the wave's next block
        }
        const size_t gi = (size_t)a * 64 + cell;
        if (MODE == 0) {
            p.gv[gi] = s;
            if (p.halo_pn > 0) {   // chain substep: blocks next to a cut go into the send buffers from here
                int bx, by, bz;
                block_coords(p.act_block[a], bx, by, bz);
                for (int k = 0; k < p.halo_pn; ++k) {
                    if (bx < p.halo_plo[k] || bx > p.halo_phi[k]) continue;   // wave-uniform
                    const int nbx = bx + p.halo_pshift[k];
                    if (nbx < 0 || nbx >= p.nb) continue;
                    uint32_t* buf = p.halo_pbuf[k];
                    const int slot = zbuf_claim(p.halo_pcnt[k] ? p.halo_pcnt[k] : &buf[0], p.halo_pcap, p.ctl);   // (see DP::halo_pcnt)
                    if (slot < 0) continue;
                    zbuf_store<1>(buf, p.halo_pcap, (unsigned)slot, block_id((uint32_t)nbx, (uint32_t)by, (uint32_t)bz), &s);
                }
            }
            continue;
        }
        float4 vs = make_float4(0.f, 0.f, 0.f, 0.f);
#if MPM_GRID_BODIES
        // One test per wave and body: the block's 4^3 nodes lie within 1.5 sqrt(3) dx of its centre, a body within
        // `bound` of its origin.  `live` is wave-uniform (a block per wave); a block outside every sphere skips the table.
        unsigned live = 0u;
        {
            int bx, by, bz;
            block_coords(p.act_block[a], bx, by, bz);
            const float c0 = (float)(bx * 4 + 2) * p.dx, c1 = (float)(by * 4 + 2) * p.dx, c2 = (float)(bz * 4 + 2) * p.dx;
            for (int k = 0; k < gb->n; ++k) {
                const GridBody& bd = gb->b[k];
                const float d0 = c0 - bd.c.p[0], d1 = c1 - bd.c.p[1], d2 = c2 - bd.c.p[2];
                const float rr = bd.bound + 2.6f * p.dx;
                if (!(d0 * d0 + d1 * d1 + d2 * d2 > rr * rr)) live |= 1u << k;   // (a NaN bound keeps the body)
            }
            live = (unsigned)__builtin_amdgcn_readfirstlane((int)live);
        }
#endif
        if (s.w > 0.f) {
            float v[3] = {s.x / s.w, s.y / s.w, s.z / s.w};
            int bx, by, bz;
            block_coords(p.act_block[a], bx, by, bz);
            const int gx = bx * 4 + cx, gy = by * 4 + cy, gz = bz * 4 + cz;
            const int N = 1 << p.bits, wl = p.M.wall;
            if (gx < wl && v[0] < 0.f) v[0] = 0.f;
            if (gx >= N - wl && v[0] > 0.f) v[0] = 0.f;
            if (gy < wl && v[1] < 0.f) v[1] = 0.f;
            if (gy >= N - wl && v[1] > 0.f) v[1] = 0.f;
            if (gz < wl && v[2] < 0.f) v[2] = 0.f;
            if (gz >= N - wl && v[2] > 0.f) v[2] = 0.f;
#if MPM_GRID_BODIES
            if (live) {
                const float pos[3] = {((float)gx + .5f) * p.dx, ((float)gy + .5f) * p.dx, ((float)gz + .5f) * p.dx};
                const float vin[3] = {v[0], v[1], v[2]};
                for (int k = 0; k < gb->n; ++k) {     // (uniform trip count and uniform `live`: scalar branches)
                    if (!((live >> k) & 1u)) continue;
                    const GridBody& bd = gb->b[k];
                    // membership and normal by the pair generator's functions (collider_inside / collider_sdf, mesh_sdf)
                    float n[3];
                    if (MESH && bd.mesh >= 0) {
                        if (!(mesh_sdf(gb->mesh[bd.mesh], pos, n) < 0.f)) continue;
                    } else {
                        if (!collider_inside(bd.c, pos)) continue;
                        if (ELL) collider_sdf(bd.c, pos, n);
                        else collider_sdf_closed(bd.c, pos, n);
                    }
                    // the body's velocity at the node: v_c(x) = v + w x (x - p_WB)
                    const float r[3] = {pos[0] - bd.c.p[0], pos[1] - bd.c.p[1], pos[2] - bd.c.p[2]};
                    const float vc[3] = {bd.c.v[0] + (bd.c.w[1] * r[2] - bd.c.w[2] * r[1]),
                                         bd.c.v[1] + (bd.c.w[2] * r[0] - bd.c.w[0] * r[2]),
                                         bd.c.v[2] + (bd.c.w[0] * r[1] - bd.c.w[1] * r[0])};
                    const float dv[3] = {vc[0] - v[0], vc[1] - v[1], vc[2] - v[2]};
                    const float dn = n[0] * dv[0] + n[1] * dv[1] + n[2] * dv[2];
                    if (bd.mode == 0) {
                        // v + (v_c - v) of :778-781 is v_c; written as such, no rounding residue of v is left in a
                        // moving body's nodes (for v_c = 0 both give +0)
                        v[0] = vc[0]; v[1] = vc[1]; v[2] = vc[2];
                    } else if (bd.mode == 2 || dn > 0.f) {
                        const float fr = bd.friction;
                        const float frac = (float)((double)dn * (1.0 - (double)fr));
                        v[0] += dv[0] * fr + n[0] * frac;
                        v[1] += dv[1] * fr + n[1] * frac;
                        v[2] += dv[2] * fr + n[2] * frac;
                    }
                    // reaction: the body receives l = -m (v_out - v_in) and (x - p_WB) x l, in double from the floats
                    const uint32_t b = bd.c.body;
                    if (b < (uint32_t)n_bodies) {
                        const double m = (double)s.w;
                        const double l[3] = {-m * ((double)v[0] - (double)vin[0]), -m * ((double)v[1] - (double)vin[1]),
                                             -m * ((double)v[2] - (double)vin[2])};
                        const double rd[3] = {(double)pos[0] - (double)bd.c.p[0], (double)pos[1] - (double)bd.c.p[1],
                                              (double)pos[2] - (double)bd.c.p[2]};
                        const double h[3] = {rd[1] * l[2] - rd[2] * l[1], rd[2] * l[0] - rd[0] * l[2], rd[0] * l[1] - rd[1] * l[0]};
                        unsigned long long* dst = b < (uint32_t)CT_LDS_BODIES ? &s_acc[b][0]
                                                                              : reinterpret_cast<unsigned long long*>(body_acc + (size_t)b * 6);
#pragma unroll
                        for (int i = 0; i < 3; ++i) {
                            const unsigned long long qh = (unsigned long long)imp_fixed(h[i], p.fix_p, bad);
                            const unsigned long long ql = (unsigned long long)imp_fixed(l[i], p.fix_p, bad);
                            if (b < (uint32_t)CT_LDS_BODIES) {
                                if (qh) __hip_atomic_fetch_add(dst + i, qh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                                if (ql) __hip_atomic_fetch_add(dst + 3 + i, ql, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            } else {
                                if (qh) __hip_atomic_fetch_add(dst + i, qh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                if (ql) __hip_atomic_fetch_add(dst + 3 + i, ql, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            }
                        }
                    }
                    break;
                }
            }
#else
            if (gc.n > 0) {
                const float pos[3] = {((float)gx + .5f) * p.dx, ((float)gy + .5f) * p.dx, ((float)gz + .5f) * p.dx};
                for (int k = 0; k < gc.n; ++k) {      // (uniform trip count: the table is a kernel argument)
                    const GridCollider& cl = gc.c[k];
                    float n[3], dist;
                    if (cl.shape == 0) {
                        const float d0 = pos[0] - cl.p[0], d1 = pos[1] - cl.p[1], d2 = pos[2] - cl.p[2];
                        const float len = sqrtf(d0 * d0 + d1 * d1 + d2 * d2);
                        const float inv = 1.f / len;
                        n[0] = d0 * inv; n[1] = d1 * inv; n[2] = d2 * inv;
                        dist = len - cl.radius;
                    } else {
                        n[0] = cl.n[0]; n[1] = cl.n[1]; n[2] = cl.n[2];
                        dist = n[0] * (pos[0] - cl.p[0]) + n[1] * (pos[1] - cl.p[1]) + n[2] * (pos[2] - cl.p[2]);
                    }
                    if (!(dist < 0.f)) continue;
                    // diff_vel = v_collider - v, dotnv = n . diff_vel  (:683-687)
                    const float dv[3] = {cl.v[0] - v[0], cl.v[1] - v[1], cl.v[2] - v[2]};
                    const float dn = n[0] * dv[0] + n[1] * dv[1] + n[2] * dv[2];
                    if (cl.mode == 0) {
                        v[0] += dv[0]; v[1] += dv[1]; v[2] += dv[2];          // :778-781
                    } else if (cl.mode == 2 || dn > 0.f) {
                        // :783-786; `dotnv * (1. - SDF_FRICTION)` is a double product in the reference
                        const float fr = cl.friction;
                        const float frac = (float)((double)dn * (1.0 - (double)fr));
                        v[0] += dv[0] * fr + n[0] * frac;
                        v[1] += dv[1] * fr + n[1] * frac;
                        v[2] += dv[2] * fr + n[2] * frac;
                    }
                    break;
                }
            }
#endif
            s.x = v[0]; s.y = v[1]; s.z = v[2];
            vs = make_float4(v[0], v[1], v[2], 0.f);
        }
        p.gv[gi] = s;
        p.gvs[gi] = vs;
    }
#if MPM_GRID_BODIES
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(&p.ctl->error, ERR_RANGE);
    __syncthreads();
    for (int q = threadIdx.x; q < min(n_bodies, CT_LDS_BODIES) * 6; q += 256) {
        const unsigned long long v = (&s_acc[0][0])[q];
        if (v != 0ull)
            __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(body_acc) + q, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#endif
