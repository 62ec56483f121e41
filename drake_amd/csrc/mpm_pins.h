// Fixed constraints: cloth vertices pinned to rigid bodies (mpm_set_pins, mpm_set_body_motions; include/mpm_hip.h).
// DeformableModel::AddFixedConstraint (deformable_model.h:227-230) for the MPM cloth: after GridToParticle a pinned
// vertex is put where its attachment point on the body is, with the body's velocity at that point and the exact
// velocity gradient of the rigid motion, and the body receives the impulse the constraint took from the cloth.
#pragma once
#include "mpm_contact_dev.h"
#include "mpm_device.h"

namespace mpm {

struct PinDev {          // one pin as k_pin reads it (24 bytes)
    uint32_t pid;        // particle id: Nf + vertex
    uint32_t motion;     // index into the motion table (resolved by the host from the pin's body)
    uint32_t body;       // accumulator index (>= n_bodies: no impulse)
    float p_BQ[3];
};
struct BodyMotionDev {   // one body's motion: pose at clock 0 and a constant spatial velocity, world frame (double)
    double p[3], R[9], v[3], w[3];
    double t;            // clock: seconds of applied substeps since the motion was set
    double pad;
};
struct PinArgs {
    const PinDev* pins;
    int n;
    BodyMotionDev* mot;
    int n_mot;
    long long* body_acc;   // [n_bodies][6] (tau, f) as in k_ct_impulse
    int n_bodies;
    double imp_fix;        // DP::fix_p
    unsigned* ticket;      // arrival counter of the workgroups (the last one advances the clocks)
};

// R(t) = Rodrigues(t w) R_WB and p(t) = p_WB + t v, in double.  Host and device (mpm_anchor_point runs it on the host):
// sin and cos are each platform's own, so the two agree within a rounding of the result, not to the bit.
__host__ __device__ __forceinline__ void pin_pose(const BodyMotionDev& m, double t, double* pt, double* Rt) {
    const double a[3] = {t * m.w[0], t * m.w[1], t * m.w[2]};
    const double th2 = a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
    double s, c;   // sin(th) / th, (1 - cos(th)) / th^2
    if (th2 < 1e-16) {
        s = 1.0 - th2 / 6.0;
        c = 0.5 - th2 / 24.0;
    } else {
        const double th = sqrt(th2);
        s = sin(th) / th;
        c = (1.0 - cos(th)) / th2;
    }
    const double K[9] = {0.0, -a[2], a[1], a[2], 0.0, -a[0], -a[1], a[0], 0.0};
    double Q[9];
    for (int r = 0; r < 3; ++r)
        for (int q = 0; q < 3; ++q) {
            double k2 = 0.0;
            for (int j = 0; j < 3; ++j) k2 += K[r * 3 + j] * K[j * 3 + q];
            Q[r * 3 + q] = (r == q ? 1.0 : 0.0) + s * K[r * 3 + q] + c * k2;
        }
    for (int r = 0; r < 3; ++r) {
        pt[r] = m.p[r] + t * m.v[r];
        for (int q = 0; q < 3; ++q) Rt[r * 3 + q] = Q[r * 3] * m.R[q] + Q[r * 3 + 1] * m.R[3 + q] + Q[r * 3 + 2] * m.R[6 + q];
    }
}

// One lane per pin, behind k_g2p on the same stream (launch_g2p).  Honours k_g2p's gate: a substep that skipped
// itself neither moves a pin nor advances a clock.
__global__ __launch_bounds__(256) void k_pin(DP p, PinArgs a, float dt) {
    __shared__ unsigned long long s_acc[CT_LDS_BODIES][6];
    __shared__ int s_last;
    if (p.gated && p.ctl->skip_this) return;   // (uniform: the same verdict k_g2p read)
    for (int q = threadIdx.x; q < CT_LDS_BODIES * 6; q += 256) (&s_acc[0][0])[q] = 0ull;
    __syncthreads();
    const PSet& S = p.set[p.ctl->cur];
    const uint32_t hi = (uint32_t)((1 << p.bits) - 3);
    const float lim = (float)(hi + 1u);
    bool bad = false;
    int left = 0;
    for (int k = blockIdx.x * 256 + threadIdx.x; k < a.n; k += gridDim.x * 256) {
        const PinDev pin = a.pins[k];
        const int slot = p.imap[pin.pid];
        if (slot < p.Nf || slot >= p.Np) continue;   // (cannot happen in a single-domain engine: every vertex has a slot)
        const BodyMotionDev& m = a.mot[min(pin.motion, (uint32_t)a.n_mot - 1u)];
        const double t = m.t + (double)dt;
        double pt[3], Rt[9];
        pin_pose(m, t, pt, Rt);
        double r[3], x[3], vq[3];
        for (int i = 0; i < 3; ++i) {
            r[i] = Rt[i * 3] * (double)pin.p_BQ[0] + Rt[i * 3 + 1] * (double)pin.p_BQ[1] + Rt[i * 3 + 2] * (double)pin.p_BQ[2];
            x[i] = pt[i] + r[i];
        }
        vq[0] = m.v[0] + (m.w[1] * r[2] - m.w[2] * r[1]);
        vq[1] = m.v[1] + (m.w[2] * r[0] - m.w[0] * r[2]);
        vq[2] = m.v[2] + (m.w[0] * r[1] - m.w[1] * r[0]);
        const float4 q0 = S.q[0][slot], q1 = S.q[1][slot];
        const float xn = (float)x[0], yn = (float)x[1], zn = (float)x[2];
        // C = [w]x, row-major; C8 = 0 rides in q[1].w
        const float w0 = (float)m.w[0], w1 = (float)m.w[1], w2 = (float)m.w[2];
        S.q[0][slot] = make_float4(xn, yn, zn, q0.w);
        S.q[1][slot] = make_float4((float)vq[0], (float)vq[1], (float)vq[2], 0.f);
        S.q[2][slot] = make_float4(0.f, -w2, w1, w2);
        S.q[3][slot] = make_float4(0.f, -w0, -w1, w0);
        // k_g2p's tile test (g2p_particle), on the target, in the tile of the block the slot was binned to by the last
        // re-sort (new slot s came from old slot src_of[s], whose key k_rb_count left in pkey); a target outside the grid
        // raises it too, so that the re-sort in front of the next ParticleToGrid reports ERR_DOMAIN
        const uint32_t src = p.src_of[slot];
        const uint32_t key = src < (uint32_t)p.Np ? p.pkey[src] : 0xFFFFFFFFu;
        bool fits = key != 0xFFFFFFFFu;
        if (fits) {
            int bx, by, bz;
            block_coords(key >> 6, bx, by, bz);
            const int ox = bx * 4 - FREE_ZONE, oy = by * 4 - FREE_ZONE, oz = bz * 4 - FREE_ZONE;
            const float guard = .125f, top = (float)(TILE_W - 2) - guard;
            const float tx = xn * p.dxinv - .5f - (float)ox, ty = yn * p.dxinv - .5f - (float)oy,
                        tz = zn * p.dxinv - .5f - (float)oz;
            fits = tx >= guard && tx < top && ty >= guard && ty < top && tz >= guard && tz < top;
        }
        auto inside = [&](float c) { const float u = c * p.dxinv - .5f; return u >= 0.f && u < lim; };
        if (!fits || !(inside(xn) && inside(yn) && inside(zn))) left = 1;
        // the reaction: the cloth received m (v_Q - v_g2p), the body the opposite, torque about the p_WB of the motion
        if (pin.body >= (uint32_t)a.n_bodies) continue;
        const double mass = (double)q0.w * (double)p.M.density;
        double l[3], h[3];
        l[0] = mass * ((double)q1.x - vq[0]);
        l[1] = mass * ((double)q1.y - vq[1]);
        l[2] = mass * ((double)q1.z - vq[2]);
        const double d[3] = {x[0] - m.p[0], x[1] - m.p[1], x[2] - m.p[2]};
        h[0] = d[1] * l[2] - d[2] * l[1];
        h[1] = d[2] * l[0] - d[0] * l[2];
        h[2] = d[0] * l[1] - d[1] * l[0];
        const uint32_t b = pin.body;
        unsigned long long* dst = b < (uint32_t)CT_LDS_BODIES ? &s_acc[b][0] : reinterpret_cast<unsigned long long*>(a.body_acc + (size_t)b * 6);
        for (int i = 0; i < 3; ++i) {
            const unsigned long long qh = (unsigned long long)imp_fixed(h[i], a.imp_fix, bad);
            const unsigned long long ql = (unsigned long long)imp_fixed(l[i], a.imp_fix, bad);
            if (b < (uint32_t)CT_LDS_BODIES) {
                __hip_atomic_fetch_add(dst + i, qh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_add(dst + 3 + i, ql, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            } else {
                __hip_atomic_fetch_add(dst + i, qh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_fetch_add(dst + 3 + i, ql, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    // (a plain store, as in k_g2p: the flag only goes 0 -> 1 here)
    if (__ballot(left) && (threadIdx.x & 63) == 0) p.ctl->need_rebuild = 1;
    if (__ballot(bad) && (threadIdx.x & 63) == 0) atomicOr(&p.ctl->error, ERR_RANGE);
    __syncthreads();
    for (int q = threadIdx.x; q < min(a.n_bodies, CT_LDS_BODIES) * 6; q += 256) {
        const unsigned long long v = (&s_acc[0][0])[q];
        if (v != 0ull)
            __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(a.body_acc) + q, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    // every workgroup has read the clocks before it arrives here; the last one to arrive advances them
    if (threadIdx.x == 0) {
        __threadfence();
        s_last = atomicAdd(a.ticket, 1u) == gridDim.x - 1u;
    }
    __syncthreads();
    if (s_last) {
        __threadfence();
        for (int q = threadIdx.x; q < a.n_mot; q += 256) a.mot[q].t += (double)dt;
        if (threadIdx.x == 0) *a.ticket = 0u;
    }
}

}  // namespace mpm
