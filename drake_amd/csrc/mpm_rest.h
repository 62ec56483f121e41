// The rest shape apart from the pose (mpm_set_rest_shape): Finalize's rest state -- Dm^-1 and the static volume per
// face, the volume or mass of every particle -- computed again from other vertex positions, on whatever particle order
// the re-sorts have made by then.  Two kernels for gfx950, launched once per call on the engine's stream:
//   k_rest_faces     one lane per face slot: k_init_faces' arithmetic (mpm_rest_face.inc, the same text) on the rest
//                    positions of the face's corners
//   k_rest_vertices  one lane per vertex slot: k_init_vertex_volumes' sum, in ascending original face id
// Both find the particle's original id through PSet::pid of the current set (Ctl::cur) and the topology through the
// tables by original id (DP::idx_orig, adj_off, adj_fc).  Positions, velocities, C, F and the particle order are not
// touched.  Single-domain engines only: a partitioned rank has no DP::dm_orig and holds a part of the scene.
#pragma once
#include "mpm_device.h"

namespace mpm {

struct RestArgs {
    const float* rest;    // [3 Nv] the rest positions by original vertex id
    float* quarter;       // [Nf] scratch of the call: a face's quarter volume by original face id (k_rest_faces writes it,
                          // k_rest_vertices sums it; DP::G3 holds the corner forces of the last FEM pass and stays as it is)
    const float* rho;     // [Np] the density of a particle's cloth by original id: a multi-material engine, whose q[0].w is
                          // the mass (k_init_masses' product, volume x density); null: q[0].w is the volume
};

// 28 bytes in per face (pid, three corner ids) + three 12-byte gathers; 40 bytes out + two scattered stores by original id
__global__ __launch_bounds__(256) void k_rest_faces(DP p, RestArgs a) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= p.Nf) return;
    const PSet& S = p.set[p.ctl->cur];
    const int f = S.pid[j];
    if ((unsigned)f >= (unsigned)p.NfG) return;   // (a free slot: a single-domain engine has none)
    float4 xa, xb, xc;
    {
        const float* r0 = a.rest + 3 * (size_t)(p.idx_orig[0][f] - p.NfG);
        const float* r1 = a.rest + 3 * (size_t)(p.idx_orig[1][f] - p.NfG);
        const float* r2 = a.rest + 3 * (size_t)(p.idx_orig[2][f] - p.NfG);
        xa = make_float4(r0[0], r0[1], r0[2], 0.f);
        xb = make_float4(r1[0], r1[1], r1[2], 0.f);
        xc = make_float4(r2[0], r2[1], r2[2], 0.f);
    }
#include "mpm_rest_face.inc"   // (Q, Di, v4 from xa, xb, xc: the text of k_init_faces)
    (void)Q;   // (the rest frame: F stays the pose's)
    S.fq[2][j] = make_float4(Di[0], Di[1], Di[3], v4);
    const_cast<float4*>(p.dm_orig)[f] = make_float4(Di[0], Di[1], Di[2], Di[3]);
    S.q[0][j].w = a.rho ? v4 * a.rho[f] : v4;
    a.quarter[f] = v4;
}

__global__ __launch_bounds__(256) void k_rest_vertices(DP p, RestArgs a) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= p.Nv) return;
    const PSet& S = p.set[p.ctl->cur];
    const int j = p.Nf + k;
    const int id = S.pid[j];
    const int v = id - p.NfG;
    if ((unsigned)v >= (unsigned)p.Nv) return;
    float vol = 0.f;
    for (int e = p.adj_off[v]; e < p.adj_off[v + 1]; ++e) vol += a.quarter[p.adj_fc[e] >> 2];
    S.q[0][j].w = a.rho ? vol * a.rho[id] : vol;
}

}  // namespace mpm
