// The body of CalcFemStateAndForce's face kernels, included by mpm_step.h into k_fem and into k_fem_mat (no include
// guard: it is meant to be read twice).  It is text rather than a shared device function so that k_fem preprocesses to
// the very tokens it had before k_fem_mat existed -- routing it through an inlined function changed which product of one
// dot product the compiler fused into an FMA in k_fem<1>, and with it the last bit of some results.  The includer
// defines, in a scope that has `p` (DP), `dt` and the template parameter FM:
//   MPM_FEM_MATERIAL_SETUP  statements run once f3 (the face's fq[3] record) is loaded (k_fem: nothing)
//   MPM_FEM_M               the Material of the face (k_fem: p.M)
//   MPM_FEM_VOLW            the face particle's q[0].w (k_fem: its volume, or in a partitioned domain its signed record)
    if (gated_out(p)) return;
    const unsigned nfa = (unsigned)p.ctl->nfa;
    const unsigned chunk = xcd_chunk_active(blockIdx.x, nfa);
    const unsigned i = chunk * 256 + threadIdx.x;
    if (chunk == 0xFFFFFFFFu || i >= nfa) return;
    const PSet& S = p.set[p.ctl->cur];
    // A full substep: 104 bytes in (F 36, Dm^-1 | vol | corners 32, C 36) + the corner gathers; 116 bytes out (F 36, face x v 32,
    // tau factor a 12 -- the other one is F's normal column, see pack_F --, corner forces 36).  The face particle's own q[0] / q[1] are written, never read: its
    // volume comes from the static record, C8 from the c8 plane (see PSet).
    // Between the substeps of a batch (DP::lean_g2p, behind a lean substep: Ctl::f_inplane_stale) F's in-plane columns are
    // neither read nor written, 20 bytes each way: 84 bytes in + the gathers, one more of them per corner (PSet::xp, 16 B
    // per VERTEX, shared by its six faces through the L2), and 96 bytes out.  The first substep of a batch reads 104 and
    // writes 96, the last reads 84 and writes 116.
    // (the flag is k_g2p's to write, from the substep before: uniform, and constant while this launch runs)
    const bool stale = p.ctl->f_inplane_stale != 0;
    const float4 f0 = S.fq[0][i], f2 = S.fq[2][i], f3 = S.fq[3][i];
    // (set and used under the same uniform condition; filling them first would make the other path wait for its loads)
    float4 f1;
    float F7;
    if (!stale) { f1 = S.fq[1][i]; F7 = S.f8[i]; }
    const float C8 = S.c8[i];
    // (C with the first round of loads: it does not wait for the corners' slots)
    const float4 q2 = S.q[2][i], q3 = S.q[3][i];
    MPM_FEM_MATERIAL_SETUP
    // normal column evolves with the affine velocity field (:216-226).  Here, in front of the corner gathers: C's eight
    // registers are free again before the gathered records need theirs (the kernel stays within the 64 VGPRs of occupancy 8 with the
    // nine old corner coordinates of the stale path in flight)
    const float C[9] = {q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w, C8};
    float nF[3];
    {
        const float F2 = f0.x, F5 = f0.y, F8 = f0.z;
        nF[0] = (1.f + dt * C[0]) * F2 + dt * C[1] * F5 + dt * C[2] * F8;
        nF[1] = dt * C[3] * F2 + (1.f + dt * C[4]) * F5 + dt * C[5] * F8;
        nF[2] = dt * C[6] * F2 + dt * C[7] * F5 + (1.f + dt * C[8]) * F8;
    }
    asm volatile("" : "+v"(nF[0]), "+v"(nF[1]), "+v"(nF[2]));   // (... which the compiler otherwise moves behind them again)
    const unsigned s0 = (unsigned)__float_as_int(f3.y), s1 = (unsigned)__float_as_int(f3.z),
                   s2 = (unsigned)__float_as_int(f3.w);
    if (p.dist.on && (int)(s0 | s1 | s2) < 0) {
        // partitioned domain: a corner vertex of this face is not on this rank, so its state cannot
        // be advanced here.  The vertex band is wider than the face band by ghost_margin_cells exactly
        // so that this never happens; if it does, a mesh edge is longer than that margin.
        atomicOr(&p.ctl->error, ERR_HALO);
        const float nan = __int_as_float(0x7FC00000);
#pragma unroll
        for (int c = 0; c < 3; ++c) p.G3[(size_t)i * 3 + c] = make_float3(nan, nan, nan);
        p.ta[i] = make_float3(nan, nan, nan);
        return;
    }
    const float4 xa = S.q[0][s0], xb = S.q[0][s1], xc = S.q[0][s2];
    const float4 va = S.q[1][s0], vb = S.q[1][s1], vc = S.q[1][s2];
    // the corner positions the last substep's k_fem gathered (its k_g2p left them): what fq[1] / f8 would hold
    float3 oa, ob, oc;
    if (stale) {
        const unsigned nf = (unsigned)p.Nf;
        oa = *reinterpret_cast<const float3*>(&S.xp[s0 - nf]);
        ob = *reinterpret_cast<const float3*>(&S.xp[s1 - nf]);
        oc = *reinterpret_cast<const float3*>(&S.xp[s2 - nf]);
    }
    // partitioned domain: the sign of q[0].w is the particle's role (ghost copies are negative) and changes
    // with migration; a single-domain engine never looks at the face particle's own record
    const float volw = MPM_FEM_VOLW;
    __builtin_amdgcn_s_setprio(2);   // (a wave that has its data computes and stores ahead of waves still issuing loads)
    const float x0[3] = {xa.x, xa.y, xa.z}, x1[3] = {xb.x, xb.y, xb.z}, x2[3] = {xc.x, xc.y, xc.z};
    // the face particle sits at the centroid and moves with the mean velocity (:203-207);
    // vol and C8 ride along unchanged
    // (a third as a product: an IEEE division costs ten vector instructions, see f_rcp in mpm_math.h)
    const float third = FM == 0 ? 0.f : (1.f / 3.f);
    auto mean3 = [&](float a, float b, float c) { return FM == 0 ? (a + b + c) / 3.f : (a + b + c) * third; };
    S.q[0][i] = make_float4(mean3(xa.x, xb.x, xc.x), mean3(xa.y, xb.y, xc.y), mean3(xa.z, xb.z, xc.z), volw);
    S.q[1][i] = make_float4(mean3(va.x, vb.x, vc.x), mean3(va.y, vb.y, vc.y), mean3(va.z, vb.z, vc.z), C8);
    const float Dm0 = f2.x, Dm1 = f2.y, Dm3 = f2.z;   // Dm^-1 = [Dm0 Dm1; 0 Dm3]
    float F[9];
    if (stale) {
        // (the floats the last k_fem would have stored: the same function of the same positions and the same Dm^-1; F0
        // is one of them and rides in fq[0], which every substep stores)
        const float o0[3] = {oa.x, oa.y, oa.z}, o1[3] = {ob.x, ob.y, ob.z}, o2[3] = {oc.x, oc.y, oc.z};
        fem_inplane(o0, o1, o2, Dm0, Dm1, Dm3, F);
        F[0] = f0.w;
    } else {
        unpack_F(f0, f1, F7, F);
    }
    const float vol = f2.w;

    float cF[9];
    cF[0] = F[0]; cF[1] = F[1]; cF[2] = nF[0];
    cF[3] = F[3]; cF[4] = F[4]; cF[5] = nF[1];
    cF[6] = F[6]; cF[7] = F[7]; cF[8] = nF[2];
    project_strain<FM>(MPM_FEM_M, cF);
    // in-plane columns from the deformed edges (:230-250); the Dm^-1[2] = 0 terms are left out
    fem_inplane(x0, x1, x2, Dm0, Dm1, Dm3, cF);
    // (a lean substep leaves the in-plane columns to the next k_fem, which forms them again as above)
    pack_F_normal(cF, S.fq[0][i]);
    if (!p.lean_g2p) pack_F_inplane(cF, S.fq[1][i], S.f8[i]);

    float P[9];
    cloth_dphi_dF<FM>(MPM_FEM_M, cF, P);
#pragma unroll
    for (int d = 0; d < 9; ++d) P[d] *= vol;
    // tau = (V P[:,2]) (x) F[:,2]  (:265-267), kept factored: the second factor is in fq[0] already
    p.ta[i] = make_float3(P[2], P[5], P[8]);
    // grad_N = Dm^-T [[-1,1,0],[-1,0,1]]  (:269-276)
    const float g00 = -Dm0, g01 = Dm0;
    const float g10 = -Dm1 - Dm3, g11 = Dm1, g12 = Dm3;
    float Gm[9];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const float a = P[d * 3 + 0], b = P[d * 3 + 1];
        Gm[d * 3 + 0] = a * g00 + b * g10;
        Gm[d * 3 + 1] = a * g01 + b * g11;
        Gm[d * 3 + 2] = b * g12;
    }
    // one 12-byte record per corner, at its place among the vertex's entries (DP::VF) -- or, for a vertex with more than
    // eight faces, in the face's own triple of G3 (a corner that is not on this rank of a partitioned domain: nowhere; that
    // face belongs to a ghost band's outer edge, or the missing corner is an error the kernel has raised above)
    const unsigned jb = (unsigned)__float_as_int(f3.x);
    const unsigned sc[3] = {s0, s1, s2};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float3 rec = make_float3(Gm[c], Gm[3 + c], Gm[6 + c]);
        const unsigned j = (jb >> (4 * c)) & 15u;
        if (j < 8u) {
            if (!p.dist.on || (int)sc[c] >= p.Nf) *reinterpret_cast<float3*>(p.VF + vf_entry(sc[c] - (unsigned)p.Nf, j) * 3u) = rec;
        } else {
            p.G3[(size_t)i * 3 + c] = rec;
        }
    }
