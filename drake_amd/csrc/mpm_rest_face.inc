// A face's rest state from its three corners: Dm^-1 and the quarter volume, with the rest frame Q on the way.  Included
// by mpm_io.h into k_init_faces (Finalize) and by mpm_rest.h into k_rest_faces (mpm_set_rest_shape); no include guard: it
// is meant to be read twice.  It is text rather than a shared device function for the reason mpm_fem_face.inc gives:
// k_init_faces preprocesses to the very tokens it had before k_rest_faces existed, so Finalize's results cannot move, and
// k_rest_faces evaluates the same expressions.  The includer has `p` (DP) and the float4 corners xa, xb, xc in scope.
    const float D0[3] = {xb.x - xa.x, xb.y - xa.y, xb.z - xa.z};
    const float D1[3] = {xc.x - xa.x, xc.y - xa.y, xc.z - xa.z};
    const float Ds[6] = {D0[0], D1[0], D0[1], D1[1], D0[2], D1[2]};
    float Q[9], R[6];
    givens_qr3<2>(Ds, Q, R);
    const float Dmat[4] = {R[0], R[1], 0.f, R[3]};
    float Di[4];
    inv2(Dmat, Di);
    const float cx = D0[1] * D1[2] - D1[1] * D0[2];
    const float cy = D0[2] * D1[0] - D1[2] * D0[0];
    const float cz = D0[0] * D1[1] - D1[0] * D0[1];
    const float v4 = sqrtf(cx * cx + cy * cy + cz * cz) / 8.f * p.dx;
