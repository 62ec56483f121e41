"""mpm_cloth_energy_density (the function of mpm_measure's kernels, compiled for the host) and the numpy restatement of
the report (tests/measure.py), without a GPU.

1. The energy density of 500 random F = Q (I + 0.2 N), half with r22 < 1 and half with r22 > 1, gamma = 0 and gamma > 0,
   against the independent psi of tests/measure.py (singular values from np.linalg.svd): within 8 x 2^-24 B per face, B
   the sum of the absolute values of psi's terms -- the only float roundings are those of the Lame parameters (mu: two,
   lambda: five), everything else is double.  s1, s2 and r22 themselves within 1e-12: the SVD and the closed form are both
   backward stable in double (a few 2^-53 of |F| <= 2).
2. For gamma = 0 its central-difference gradient equals the stress orc_kat_dphi_dF of the plain-C restatement of the
   reference to the 2e-6 that tests/test_oracle_model.py uses.  The entry takes FLOAT deformation gradients, so the step
   is h = 2^-20 (0.954e-6, the power of two next to 1e-6) on F rounded to multiples of 2^-22: F, F + h and F - h are then
   exact floats and the difference quotient is that of the double function, as in test_oracle_model.py.  (With h = 1e-6
   itself F +- h would be rounded to float by up to 2^-24 |F|: 6 % of the step.)
3. The restatement reproduces the analytic mass, momentum, angular momentum and kinetic energies of a rigidly translating
   and rotating rest sheet (rigid-body formulas: P = M v_c, L = c x M v_c + I_c w, KE = 1/2 M |v_c|^2 + 1/2 w . I_c w), its
   zero in-plane energy and the normal energy of a uniformly compressed director."""
import ctypes as C

import numpy as np

from tests import bending as bd
from tests import measure as ms

U = ms.U


def _materials():
    from drake_amd import ClothMaterial, GpuMpm
    base = ClothMaterial.of(GpuMpm.default_material())
    out = [base]
    for E, nu, K, gamma in ((1.7e5, 0.2, 3.1e4, 250.0), (9.3e5, 0.41, 2.2e5, 1300.0)):
        m = ClothMaterial.of(GpuMpm.default_material())
        m.youngs_modulus, m.poisson_ratio, m.K, m.gamma = E, nu, K, gamma
        out.append(m)
    return out


def _random_F(rng, n):
    F = np.zeros((n, 3, 3))
    for t in range(n):
        while True:
            A = np.eye(3) + 0.2 * rng.standard_normal((3, 3))
            if t % 2:
                A[:, 2] *= 1.3           # r22 > 1: no normal penalty
            Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
            if np.linalg.det(Q @ A) >= 0.2:
                break
        F[t] = Q @ A
    return F


def test_energy_density_against_the_independent_psi():
    from drake_amd import cloth_energy_density
    rng = np.random.default_rng(20261019)
    F = _random_F(rng, 500).astype(np.float32)
    worst, n_lo, n_hi = 0.0, 0, 0
    for mi, mat in enumerate(_materials()):
        out = cloth_energy_density(mat, F)
        mu, la = ms.lame(mat.youngs_modulus, mat.poisson_ratio)
        ref = ms.psi_terms(F, mu, la, float(mat.K), float(mat.gamma))
        n_lo, n_hi = int((ref["r22"] < 1).sum()), int((ref["r22"] > 1).sum())
        for col, key in enumerate(("s1", "s2", "r22")):
            assert np.abs(out[:, col] - ref[key]).max() <= 1e-12, (mi, key)
        for col, key, bk in ((3, "psi_in", "B_in"), (4, "psi_n", "B_n"), (5, "psi_s", "B_s")):
            err = np.abs(out[:, col] - ref[key])
            assert np.all(err <= 8 * U * ref[bk]), (mi, key, float((err / np.maximum(8 * U * ref[bk], 1e-300)).max()))
        tot = out[:, 3] + out[:, 4] + out[:, 5]
        err = np.abs(tot - (ref["psi_in"] + ref["psi_n"] + ref["psi_s"]))
        assert np.all(err <= 8 * U * ref["B"]), mi
        worst = max(worst, float((err / (8 * U * ref["B"])).max()))
        if float(mat.gamma) > 0:
            assert (ref["psi_s"] > 0).sum() > 400, "the random directors are tilted: the shear term is exercised"
        else:
            assert not out[:, 5].any()
        assert (out[ref["r22"] >= 1, 4] == 0).all() and (out[ref["r22"] < 1, 4] > 0).all()
    assert n_lo >= 200 and n_hi >= 200, (n_lo, n_hi)
    print(f"energy density: worst {worst:.3g} of 8 x 2^-24 B")
    from tests import helpers
    helpers.MARGINS.append((worst, "measure: host energy density", 1.0, worst, worst))


def test_degenerate_faces():
    """|n| = 0 (collinear tangents) takes r22 = 0 and no normal or shear energy; the rest configuration costs nothing"""
    from drake_amd import cloth_energy_density
    mat = _materials()[1]
    F = np.zeros((3, 3, 3), np.float32)
    F[0] = np.eye(3)
    F[1][:, 0], F[1][:, 1], F[1][:, 2] = (1, 0, 0), (2, 0, 0), (0.3, 0.2, 0.5)      # d2 parallel to d1
    F[2][:, 2] = (0, 0, 1)                                                           # d1 = d2 = 0
    out = cloth_energy_density(mat, F)
    assert np.array_equal(out[0], [1, 1, 1, 0, 0, 0])
    mu, la = ms.lame(mat.youngs_modulus, mat.poisson_ratio)
    assert out[1][1] == 0 and abs(out[1][0] - np.sqrt(5.0)) < 1e-14 and not out[1][2:3].any() and not out[1][4:].any()
    assert abs(out[1][3] - (mu * ((np.sqrt(5.0) - 1) ** 2 + 1) + 0.5 * la)) <= 8 * U * out[1][3]
    assert not out[2][:3].any() and not out[2][4:].any() and abs(out[2][3] - (2 * mu + 0.5 * la)) <= 8 * U * out[2][3]


def test_gradient_is_the_stress_of_the_reference_restatement():
    from drake_amd import ClothMaterial, cloth_energy_density
    from oracle import oracle as orc
    p = orc.default_params(6)
    assert float(p.gamma) == 0.0
    mat = ClothMaterial(float(p.youngs), float(p.poisson), float(p.density), 0.0, float(p.K), float(p.cF))
    rng = np.random.default_rng(20261005)
    h = 2.0 ** -20
    F64 = np.round(_random_F(rng, 200) * 2.0 ** 22) / 2.0 ** 22
    assert np.abs(F64).max() < 4.0 and np.array_equal(F64.astype(np.float32).astype(np.float64), F64)
    worst = 0.0
    mu = ms.lame(p.youngs, p.poisson)[0]
    for F in F64:
        batch = np.repeat(F[None], 18, axis=0)
        for i in range(3):
            for j in range(3):
                batch[2 * (3 * i + j), i, j] += h
                batch[2 * (3 * i + j) + 1, i, j] -= h
        b32 = batch.astype(np.float32)
        assert np.array_equal(b32.astype(np.float64), batch)
        e = cloth_energy_density(mat, b32)[:, 3:].sum(axis=1)
        Pn = ((e[0::2] - e[1::2]) / (2 * h)).reshape(3, 3)
        P = np.zeros(9, np.float64)
        Fc = np.ascontiguousarray(F, np.float64).reshape(9)
        orc.lib64().orc_kat_dphi_dF(C.byref(p), Fc.ctypes.data_as(C.POINTER(C.c_double)), P.ctypes.data_as(C.POINTER(C.c_double)))
        scale = max(np.abs(Pn).max(), mu * 1e-3)
        worst = max(worst, float(np.abs(P.reshape(3, 3) - Pn).max() / scale))
    print(f"gradient of the energy density against the stress: worst {worst:.3g}")
    assert worst < 2e-6, worst


def test_restatement_on_a_rigid_motion():
    rng = np.random.default_rng(5)
    X0, T = bd.sheet(7, 6, jitter=0.2, seed=4)
    X0 = X0.astype(np.float64)
    nf, nv = len(T), len(X0)
    Rot, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(Rot) < 0:
        Rot[:, 0] *= -1
    xv = (X0 - bd.CENTER) @ Rot.T + bd.CENTER
    w, v0 = np.array([1.3, -0.7, 2.1]), np.array([0.4, 0.2, -0.9])
    vel = lambda x: v0 + np.cross(w, x)            # noqa: E731
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    xf = xv[T].mean(axis=1)
    x = np.concatenate([xf, xv])
    m = rng.uniform(1e-6, 3e-6, nf + nv)
    vol = rng.uniform(1e-9, 2e-9, nf + nv)
    # Dm^-1 from the rest triangles (QR of the two edges), the director 0.9 of the rotated rest normal
    dminv, Fm = np.zeros((nf, 4)), np.zeros((nf, 3, 3))
    for f, (a, b, c) in enumerate(T):
        E = np.stack([X0[b] - X0[a], X0[c] - X0[a]], 1)
        q, r = np.linalg.qr(E)
        s = np.sign(np.diag(r))
        q, r = q * s, r * s[:, None]
        ri = np.linalg.inv(r)
        dminv[f] = (ri[0, 0], ri[0, 1], 0.0, ri[1, 1])
        d = Rot @ q
        Fm[f] = np.stack([d[:, 0], d[:, 1], 0.9 * np.cross(d[:, 0], d[:, 1])], 1)
    pids = rng.permutation(nf + nv)
    E_, nu_, K_, g_ = 4e5, 0.3, 1e5, 700.0
    d = dict(pids=pids, x=x[pids], v=vel(x)[pids], C=np.broadcast_to(W.reshape(9), (nf + nv, 9))[pids], m=m[pids], vol=vol[pids],
             F=Fm.reshape(nf, 9), dminv=dminv, tri=T)
    dx, g = 1.0 / 64, -9.8
    rows, faces = ms.restate(d, [dict(first_vertex=0, n_verts=nv, first_face=0, n_faces=nf, E=E_, nu=nu_, K=K_, gamma=g_)],
                             dx, g, 2)
    r = rows[0]
    M = m.sum()
    c = (m[:, None] * x).sum(axis=0) / M
    vc = vel(c)
    y = x - c
    Ic = (m[:, None, None] * ((y ** 2).sum(axis=1)[:, None, None] * np.eye(3) - y[:, :, None] * y[:, None, :])).sum(axis=0)
    D = 0.25 * dx * dx
    tol = lambda a: 1e-12 * max(float(np.abs(a).max()), 1e-300)      # noqa: E731
    assert abs(r["mass"][0] - M) <= tol(M)
    assert np.abs(r["mass_position"][0] - M * c).max() <= tol(M * c)
    assert np.abs(r["momentum"][0] - M * vc).max() <= 1e-12 * float(r["momentum"][1].max())
    L = np.cross(c, M * vc) + Ic @ w
    assert np.abs(r["angular_momentum"][0] - L).max() <= 1e-12 * float(r["angular_momentum"][1].max())
    assert abs(r["kinetic"][0] - (0.5 * M * vc @ vc + 0.5 * w @ Ic @ w)) <= 1e-12 * r["kinetic"][1]
    assert np.abs(r["affine_angular_momentum"][0] - 2 * D * M * w).max() <= tol(2 * D * M * w)
    assert abs(r["kinetic_affine"][0] - D * M * w @ w) <= tol(D * M * w @ w)
    assert abs(r["gravity_potential"][0] + g * M * c[2]) <= 1e-12 * r["gravity_potential"][1]
    # (in-plane: second order in the rounding of s - 1; shear: |d3|^2 - r22^2 is a difference of two roundings of 0.81)
    assert r["elastic_in_plane"][0] <= 1e-24 * E_ * vol[:nf].sum() and r["elastic_shear"][0] <= 1e-14 * g_ * vol[:nf].sum()
    en = (vol[:nf] * K_ / 3.0 * 0.1 ** 3).sum()
    assert abs(r["elastic_normal"][0] - en) <= 1e-12 * en
    assert np.abs(faces["s1"] - 1).max() < 1e-13 and np.abs(faces["s2"] - 1).max() < 1e-13 and np.abs(faces["r22"] - 0.9).max() < 1e-13
    assert r["stretch_max"] == 1 and r["stretch_min"] == 1 and r["normal_min"] == np.float32(0.9)
    assert r["speed_max"] == np.float32(np.linalg.norm(vel(xv), axis=1).max())
    assert (r["faces"], r["vertices"]) == (nf, nv) and r["bending"] == (0.0, 0.0)
    # the bending term against the hinge-by-hinge energy of tests/bending.py, on a bent image of the same sheet
    Xs = X0.astype(np.float32)
    H = bd.hinges(Xs, T)
    Q, _ = bd.q_dense(nv, H)
    xb = bd.state("cylinder3", Xs).astype(np.float64)
    d["x"] = np.concatenate([xb[T].mean(axis=1), xb])[pids]
    rows, _ = ms.restate(d, [dict(first_vertex=0, n_verts=nv, first_face=0, n_faces=nf, E=E_, nu=nu_, K=K_, gamma=g_)],
                         dx, g, 2, bending=[(2.5e-5, Q)])
    Eb = bd.energy64(float(np.float32(2.5e-5)), H, xb)
    assert Eb > 0 and abs(rows[0]["bending"][0] - Eb) <= 1e-9 * rows[0]["bending"][1]
