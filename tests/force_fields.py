"""External force fields (mpm_set_force_fields; drake_amd/csrc/mpm_fields.h) on the CPU: the field tables of the
tests, a float64 and a float32 numpy restatement of the model, the extension of transfer_layouts.p2g64's inputs and of
its per-node bound.  Nothing here imports the engine.

Model (all coefficients per unit mass).  A field has u(x) = u0 + G (x - x0) and, with FF_REGION, the closed box
lo <= x <= hi, tested on the float32 position against the float32 corners -- float and double evaluation cannot
disagree about membership.  A particle's acceleration is the sum in table order over the fields that contain it:
    FF_ACCEL        u                                   faces and vertices
    FF_DRAG         -gamma (v - u)                      faces and vertices
    FF_NORMAL_DRAG  -gamma s n   (quadratic: s |s|)     faces only; s = (v - u) . n, n = d / |d|, d = F[:,2];
                                                        nothing where |d|^2 < 1e-30 (the float32 constant)
The director rule is exact on float inputs as long as |d|^2 is not within rounding of 1e-30: the tests use d = 0 and
|d| of order one.

Absolute terms.  T[p, r] is the sum over the fields acting on particle p of the absolute values of every term the
evaluation of component r forms separately, so that cancellation inside a field (v against the wind) and between fields
(drag against gravity) is covered:
    U_r = |u0_r| + sum_c |G_rc (x - x0)_c|                                  every kind (the terms of u_r)
    FF_ACCEL        U_r
    FF_DRAG         gamma |v_r| + gamma U_r
    FF_NORMAL_DRAG  gamma Wn   (quadratic: gamma Wn^2),   Wn = |(|v_c| + U_c)_c|_2  >=  |v - u|
        -- |v - u| itself would not do: where v nearly equals u the rounding error of the difference is of the size of
        |v| + U, not of |v - u|; |n_r| <= 1 is taken as 1.

Bounds (u = 2^-24).  R = 37 is the longest rounding chain of one field's evaluation, counted from the code of
mpm_fields.h (its header lists the count step by step): first order, a value that enters a product twice counted
twice; the quadratic normal drag is the longest (x - x0: 1, u: +3, v - u: +1 = 5; n: 6; s: 5 + 6 + 3 = 14; gamma s |s|:
14 + 14 + 2 = 30; times n and the accumulation: + 6 + 1 = 37).
    per particle    |a32 - a64|[r]  <=  K (R + 2) u T[r]        (K = 2; each of up to 8 accumulations rounds a partial
                    sum bounded by T: R - 1 + 8 <= K (R + 2))
    per node        the bound of transfer_layouts with 16 + R in place of 16 and A_n extended by w dt m T: the kernel
                    forms m (a dt) with two more roundings (a dt, the fused multiply-add with m) and adds it to the
                    vertex's f dt; those and the accumulations are within the factor K (K R >= R + 10).
They are rounding bounds, not fits: tests/test_force_fields.py pushes the float32 restatement below through the same
sums and finds it inside."""
import numpy as np

from tests import transfer_layouts as tl

FF_ACCEL, FF_DRAG, FF_NORMAL_DRAG = 0, 1, 2
FF_QUADRATIC, FF_REGION = 1, 2
R = 37
D2_MIN = np.float32(1e-30)
TABLES = ("accel", "drag_wind", "normal_linear", "normal_quadratic", "regions", "eight")


def field(kind, gamma=0.0, u0=(0, 0, 0), G=None, x0=(0, 0, 0), region=None, quadratic=False):
    """one field as a dict of float32 values (what mpm_force_field_t holds)"""
    f = dict(kind=int(kind), flags=(FF_QUADRATIC if quadratic else 0) | (FF_REGION if region is not None else 0),
             gamma=np.float32(gamma), u0=tl.f32(u0), G=tl.f32(np.zeros(9) if G is None else G).reshape(9).copy(),
             x0=tl.f32(x0), lo=tl.f32(np.zeros(3) if region is None else region[0]),
             hi=tl.f32(np.zeros(3) if region is None else region[1]))
    return f


def table(name, lo=(0.3, 0.3, 0.3), hi=(0.7, 0.7, 0.7), mid=None):
    """the field table `name` for particles inside the box lo .. hi (a layout's bounding box) with per-axis medians mid"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    c, e = 0.5 * (lo + hi), hi - lo
    mid = c if mid is None else np.asarray(mid, np.float64)
    shear = np.array([[0.0, 20.0, -5.0], [8.0, 0.0, 3.0], [-12.0, 6.0, 0.0]])
    spring = -400.0 * np.eye(3) + np.array([[0.0, 30.0, 0.0], [-30.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    if name == "accel":          # off-axis gravity plus a spring towards the centre with a swirl
        return [field(FF_ACCEL, u0=(1.5, -2.0, 3.0), G=spring, x0=c)]
    if name == "drag_wind":      # air drag towards an affine wind
        return [field(FF_DRAG, gamma=40.0, u0=(3.0, 0.5, -1.0), G=shear, x0=c)]
    if name == "normal_linear":
        return [field(FF_NORMAL_DRAG, gamma=60.0, u0=(2.0, -1.0, 0.5))]
    if name == "normal_quadratic":
        return [field(FF_NORMAL_DRAG, gamma=8.0, u0=(2.0, -1.0, 0.5), G=shear, x0=c, quadratic=True)]
    if name == "regions":        # boxes that cut through the particles at a median, one of them empty of particles
        return [field(FF_ACCEL, u0=(0.0, 4.0, -6.0), region=(lo - 1.0, [mid[0], hi[1] + 1, hi[2] + 1])),
                field(FF_DRAG, gamma=25.0, u0=(1.0, 1.0, 1.0), region=([lo[0] - 1, mid[1], lo[2] - 1], hi + 1.0)),
                field(FF_ACCEL, u0=(100.0, 100.0, 100.0), region=(hi + 1.0, hi + 2.0)),
                field(FF_NORMAL_DRAG, gamma=10.0, u0=(0.0, 0.0, 2.0), quadratic=True, region=(lo - 1.0, [hi[0] + 1, hi[1] + 1, mid[2]]))]
    if name == "eight":
        return [field(FF_ACCEL, u0=(0.0, 9.8, 0.0)),
                field(FF_DRAG, gamma=30.0, u0=(3.0, 0.5, -1.0), G=shear, x0=c),
                field(FF_ACCEL, G=spring, x0=c + 0.1 * e, region=(lo - 1.0, c + [1.0, 0.0, 1.0])),
                field(FF_NORMAL_DRAG, gamma=50.0, u0=(0.0, 0.0, 1.0)),
                field(FF_NORMAL_DRAG, gamma=5.0, u0=(1.0, 0.0, 0.0), G=0.5 * shear, x0=lo, quadratic=True),
                field(FF_DRAG, gamma=15.0, region=(c - 0.2 * e, hi + 1.0)),
                field(FF_ACCEL, u0=(-2.0, 0.0, 0.0), G=np.diag([50.0, 0.0, -50.0]), x0=c),
                field(FF_NORMAL_DRAG, gamma=20.0, u0=(0.0, -2.0, 0.0), region=(c, hi + 1.0))]
    raise KeyError(name)


def bbox(pos):
    """(lo, hi, per-axis median) of the positions: the arguments of table()"""
    pos = np.asarray(pos, np.float64)
    return pos.min(axis=0), pos.max(axis=0), np.median(pos, axis=0)


def _member(f, x32, is_face):
    """(n,) bool: the field acts on the particle -- region on the float32 inputs, normal drag on faces only"""
    on = np.ones(len(x32), bool)
    if f["flags"] & FF_REGION:
        on = ((x32 >= f["lo"][None]) & (x32 <= f["hi"][None])).all(axis=1)
    if f["kind"] == FF_NORMAL_DRAG:
        on = on & is_face
    return on


def _evaluate(fields, x, v, d, is_face, real):
    """the model in arithmetic `real` (np.float64, or np.float32: every operation rounded, no fused multiply-adds);
    -> (a, T): acceleration (n, 3) in `real` and the absolute terms (n, 3) in float64"""
    x32, v32 = tl.f32(x).reshape(-1, 3), tl.f32(v).reshape(-1, 3)
    n = len(x32)
    d32 = np.zeros((n, 3), np.float32) if d is None else tl.f32(d).reshape(-1, 3)
    is_face = np.broadcast_to(np.asarray(is_face, bool), (n,))
    X, V, D = x32.astype(real), v32.astype(real), d32.astype(real)
    X64, V64 = x32.astype(np.float64), v32.astype(np.float64)
    a, T = np.zeros((n, 3), real), np.zeros((n, 3))
    for f in fields:
        on = _member(f, x32, is_face)
        G, G64 = f["G"].reshape(3, 3).astype(real), f["G"].reshape(3, 3).astype(np.float64)
        gamma, g64 = real(f["gamma"]), float(f["gamma"])
        r = X - f["x0"].astype(real)[None]
        u = f["u0"].astype(real)[None] + G[None, :, 0] * r[:, 0:1]
        u = u + G[None, :, 1] * r[:, 1:2]
        u = u + G[None, :, 2] * r[:, 2:3]
        U = np.abs(f["u0"].astype(np.float64))[None] + np.einsum("rc,pc->pr", np.abs(G64), np.abs(X64 - f["x0"].astype(np.float64)[None]))
        if f["kind"] == FF_ACCEL:
            da, dT = u, U
        elif f["kind"] == FF_DRAG:
            da, dT = -gamma * (V - u), g64 * (np.abs(V64) + U)
        else:
            d2 = (D[:, 0] * D[:, 0] + D[:, 1] * D[:, 1]) + D[:, 2] * D[:, 2]
            on = on & (d2 >= real(D2_MIN))
            with np.errstate(all="ignore"):
                nrm = D * (real(1) / np.sqrt(d2))[:, None]
            w = V - u
            s = (w[:, 0] * nrm[:, 0] + w[:, 1] * nrm[:, 1]) + w[:, 2] * nrm[:, 2]
            c = gamma * s
            Wn = np.linalg.norm(np.abs(V64) + U, axis=1)
            if f["flags"] & FF_QUADRATIC:
                c = c * np.abs(s)
                dT = g64 * Wn * Wn
            else:
                dT = g64 * Wn
            da, dT = -c[:, None] * nrm, np.broadcast_to(dT[:, None], (n, 3))
        a = np.where(on[:, None], a + np.where(on[:, None], da, real(0)), a)
        T = T + np.where(on[:, None], dT, 0.0)
    return a, T


def accel64(fields, x, v, d=None, is_face=False):
    """float64 restatement: (a (n, 3), T (n, 3)); d: directors (n, 3) of the face particles (rows of the others unused)"""
    return _evaluate(fields, x, v, d, is_face, np.float64)


def accel32(fields, x, v, d=None, is_face=False):
    """the same formulas in float32, every operation rounded"""
    return _evaluate(fields, x, v, d, is_face, np.float32)[0]


def accel_bound(T):
    return tl.K * (R + 2) * tl.U32 * T


def p2g64_fields(fields, pos, vel, C, mass, taus, forces, directors, is_face, bits, gravity_axis, accel=None, dt=tl.DT32):
    """transfer_layouts.p2g64 with the fields' force m a added to `forces` (faces and vertices alike) and A_mv extended
    by w dt m T per node.  accel: the accelerations to scatter instead of the float64 ones (the float32 restatement)
    -> (r, a64, T)"""
    a64, T = accel64(fields, pos, vel, directors, is_face)
    m = np.asarray(mass, np.float64)
    a = a64 if accel is None else np.asarray(accel, np.float64)
    r = tl.p2g64(pos, vel, C, mass, taus, np.asarray(forces, np.float64) + m[:, None] * a, bits, gravity_axis, dt=dt)
    _, _, wt, keys = tl._stencil(pos, bits)
    ext = (np.abs(m) * dt)[:, None] * T                                    # (n, 3)
    k = keys.reshape(-1)
    for c in range(3):
        np.add.at(r["A_mv"][:, c], k, (wt * ext[:, c:c + 1]).reshape(-1))
    return r, a64, T


def p2g_bounds(r, quanta=None, L=None):
    """transfer_layouts.p2g_bounds with 16 + R: per-node bounds for mass (n_cells,) and momentum (n_cells, 3)"""
    L = r["L"] if L is None else L
    q_m, q_p = quanta if quanta else (0.0, 0.0)
    bm = tl.K * (L + 16) * tl.U32 * r["A_m"] + r["N"] * q_m
    bmv = tl.K * (L + 16 + R)[:, None] * tl.U32 * r["A_mv"] + r["N"][:, None] * q_p
    return bm, bmv


def layout_directors(lay, seed=11):
    """CPU stand-ins for F[:,2] of a layout's particles (the engine tests download the real ones): random directions,
    lengths 0.5 .. 1.5, rows of the vertex particles zero"""
    rng = np.random.default_rng(seed)
    n = lay["nf"] + lay["nv"]
    d = rng.normal(size=(n, 3))
    d *= (rng.uniform(0.5, 1.5, (n, 1)) / np.linalg.norm(d, axis=1, keepdims=True))
    d[lay["nf"]:] = 0.0
    return tl.f32(d)
