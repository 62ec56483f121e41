"""Fixed constraints (k_pin, drake_amd/csrc/mpm_pins.h) per pin and per body on the CPU: what tests/pin_reference.py states,
restated in numpy float64 with error bounds, the layouts of tests/test_pin_layouts_gpu.py, and deliberately wrong
restatements for the self-test of tests/test_pin_layouts.py.  No GPU at import.

Inputs: the float32 state the engine holds, the pin table, the motions as the float32 values given (anchors.motion32), and
per-body clocks as sums of float64(float32(dt)) in the order the substeps ran (the device's `m.t += (double)dt`).

The model.  With t = clock + dt, p(t) = p_WB + t v, R(t) = Rodrigues(t w) R_WB (anchors.pose64), per pin
    x = p(t) + R(t) p_BQ,   v_Q = v + w x (R(t) p_BQ),   C = [w]x (float32 values of w, exact),   q[1].w = C8 = 0
and per body b < n_bodies, with m_i the mass k_pin forms ((double)q[0].w (double)density: the volume times the density,
or on a multi-material engine the mass times 1) and v_g2p,i what GridToParticle left in the record,
    l_i = m_i (v_g2p,i - v_Q,i),   f_b = sum l_i,   tau_b = sum (x_i - p_WB) x l_i     (p_WB: the motion's pose at clock 0)
Bodies at or beyond n_bodies receive nothing.

Bounds, from the kernel's arithmetic (u = 2^-53, U = 2^-24).

pin_pose in double.  a = t w: 1 rounding.  th2: 3 squares and 2 sums of rounded a, relative 5u; th = sqrt: 4u.  The term
s K = sin(th) (a / th): sin's argument carries 4u th absolute, the device library's sin 2 ulp <= 4u, the division, a and
the product 7u relative of a value <= 1: (11 + 4 th) u.  The term c K K = (1 - cos th) (K K / th2), |K K / th2| <= 1: cos
likewise 4u th + 4u, the subtraction 2u, the division by th2 (6u), the three products and two sums of K K (5u) and the
product (1u) relative of 1 - cos <= 2: (30 + 4 th) u.  (Just above the series' threshold 1 - cos th is wrong by its own
size, about u: that is inside the 4u of the cosine.)  The two sums into Q, entries <= 3: 6u.  An entry of Q: (47 + 8 th) u.
R(t) = Q R_WB, three products and two sums per entry with sum |R_WB| <= sqrt 3 per column: sqrt 3 (47 + 8 th) u + 6u; then
R(t) p_BQ, three products, two sums: a component of the arm r is wrong by at most
    (3 (sqrt 3 (47 + 8 th) + 6) + 6) u |p_BQ| <= (269 + 42 th) u |p_BQ| <= 280 (1 + th) u |p_BQ|.
p(t): 2u (|p_WB| + |t v|); the sum x = p(t) + r: u |x|.  Rounded up, one evaluation of x is within
    C_POSE u (1 + |w| t) (|p(t)| + |p_BQ|),   C_POSE = 300,
and v_Q = v + w x r, two products and a difference per component on sqrt 2 |w| of the arm's error, plus the sum: within
C_POSE u sqrt 2 (1 + |w| t) (|v| + |w| |p_BQ|).  The reference below is float64 itself with the same operations, so the
double term of a comparison is twice that; one constant for both: 2 sqrt 2 C_POSE < 900.
    position:  U_half(|x64|) + 900 u (1 + |w| t) (|p(t)| + |p_BQ|)       per component; U_half = half a float32 ulp:
    velocity:  U_half(|v_Q64|) + 900 u (1 + |w| t) (|v| + |w| |p_BQ|)     the kernel rounds its double once
(where the double values straddle a power of two the float lies within the double term of it).  C is exact.

Body sums (read after a single substep that follows a zeroing mpm_reallocate_external_bodies).  Every l_i and every
(x_i - p_WB) x l_i is converted to fixed point by rounding to the nearest multiple of the quantum q (read from the engine;
quantum_of restates it), the integer sums are exact, and mpm_external_body_force_to_host rounds the sum to float32 once:
    force:   n_b q / 2 + sum_i (m_i Dv_i + 4u |l_i|) + U |f_b|
    torque:  n_b q / 2 x reach_b + sum_i 2 (|d_i| (m_i Dv_i + 4u |l_i|) + |l_i| (Dx_i + u |d_i|)) + 4u sum |d_i| |l_i| + U |tau_b|
with Dx_i, Dv_i the double terms above, d_i = x_i - p_WB, reach_b = max |d_i|: the quantum term times the arm's reach,
as tests/test_anchors_gpu.py takes it.  (The kernel converts the cross product itself, q / 2 per pin whatever the arm, so
with reach_b < 1, as in these layouts, this term understates the conversion; n_b q / 2 is 1e-2 of the float32 rounding
here.)  4u |l_i|: the mass product, the difference and the product; the cross product doubles what enters it and adds
its own three roundings on the gross |d| |l|.

The tile-fit verdict is float32 as the kernel writes it: dxinv is a power of two, so x * dxinv is exact and contraction
cannot change `x * dxinv - .5f - (float)o`; numpy's float32 operations round as the device's do."""
import numpy as np

from tests import anchors as an
from tests import links as lk
from tests.pin_reference import pin_target, skew

U = 2.0 ** -24
U64 = 2.0 ** -53
C_POSE = 300.0
C_CMP = 900.0            # 2 sqrt 2 C_POSE, rounded up: a device evaluation against a float64 one
H0 = lk.H0
BITS, DXINV = 6, 64.0
FREE_ZONE, TILE_W, GUARD = 2, 10, 0.125
CT_LDS_BODIES, GROUP = 32, 256
PIN_DTYPE = np.dtype([("vertex", "<u4"), ("body", "<u4"), ("p_BQ", "<f4", (3,))])
N = 25                   # vertices along a sheet's side
NV = N * N
DT = 1e-3
DRIFT = (9.0, 0.0, 0.0)  # 9 m/s * 1e-3 s * 64 cells = 0.58 cells per substep: re-sorts inside a batch of 8
N_BODIES = 34
BODIES = (0, 1, 31, 32, 33, 40)    # 32, 33: beyond the LDS accumulators; 40: beyond the accumulators' count
BODY_FAR, BODY_NONE = 33, 40


def make_table(rows):
    out = np.zeros(len(rows), PIN_DTYPE)
    for i, (v, b, q) in enumerate(rows):
        out[i] = (v, b, tuple(np.asarray(q, np.float32)))
    return out


def clock_after(dts, start=0.0):
    """the device's clock: float64(float32(dt)) added in double, in order"""
    t = float(start)
    for d in dts:
        t += float(np.float32(d))
    return t


def quantum_of(total_mass):
    """the accumulators' quantum as the engine derives it from the scene's mass: 2^(ceil(log2 M) - 47)"""
    return 2.0 ** (int(np.ceil(np.log2(total_mass))) - 47)


def half_ulp32(a):
    """half a float32 ulp of |a|, elementwise"""
    return 0.5 * np.spacing(np.abs(np.asarray(a, np.float64)).astype(np.float32)).astype(np.float64)


def _series_pose(motion, t):
    """anchors.pose64 with the series of pin_pose's small-angle branch whatever the angle (a wrong restatement)"""
    p, R, v, w = (np.asarray(a, np.float32).astype(np.float64) for a in motion)
    a = t * w
    th2 = float(a @ a)
    K = skew(a)
    return p + t * v, (np.eye(3) + (1.0 - th2 / 6.0) * K + (0.5 - th2 / 24.0) * (K @ K)) @ R.reshape(3, 3), p, v, w


WRONG = ("torque_about_pt", "arm_at_t", "clock_per_workgroup", "other_mass", "series_above", "drop_far", "none_into_far")


def restate(table, motions, clocks, dt, n_bodies=0, mass=None, v_g2p=None, quantum=0.0, wrong=None):
    """The substep of size dt on pins `table` (PIN_DTYPE), clocks {body: t} (or one t) before it.
    -> dict: x, vq (n, 3) float64; C (n, 3, 3) float32; bx, bv (n, 3) bounds; t {body: clock + dt};
    with mass (n,) and v_g2p (n, 3) per pin also f, tau (n_bodies, 3) float64, bf, btau (n_bodies,), count (n_bodies,),
    gross_f, gross_tau.  `wrong`: one of WRONG ("other_mass" is the caller's: it passes the other cloth's masses)."""
    assert wrong is None or wrong in WRONG
    dt64 = float(np.float32(dt))
    n = len(table)
    x, vq, arm0 = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
    C = np.zeros((n, 3, 3), np.float32)
    dx, dv = np.zeros(n), np.zeros(n)
    groups = (n + GROUP - 1) // GROUP
    ts = {}
    for b in np.unique(table["body"]):
        b = int(b)
        sel = table["body"] == b
        t0 = clocks[b] if isinstance(clocks, dict) else float(clocks)
        if wrong == "clock_per_workgroup":
            t0 *= groups
        t = ts[b] = t0 + dt64
        pose = _series_pose if wrong == "series_above" else an.pose64
        pt, Rt, p0, v, w = pose(motions[b], t)
        if wrong == "arm_at_t":
            Rt = pose(motions[b], t0)[1]
        q = table["p_BQ"][sel].astype(np.float64)
        r = q @ Rt.T
        x[sel] = pt + r
        vq[sel] = v + np.cross(w, r)
        C[sel] = skew(w).astype(np.float32)
        arm0[sel] = r if wrong == "torque_about_pt" else x[sel] - p0
        qn, wn = np.linalg.norm(q, axis=1), float(np.linalg.norm(w))
        dbl = C_CMP * U64 * (1.0 + wn * abs(t))
        dx[sel] = dbl * (np.linalg.norm(pt) + qn)
        dv[sel] = dbl * (np.linalg.norm(v) + wn * qn)
    out = dict(x=x, vq=vq, C=C, bx=half_ulp32(x) + dx[:, None], bv=half_ulp32(vq) + dv[:, None], t=ts)
    if mass is None:
        return out
    m = np.asarray(mass, np.float64)
    l = m[:, None] * (np.asarray(v_g2p, np.float32).astype(np.float64) - vq)
    ln, dn = np.linalg.norm(l, axis=1), np.linalg.norm(arm0, axis=1)
    el = m * dv + 4 * U64 * ln
    f, tau = np.zeros((n_bodies, 3)), np.zeros((n_bodies, 3))
    bf, btau, count = np.zeros(n_bodies), np.zeros(n_bodies), np.zeros(n_bodies, int)
    gf, gt = np.zeros(n_bodies), np.zeros(n_bodies)
    for b in range(n_bodies):
        src = BODY_NONE if wrong == "none_into_far" and b == BODY_FAR else None
        sel = (table["body"] == b) | (table["body"] == src if src is not None else False)
        if not sel.any() or (wrong == "drop_far" and b == BODY_FAR):
            continue
        count[b] = int(sel.sum())
        f[b], tau[b] = l[sel].sum(axis=0), np.cross(arm0[sel], l[sel]).sum(axis=0)
        gf[b], gt[b] = ln[sel].sum(), (dn[sel] * ln[sel]).sum()
        bf[b] = count[b] * quantum / 2 + el[sel].sum() + U * np.abs(f[b]).max()
        btau[b] = (count[b] * quantum / 2 * dn[sel].max() + 2 * (dn[sel] * el[sel] + ln[sel] * (dx[sel] + U64 * dn[sel])).sum()
                   + 4 * U64 * gt[b] + U * np.abs(tau[b]).max())
    out.update(f=f, tau=tau, bf=bf, btau=btau, count=count, gross_f=gf, gross_tau=gt)
    return out


def pin_bounds(motion, p_BQ, t):
    """(x, v_Q, C, bound of x (n, 3), bound of v_Q (n, 3)) of pins p_BQ (n, 3) on one motion at clock t: pin_target of
    tests/pin_reference.py with the bounds of this module"""
    q = np.asarray(p_BQ, np.float32).reshape(-1, 3)
    r = restate(make_table([(i, 0, q[i]) for i in range(len(q))]), {0: an.motion32(*motion)}, t, 0.0)
    xt, vt, Ct = pin_target(motion, q, t)
    assert np.array_equal(xt, r["x"]) and np.array_equal(vt, r["vq"])
    return xt, vt, Ct, r["bx"], r["bv"]


# ---- the tile-fit verdict, float32 as the kernel writes it ---------------------------------------------------------------
def _compact3(v):
    v &= 0x09249249
    v = (v ^ (v >> 2)) & 0x030C30C3
    v = (v ^ (v >> 4)) & 0x0300F00F
    v = (v ^ (v >> 8)) & 0xFF0000FF
    v = (v ^ (v >> 16)) & 0x000003FF
    return v


def block_coords(block):
    """Morton id of a 4^3 block, x in the highest bit of each triple -> (bx, by, bz)"""
    block = int(block)
    return _compact3(block >> 2), _compact3(block >> 1), _compact3(block)


def block_of(x32):
    """the block a particle at rest at x32 is binned to: base cell int(x * dxinv - .5), four cells to a block"""
    f = np.float32
    t = np.asarray(x32, f) * f(DXINV) - f(0.5)
    return tuple(int(c) >> 2 for c in np.maximum(t, 0).astype(np.int64))


def tile_verdict(x32, block, bits=BITS):
    """(fits, inside) of a target x32 (3,) float32 for a slot binned to `block` (bx, by, bz), or None for the key
    0xFFFFFFFF: k_pin raises need_rebuild unless both hold"""
    f = np.float32
    x32 = np.asarray(x32, f)
    u = x32 * f(DXINV) - f(0.5)
    inside = bool(np.all((u >= f(0)) & (u < f((1 << bits) - 2))))
    if block is None:
        return False, inside
    o = np.array([4 * c - FREE_ZONE for c in block], f)
    t = u - o
    top = f(TILE_W - 2) - f(GUARD)
    return bool(np.all((t >= f(GUARD)) & (t < top))), inside


def host_verdicts(x32, vertices, nf, imap, src_of, pkey):
    """need_rebuild as k_pin decides it, per pin: targets x32 (n, 3) float32, the tables of the last re-sort
    (IMAP, SRC_OF, PKEY of mpm_debug_resort_tables).  -> (left (n,) bool, inside (n,) bool)"""
    left, ins = np.zeros(len(vertices), bool), np.zeros(len(vertices), bool)
    for k, v in enumerate(vertices):
        slot = int(imap[nf + int(v)])
        src = int(src_of[slot])
        key = int(pkey[src]) if src < len(pkey) else 0xFFFFFFFF
        fits, inside = tile_verdict(x32[k], None if key == 0xFFFFFFFF else block_coords(key >> 6))
        left[k], ins[k] = not (fits and inside), inside
    return left, ins


# ---- layouts -------------------------------------------------------------------------------------------------------------
def _x_of(u):
    """the position whose grid coordinate x * dxinv - .5 is u"""
    return (np.asarray(u, np.float64) + 0.5) / DXINV


def _sheets(ua, ub):
    return [lk.sheet(N, N, _x_of(ua)), lk.sheet(N, N, _x_of(ub))]


def _drifting(cloths, seed):
    X = np.concatenate([c[0] for c in cloths])
    v0 = np.asarray(DRIFT, np.float32) + (0.05 * np.random.default_rng(seed).normal(size=X.shape)).astype(np.float32)
    return X, v0


def _p_BQ(motion, target, t=0.0):
    return an._p_BQ(motion, t, target)


_UA, _UB = (8.0, 20.0, 30.5), (8.0, 20.0, 31.5)      # B one cell above A
_CENTRE = _x_of((14.0, 26.0, 31.0))


def _many_motions():
    V = np.asarray(DRIFT)
    spec = {   # offset of p_WB from the centre, axis and angle of R_WB, v - drift, w
        0: ((0.01, 0.0, 0.02), (1, 2, 3), 0.4, (0.02, -0.01, 0.01), (0.3, -0.2, 0.5)),
        1: ((0.0, 0.01, 0.03), (3, -1, 2), 1.1, (-0.02, 0.02, 0.0), (-0.4, 0.5, 0.2)),
        31: ((-0.01, 0.0, 0.02), (0, 1, 0), 0.2, (0.01, 0.02, -0.01), (0.6, 0.3, -0.4)),
        32: ((0.0, -0.01, 0.03), (1, 0, 0), 0.7, (0.0, -0.03, 0.02), (-0.5, -0.6, 0.3)),
        33: ((0.02, 0.02, 0.04), (1, 1, 0), 2.9, (-0.03, 0.01, 0.0), (0.7, -0.5, -0.6)),
        40: ((-0.02, 0.02, 0.04), (2, 0, 1), 0.5, (0.02, 0.0, 0.03), (0.2, 0.8, 0.4)),
    }
    return {b: an.motion32(_CENTRE + off, an._rot(ax, ang), V + dv, w) for b, (off, ax, ang, dv, w) in spec.items()}


def layout_many():
    """two 25 x 25 sheets flying along x; every other vertex pinned, 625 pins (three workgroups: 256 + 256 + 113) listed
    in the order vertex 2 (383 k mod 625), bodies 0, 1, 31, 32, 33, 40 in turn along the table: every body has pins in
    every workgroup.  Each pin's target at clock 0 is its vertex's rest position."""
    cloths = _sheets(_UA, _UB)
    X, v0 = _drifting(cloths, 11)
    motions = _many_motions()
    rows = []
    for k in range(NV):
        v, b = 2 * ((383 * k) % NV), BODIES[k % len(BODIES)]
        rows.append((v, b, _p_BQ(motions[b], X[v])))
    return dict(name="many", cloths=cloths, X=X, v0=v0, table=make_table(rows), motions=motions, n_bodies=N_BODIES, dt=DT,
                densities=None)


def layout_materials():
    """the `many` scene on a multi-material engine: cloth B four times as dense as cloth A"""
    out = dict(layout_many(), name="materials", densities=(1.0, 4.0))
    return out


REGIMES = ("zero", "series", "above", "one", "pi", "far")
_REGIME_ANGLE = dict(zero=0.0, series=5e-9, above=1.2e-8, one=1.0, pi=np.pi - 5e-4, far=41.0)
_REGIME_ARM = dict(one=1e-3, pi=3e-4, far=2.5e-5)       # |w| |p_BQ| = 1 m/s at most


def layout_regimes():
    """One body per rotation regime at the first substep (clock 0, so the angle is |w| dt): w = 0; 5e-9 (the series
    branch); 1.2e-8 (just above it); 1; pi - 5e-4; 41 rad.  Each with a non-identity R_WB, an oblique axis and the
    drift plus a little as v.  The three slow bodies hold 12 vertices each at their rest positions; a fast body pinches a
    vertex of sheet A and the one above it on sheet B to within its arm (|w| |p_BQ| <= 1 m/s) of the point between them,
    half a cell from either: inside the domain and within two cells of the vertex."""
    cloths = _sheets(_UA, _UB)
    X, v0 = _drifting(cloths, 12)
    V, dt64 = np.asarray(DRIFT), float(np.float32(DT))
    axes = [(1, 2, 3), (3, -1, 2), (-2, 1, 2), (1, -3, 1), (2, 2, -1), (-1, 2, 3)]
    motions, rows = {}, []
    for b, name in enumerate(REGIMES):
        ax = np.asarray(axes[b], np.float64) / np.linalg.norm(axes[b])
        w = ax * _REGIME_ANGLE[name] / dt64
        R, dv = an._rot(axes[(b + 1) % 6], 0.3 + 0.4 * b), 0.01 * np.asarray(axes[(b + 2) % 6], np.float64)
        if name in _REGIME_ARM:
            i, j = 4 + 5 * (b - 3), 12
            va, vb = i * N + j, NV + i * N + j
            motions[b] = an.motion32(0.5 * (X[va].astype(np.float64) + X[vb]) + (1e-4, -2e-4, 0.0), R, V + dv, w)
            e = np.cross(ax, (0.0, 0.0, 1.0))
            e *= _REGIME_ARM[name] / np.linalg.norm(e)
            rows += [(va, b, -e), (vb, b, e)]
        else:
            motions[b] = an.motion32(_CENTRE + (0.01 * b, -0.01, 0.02), R, V + dv, w)
            for k in range(12):
                v = (b % 2) * NV + (3 + 6 * (k % 4)) * N + 2 + 3 * b + 8 * (k // 4)
                rows.append((v, b, _p_BQ(motions[b], X[v])))
    return dict(name="regimes", cloths=cloths, X=X, v0=v0, table=make_table(rows), motions=motions, n_bodies=8, dt=DT, densities=None)


def regime_angles(lay):
    """{body: |w| (0 + dt)} of the regimes layout, from the float32 values the engine is given"""
    dt64 = float(np.float32(lay["dt"]))
    return {b: float(np.linalg.norm(m[3].astype(np.float64))) * dt64 for b, m in lay["motions"].items()}


# clocks: (what, argument) in order; a substep is (dt, the entry point that runs it)
CLOCK_BODIES = 18
CLOCK_EARLY, CLOCK_RESET = 10, 3
CLOCK_STEPS = ((1e-3, "phases"), (5e-4, "substep"), (7.5e-4, "run")), ((2.5e-4, "phases"), (1e-3, "run")), ((5e-4, "substep"), (1.25e-4, "phases"))


def layout_clocks():
    """18 bodies with four pins each on two sheets at rest.  Schedule: motions of bodies 0 .. 9 and their pins; three
    substeps of unequal dt; motions of bodies 10 .. 17 (the motion table grows past its 16 slots) and all pins; two
    substeps; body 3's motion set again, from where it is now with another velocity; two substeps.  `expected`: every
    body's clock at the end; `reset`: body 3's second motion."""
    cloths = _sheets(_UA, _UB)
    X = np.concatenate([c[0] for c in cloths])
    motions, rows = {}, []
    for b in range(CLOCK_BODIES):
        ax = (1 + b % 3, 2 - b % 5, 3 - b % 4)
        motions[b] = an.motion32(_CENTRE + (0.004 * (b % 5), -0.003 * (b % 4), 0.02), an._rot(ax, 0.1 + 0.05 * b),
                                 0.01 * np.asarray([(b % 3) - 1, (b % 4) - 1.5, 2 - (b % 5)]), (0.2 + 0.1 * b) * np.asarray(ax) / np.linalg.norm(ax))
    for k in range(4 * CLOCK_BODIES):
        v, b = 7 * k + 3 + (NV if k % 2 else 0), k % CLOCK_BODIES
        rows.append((v, b, _p_BQ(motions[b], X[v])))
    s1, s2, s3 = ([d for d, _ in part] for part in CLOCK_STEPS)
    t_reset = clock_after(s1 + s2)
    pt, Rt, _, _, _ = an.pose64(motions[CLOCK_RESET], t_reset)
    reset = an.motion32(pt, Rt, (-0.02, 0.03, 0.01), (0.5, -0.3, 0.4))
    expected = {b: clock_after(s1 + s2 + s3) if b < CLOCK_EARLY else clock_after(s2 + s3) for b in range(CLOCK_BODIES)}
    expected[CLOCK_RESET] = clock_after(s3)
    final = dict(motions)
    final[CLOCK_RESET] = reset
    return dict(name="clocks", cloths=cloths, X=X, v0=np.zeros_like(X), table=make_table(rows), motions=motions, reset=reset, final=final,
                expected=expected, n_bodies=CLOCK_BODIES, dt=None, densities=None)


# tile_fit: the pinned vertices in grid coordinates u = x * dxinv - .5
_TA, _TB = (1.0, 1.0, 1.5), (49.0, 25.0, 30.5)
EPS = 2.0 ** -10


def layout_tile_fit():
    """Two sheets at rest, zero gravity (k_g2p alone leaves need_rebuild at 0), body 0 still at the origin with the
    identity as R_WB: a target is its p_BQ to the bit.  Three pins hold their vertices where they are: vertex 0 of sheet
    A at u = (1, 1, 1.5), block (0, 0, 0); the vertex of sheet B at u = (61, 25, 30.5), block 15 along x; and the vertex of
    sheet B at u = (51, 31, 30.5), block (12, 7, 7), whose fit box [4 b - 2 + 1/8, 4 b + 6 - 1/8) lies inside the domain.
    `variants`: (name, pin, target u, left, outside): one pin's target moved to a face of the last vertex's fit box, or
    to the domain's limit 0 (first vertex) or 62 (second), at -+ 2^-10 cell."""
    cloths = _sheets(_TA, _TB)
    X = np.concatenate([c[0] for c in cloths])
    vs = [0, NV + 24 * N, NV + 4 * N + 12]
    us = [np.asarray(_TA), np.asarray(_TB) + (12.0, 0, 0), np.asarray(_TB) + (2.0, 6.0, 0)]
    for v, u in zip(vs, us):
        assert np.array_equal(X[v], _x_of(u).astype(np.float32))
    motions = {0: an.motion32((0, 0, 0), np.eye(3), (0, 0, 0), (0, 0, 0))}
    table = make_table([(v, 0, X[v]) for v in vs])
    variants = [("fits", 0, us[0], False, False)]
    blk = block_of(X[vs[2]])
    for a in range(3):
        lo, hi = 4 * blk[a] - FREE_ZONE + GUARD, 4 * blk[a] - FREE_ZONE + TILE_W - 2 - GUARD
        for name, thr, sides in (("lower", lo, ((-EPS, True), (EPS, False))), ("upper", hi, ((-EPS, False), (EPS, True)))):
            for d, left in sides:
                u = us[2].copy()
                u[a] = thr + d
                variants.append((f"{name} face {'xyz'[a]} {d:+.0e}", 2, u, left, False))
    for name, pin, thr, sides in (("domain 0", 0, 0.0, ((-EPS, True), (EPS, False))), ("domain 62", 1, 62.0, ((-EPS, False), (EPS, True)))):
        for d, out in sides:
            u = us[pin].copy()
            u[0] = thr + d
            variants.append((f"{name} {d:+.0e}", pin, u, out, out))
    return dict(name="tile_fit", cloths=cloths, X=X, v0=np.zeros_like(X), table=table, motions=motions, n_bodies=1, dt=DT,
                densities=None, variants=variants, material=dict(gravity=0.0))


def tile_fit_table(lay, variant):
    """the layout's table with the variant's pin moved to its target"""
    _, pin, u, _, _ = variant
    t = lay["table"].copy()
    t["p_BQ"][pin] = _x_of(u).astype(np.float32)
    assert np.array_equal(t["p_BQ"][pin].astype(np.float64), _x_of(u))      # (2^-10 cell is a float32 value)
    return t


LAYOUTS = dict(many=layout_many, regimes=layout_regimes, materials=layout_materials, clocks=layout_clocks, tile_fit=layout_tile_fit)
_LAYOUT = {}


def layout(name):
    if name not in _LAYOUT:
        _LAYOUT[name] = LAYOUTS[name]()
    return _LAYOUT[name]


def cloth_of(lay, vertices):
    return (np.asarray(vertices) >= NV).astype(int)


def stand_in_mass(lay, other=False):
    """per pin, for the self-test only: a vertex's share of a sheet H0 x H0 x 1e-3 at 1000 kg/m^3 times its cloth's
    density factor; `other`: the other cloth's factor"""
    d = lay["densities"] or (1.0, 1.0)
    c = cloth_of(lay, lay["table"]["vertex"])
    return (1000.0 * 1e-3 * H0 * H0 * np.asarray(d)[1 - c if other else c]).astype(np.float32).astype(np.float64)


def coverage(lay):
    t = lay["table"]
    n = len(t)
    group = np.arange(n) // GROUP
    return dict(n=n, groups=(n + GROUP - 1) // GROUP, bodies=sorted(set(t["body"].tolist())),
                groups_of={int(b): sorted(set(group[t["body"] == b].tolist())) for b in np.unique(t["body"])},
                monotone=bool(np.all(np.diff(t["vertex"].astype(np.int64)) > 0)), cloths=sorted(set(cloth_of(lay, t["vertex"]).tolist())))
