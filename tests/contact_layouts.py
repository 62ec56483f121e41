"""Contact layouts that reach the branches of the grid-space contact solve (k_ct_prepare, k_ct_tile, k_ct_node_dir, k_ct_ls,
k_ct_decide, k_ct_apply and k_ct_impulse of drake_amd/csrc/mpm_contact_dev.h), float64 restatements of each phase in the
world frame, and per-contact / per-node / per-body rounding bounds.  CPU only: nothing here imports the engine.

Layouts
-------
Particles are small disconnected triangles (tests/transfer_layouts.py: _Mesh, cell keys, stencils, fixed-point scales),
rest shape = uploaded shape, single material (the oracle's contact mass is vol * density).  Every field of every contact
pair is chosen here and uploaded with mpm_copy_contact_pairs; the contact position is always the particle's own position
(what the driver produces: its base cell is on the active grid), and dist < 0.  `claims` lists what a layout is built to
reach; tests/test_contact_layouts.py checks every claim with the restatement.

    normals    unit normals uniform on the sphere, the 6 axes, the 8 body diagonals, normals whose two smallest components
               tie (the index choice of frame_from_normal), normals within 1e-4 .. 1e-3 rad of an axis
    regimes_*  >= 100 contacts in each regime: separating (v0_n > v_hat, clear of it), approaching and sliding
               (|v_t| >= 100 epsv), sticking (|v_t| <= 0.01 epsv: rigid_v matches the particle's tangential velocity) and
               transitional (|v_t| ~ epsv); parameter sets soft, config3, mu = 0, d = 0, and `damped` (d = 1, half of the
               contacts with phi0 > dt: v_hat = 1/d)
    bodies     40 bodies: ids 0-31 take k_ct_impulse's LDS accumulators, 32-39 the device-scope atomics; every body has its
               own p_WB 20 - 30 cells from its contacts and a rigid point velocity v_B + w_B x (x - p_WB); a third of the
               particles are in contact with two bodies, a sixth with three (the same particle and cell under other frames)
    occupancy  cells holding n contacts for every n of transfer_layouts.RUNS (1 .. 1000; cells across 64-contact tiles),
               a block with one contact in each of its 64 cells, blocks with 2 contacts in 8 / 16 cells, 6 in 22 (tiles of
               1, 2-8, 9-16 and 17-64 segments: every subset count S of k_ct_tile and 1 - 4 CT_STAGE rounds), a 3 x 3 x 3
               group of occupied cells (a node reached from all 27 base cells: lanes sub and sub + 16 of k_ct_node_dir)
    fringe     light particles and far-corner weights (stencil nodes with 0 < m <= 1e-7, dropped by the gathers and kept by
               k_ct_ls), nodes reached by separated contacts only (direction exactly zero, no DoF), contact masses over
               six decades (nodes on both sides of the 1e-7 DoF threshold), contacts at base cells 0 and hi = 2^bits - 3
               (the wall band)

Restatements (float64, numpy; each phase on the engine's own inputs: GRID_MASSES, the grid velocity after UpdateGrid
(GRID_MOMENTUM), GRID_V_STAR, the particle velocities and MASSES, the pairs as uploaded)
----------------------------------------------------------------------------------------------------------------------
No contact frame: with n = -normal, u = v - rigid_v, u_t = (I - n n^T) u, ts = sqrt(|u_t|^2 + epsv^2), tau = u_t / ts and
co = -mu yn0 / ts, the contact-frame Hessian and gradient of contact_grad_hess are, in the world frame,
    H = co (I - n n^T - tau tau^T) + d2n n n^T,      G = -mu yn0 tau + yn n
(invariant under the choice of tangents, so the restatement cannot inherit a mistake of frame_from_normal).
    setup      base cell, 27 nodes and weights, contact mass, vel0 = sum w v_n over the nodes with m > 1e-7
    direction  H_n = sum m w^2 H, G_n = sum m w G; D = relax (H_n - m_n I)^-1 (G_n - m_n (v - v*)) where m_n > 0 and
               |H_n|_F or |G_n| exceeds 1e-7; H and G at the particle velocity in iteration 1 (CopyContactPairs), at the
               velocity gathered over m > 1e-7 from the grid later
    energy     E(a) = sum_c m_c l_c(v~_c - a d_c) + sum_n 1/2 m_n |v - v* - a D|^2, v~ and d gathered over every stencil
               node (k_ct_ls), the inertia sum over the nodes that see contacts; dE and d2E as the exact search forms them
    impulse    per body f = sum m (vel0 - v), tau = sum (x - p_WB) x m (vel0 - v), v gathered from the final grid

Bounds (u = 2^-24; first-order rounding bounds of the float arithmetic, times K = 2 for the second-order terms)
--------------------------------------------------------------------------------------------------------------
Per contact, the relative velocity the kernel forms (v - rigid_v, then three-term frame products) is off by at most
du = 8 u (|v|_1 + |rigid_v|_1) + the gather bound of v, so every quantity is bounded by its own rounding plus its
sensitivity to du -- the cancellations in phi0 - dt v_n, in 1 - d v_n and in tau = u_t / ts (sticking: |u_t| << epsv while
|v| is not) are covered that way, not by the magnitude of the result:
    e_yn  = k dt [(dt (1 + d|v_n|) + d (|phi0| + dt |v_n|)) du + 8 u (|phi0| + dt |v_n|)(1 + d |v_n|)]
    e_d2n = k dt [2 d dt du + 8 u (dt + d |phi0| + 2 d dt |v_n|)],   e_yn0 = k dt |phi0| [d du0 + 8 u (1 + d |v0_n|)]
    e_tau = 3 du / ts + 8 u,   e_co = mu e_yn0 / ts + |co| (3 du / ts + 8 u)
    e_H   = 2 e_co + 3 |co| e_tau + e_d2n + 16 u (2 |co| + |d2n|)          (every world entry)
    e_G   = mu (e_yn0 + yn0 e_tau) + e_yn + 16 u (mu yn0 + |yn|)
Per node:  |H_n - H64_n| <= K sum_c m w^2 (e_H + (L_n + 16) u M_H),  |G_n - G64_n| <= K sum_c m w (e_G + (L_n + 16) u M_G)
    with M_H = 2 |co| + |d2n|, M_G = mu yn0 + |yn|, and L_n the length of the float chain: the longest segment (contacts of
    one cell inside one 64-contact tile) whose stencil reaches n, plus 8 (the subset sums of k_ct_tile), plus the segments
    that reach n, plus 4 (the butterfly of k_ct_node_dir's 16 lanes).  The float oracle adds sequentially: L_n = N_n.
Direction: A = H_n - m_n I, b = G_n - m_n (v - v*), d = A^-1 b:
    |d - d64| <= K [|A^-1| (E_A |d| + e_b) + 24 u cond(A) |d|],  cond(A) = max row sum of |A^-1| |A|  (inv33 and the
    product), and |D - D64| <= relax |d - d64| + u |D|.
Energies: per contact e_l = m [mu e_yn0 (ts - epsv) + mu yn0 (|u_t| / ts du_t + 8 u (ts + epsv)) + s_n du_n + 8 u
    (|a| |v_n|^3 / 3 + |b| v_n^2 / 2 + |c| |v_n|)] + 3 u m |l| with s_n = |a| v_n^2 + |b| |v_n| + |c| (the slope of the
    normal cost); per node e = m |n| . (|o| u + 2 u (|n| + a |D|)) + 2 u m |n|^2; summed in double (1e-14 of the sum of
    magnitudes), and the float the decision compares (u |E|).  Times K.
Impulses: the gather bounds of vel0 and v (K (27 + 16) u sum w |v_n|), the roundings of m (vel0 - v), x - p_WB and the
    cross product, plus half a fixed-point quantum per term (imp_fix = DP::fix_p = 2^(61 - ceil(log2 M) - 14) with M the
    total mass: transfer_layouts.fixed_quanta) and half an ulp of the float result.
The bounds hold with and without fused multiply-adds (every product-sum above is bounded by magnitudes, not by an
evaluation order).  Decisions within their bound of a threshold are excluded from the decision assertions: the
separated test (none by construction, a claim), the DoF threshold (`amb` nodes: direction and DoF count not asserted
there, the count bracketed), and the Armijo test E(a) <= E0 (the candidate's decision is then free).
"""
import numpy as np

from tests import transfer_layouts as tl

U32 = 2.0 ** -24
K = 2.0
BITS = 6
EPSV = float(np.float32(1e-3))
RELAX = 0.3
THRESH = 1e-7              # k_ct_node_dir's DoF threshold and the gathers' node-mass threshold
GATHER = K * (27 + 16) * U32
# (stiffness, damping, dt): tests/test_contact_gpu.py's CONTACT_PARAMS
CONTACT_PARAMS = {"soft": (1e5, 1e-3, 1e-3), "config3": (1e6, 1e-5, 2e-4)}
# per layout: (stiffness, damping, dt, mu)
PARAM_SETS = {
    "soft": CONTACT_PARAMS["soft"] + (0.5,),
    "config3": CONTACT_PARAMS["config3"] + (1.0,),
    "mu0": CONTACT_PARAMS["soft"] + (0.0,),
    "d0": (1e5, 0.0, 1e-3, 0.5),
    "damped": (1e5, 1.0, 1e-3, 0.5),
}


def f32v(x):
    return float(np.float32(x))


def params32(name):
    """the parameter set as the engine holds it (float32)"""
    return tuple(f32v(x) for x in PARAM_SETS[name])


def _unit(a):
    a = np.asarray(a, np.float64)
    return a / np.linalg.norm(a, axis=-1, keepdims=True)


# ---- builders ------------------------------------------------------------------------------------------------------
class _Layout:
    def __init__(self, name, seed, params):
        self.name, self.params = name, params
        self.M = tl._Mesh(BITS, seed)
        self.rng = self.M.rng
        self.tvol = []            # per triangle: volume scale
        self.contacts = []        # (triangle, corner 0..3 (3 = face), normal, dist, rigid_v or None, body, p_WB, u_rel)

    def tri(self, centre, size=0.3, vel=None, vol=1.0):
        self.M.small(centre, size, vel)
        self.tvol.append(vol)
        return self.M.n() - 1

    def contact(self, t, corner, normal, dist, u_rel=None, rigid_v=None, body=0, p_WB=(0.0, 0.0, 0.0)):
        """u_rel: the particle's velocity relative to the body (rigid_v = v_particle - u_rel); else rigid_v"""
        self.contacts.append((t, corner, np.asarray(normal, np.float64), float(dist), u_rel, rigid_v, body,
                              np.asarray(p_WB, np.float64)))

    def finish(self, claims, n_bodies=1):
        M = self.M
        nt = M.n()
        dx = 1.0 / (1 << BITS)
        xv = tl.f32(np.concatenate(M.verts) * dx)
        vv = tl.f32(np.concatenate(M.vvel))
        idx = np.arange(3 * nt, dtype=np.int32).reshape(nt, 3)
        cen = ((xv[idx[:, 0]] + xv[idx[:, 1]]) + xv[idx[:, 2]]) / np.float32(3)
        cvel = ((vv[idx[:, 0]] + vv[idx[:, 1]]) + vv[idx[:, 2]]) / np.float32(3)
        pos, vel = np.concatenate([cen, xv]), np.concatenate([cvel, vv])
        n = 4 * nt
        tv = np.asarray(self.tvol)
        vol = np.concatenate([tv, np.repeat(tv, 3)]) * 1e-8 * self.rng.uniform(0.5, 1.5, n)
        vol = tl.f32(vol)
        mass = tl.f32(vol * np.float32(2000.0))
        pid, body, dist, normal, rv, pwb = [], [], [], [], [], []
        for t, corner, nrm, d, u_rel, rigid_v, b, p in self.contacts:
            i = t if corner == 3 else nt + 3 * t + corner
            pid.append(i)
            body.append(b)
            dist.append(d)
            normal.append(nrm)
            rv.append(vel[i].astype(np.float64) - u_rel if u_rel is not None else rigid_v)
            pwb.append(p)
        pid = np.asarray(pid, np.uint32)
        return dict(name=self.name, bits=BITS, params=self.params, cloths=[(xv, vv, idx)], nf=nt, nv=3 * nt, pos=pos,
                    vel=vel, C=np.zeros((n, 9), np.float32), vol=vol, mass=mass, gravity_axis=2, claims=claims,
                    n_bodies=n_bodies,
                    cp=dict(particle=pid, body=np.asarray(body, np.uint32), dist=tl.f32(dist), normal=tl.f32(normal),
                            pos=pos[pid].copy(), rigid_v=tl.f32(rv), p_WB=tl.f32(pwb)))


def _sphere(rng, n):
    return _unit(rng.normal(size=(n, 3)))


def _tangent(rng, nrm, mag):
    """a vector perpendicular to nrm (unit, world) of length mag"""
    t = np.cross(nrm, rng.normal(size=3))
    return _unit(t) * mag


def _centre(rng, lo=20.0, hi=44.0):
    return rng.uniform(lo, hi, 3)


def normals(seed=11):
    L = _Layout("normals", seed, "soft")
    special = [np.eye(3)[i] * s for i in range(3) for s in (1, -1)]
    special += [np.array([sx, sy, sz]) for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)]
    for i in range(3):                       # the two smallest components tie
        for s in (1, -1):
            v = np.full(3, 0.3 * s)
            v[i] = 1.0
            special.append(v)
            v = np.full(3, 0.7)
            v[i] = 0.2 * s
            special.append(v)
    near = []
    for i in range(3):                       # within 1e-4 .. 1e-3 rad of an axis
        for s in (1, -1):
            for eps in (1e-4, 3e-4, 1e-3):
                v = np.eye(3)[i] * s
                v = v + _tangent(L.rng, v, np.tan(eps))
                near.append(v)
    nrms = [_unit(v) for v in special + near]
    nrms += list(_sphere(L.rng, 400))
    for k, nrm in enumerate(nrms):
        t = L.tri(_centre(L.rng), 0.3, L.rng.uniform(-0.3, 0.3, 3))
        u = -nrm * L.rng.uniform(0.05, 0.4) + _tangent(L.rng, nrm, L.rng.uniform(0.1, 0.4))   # approaching, sliding
        # (v_n = n . u with n = -normal: u along -normal approaches)
        L.contact(t, k % 4, nrm, -L.rng.uniform(2e-4, 6e-3), u_rel=-u)
    return L.finish(dict(normals=len(nrms), special=len(special), near_axis=len(near)))


REGIMES = ("separating", "sliding", "sticking", "transitional")


def regimes(pset, seed=12):
    L = _Layout(f"regimes_{pset}", seed + len(pset), pset)
    k, d, dt, mu = params32(pset)
    for q in range(4 * 130):
        reg = REGIMES[q % 4]
        nrm = _sphere(L.rng, 1)[0]
        n = -nrm
        phi0 = L.rng.uniform(2e-4, 2e-3) if pset != "damped" or q % 8 < 4 else L.rng.uniform(2.5e-3, 6e-3)
        vhat = min(phi0 / dt, 1.0 / d if d > 0 else np.inf)
        if reg == "separating":
            vn, vt = vhat * L.rng.uniform(1.2, 2.0) + 0.01, L.rng.uniform(0.0, 0.3)
        else:
            vn = -L.rng.uniform(0.02, 0.4)
            vt = {"sliding": L.rng.uniform(100 * EPSV, 0.4), "sticking": L.rng.uniform(0.0, 0.005 * EPSV),
                  "transitional": EPSV * L.rng.uniform(0.3, 3.0)}[reg]
        u = vn * n + _tangent(L.rng, n, vt)
        t = L.tri(_centre(L.rng), 0.3, L.rng.uniform(-0.5, 0.5, 3))
        L.contact(t, q % 4, nrm, -phi0, u_rel=u)
    return L.finish(dict(regimes=REGIMES, pset=pset))


def bodies(seed=13):
    L = _Layout("bodies", seed, "soft")
    nb = 40
    c0 = np.array([0.5, 0.5, 0.5])
    pw = c0 + _sphere(L.rng, nb) * L.rng.uniform(20, 30, (nb, 1)) / (1 << BITS)
    vb, wb = L.rng.uniform(-0.3, 0.3, (nb, 3)), L.rng.uniform(-2.0, 2.0, (nb, 3))
    ntri = 160
    q = 0
    for i in range(ntri):
        t = L.tri(_centre(L.rng, 26, 38), 0.3, L.rng.uniform(-0.3, 0.3, 3))
        for corner in range(4):
            nb_here = 3 if (4 * i + corner) % 6 == 0 else (2 if (4 * i + corner) % 3 == 0 else 1)
            for _ in range(nb_here):
                b = q % nb
                q += 1
                # (the rigid velocity at the particle's position; the contact's relative velocity follows from it)
                L.contact(t, corner, _sphere(L.rng, 1)[0], -L.rng.uniform(2e-4, 4e-3), rigid_v=np.zeros(3), body=b,
                          p_WB=pw[b])
    lay = L.finish(dict(bodies=nb, lds_bodies=32, multi_body_particles=True), n_bodies=nb)
    # rigid point velocities v_B + w_B x (x - p_WB) at the contact positions
    x = lay["cp"]["pos"].astype(np.float64)
    b = lay["cp"]["body"].astype(np.int64)
    lay["cp"]["rigid_v"] = tl.f32(vb[b] + np.cross(wb[b], x - pw[b]))
    return lay


def occupancy(seed=14):
    L = _Layout("occupancy", seed, "soft")

    def fill(cell, n, vel):
        """n contacts whose base cell is `cell` (triangles inside the cell: u in [b + 0.7, b + 1.3])"""
        for j in range((n + 3) // 4):
            t = L.tri(np.asarray(cell, np.float64) + 1.0, 0.28, vel)
            for corner in range(min(4, n - 4 * j)):
                nrm = _sphere(L.rng, 1)[0]
                L.contact(t, corner, nrm, -L.rng.uniform(2e-4, 4e-3),
                          u_rel=-nrm * 0.2 + _tangent(L.rng, nrm, L.rng.uniform(0.0, 0.2)))
    runs = {}
    for i, n in enumerate(tl.RUNS):
        cell = (4 * (2 + 3 * (i % 4)) + 1, 4 * (2 + 3 * (i // 4)) + 1, 4 * 3 + 1)
        fill(cell, n, L.rng.uniform(-0.2, 0.2, 3))
        runs[n] = cell
    # one contact in each of the 64 cells of block (10, 10, 10); two in 8 and in 16 cells of two more blocks
    for c in range(64):
        fill((40 + c // 16, 40 + (c // 4) % 4, 40 + c % 4), 1, L.rng.uniform(-0.2, 0.2, 3))
    for blk, ncell in (((10, 10, 2), 8), ((10, 2, 10), 16)):
        for c in range(ncell):
            fill((4 * blk[0] + c // 4, 4 * blk[1] + c % 4, 4 * blk[2] + 1), 2, L.rng.uniform(-0.2, 0.2, 3))
    # six contacts in each of 22 cells of one block: a tile of 10 - 12 segments lies inside them
    for c in range(22):
        fill((8 + c // 16, 40 + (c // 4) % 4, 40 + c % 4), 6, L.rng.uniform(-0.2, 0.2, 3))
    # a 3 x 3 x 3 group of occupied cells: its centre + (1, 1, 1) ... every node of the middle is reached from 27 cells
    for c in range(27):
        fill((20 + c // 9, 44 + (c // 3) % 3, 44 + c % 3), 3, L.rng.uniform(-0.2, 0.2, 3))
    return L.finish(dict(runs=runs, all27=(22, 46, 46)))


def fringe(seed=15):
    L = _Layout("fringe", seed, "soft")
    hi = (1 << BITS) - 3

    def approach(nrm):
        return -nrm * L.rng.uniform(0.05, 0.3) + _tangent(L.rng, nrm, L.rng.uniform(0.0, 0.3))

    # light isolated triangles: every one of their stencil nodes is light; far-corner weights (u - b near 1.45)
    for q in range(40):
        c = np.array([8 + 5 * (q % 8), 8 + 5 * (q // 8), 30.0]) + (0.45 if q % 2 else 0.0)
        t = L.tri(c, 0.04, L.rng.uniform(-0.2, 0.2, 3), vol=10.0 ** L.rng.uniform(-6, -2))
        for corner in range(4):
            nrm = _sphere(L.rng, 1)[0]
            L.contact(t, corner, nrm, -L.rng.uniform(2e-4, 4e-3), u_rel=approach(nrm))
    # contact masses over six decades in a shared region: nodes on both sides of the 1e-7 DoF threshold
    for q in range(120):
        t = L.tri(_centre(L.rng, 40, 50), 0.3, L.rng.uniform(-0.2, 0.2, 3), vol=10.0 ** L.rng.uniform(-6, 0))
        nrm = _sphere(L.rng, 1)[0]
        L.contact(t, q % 4, nrm, -L.rng.uniform(1e-5, 4e-3), u_rel=approach(nrm))
    # triangles whose contacts all separate (their nodes see separated contacts only)
    for q in range(30):
        t = L.tri(np.array([12 + 4 * (q % 6), 50 + 4 * (q // 6) % 12, 12.0]), 0.3, L.rng.uniform(-0.2, 0.2, 3))
        for corner in range(4):
            nrm = _sphere(L.rng, 1)[0]
            phi0 = L.rng.uniform(2e-4, 2e-3)
            L.contact(t, corner, nrm, -phi0, u_rel=-nrm * (phi0 / 1e-3 * 1.5 + 0.05))
    # wall band and the base-cell clamp: base cells 0 and hi on every axis
    for q in range(16):
        side = np.array([(q >> a) & 1 for a in range(3)])
        c = np.where(side == 1, hi + 1.0, 1.0) + L.rng.uniform(-0.15, 0.15, 3)
        t = L.tri(c, 0.25, L.rng.uniform(-0.3, 0.3, 3))
        for corner in range(4):
            nrm = _sphere(L.rng, 1)[0]
            L.contact(t, corner, nrm, -L.rng.uniform(2e-4, 4e-3), u_rel=approach(nrm))
    return L.finish(dict(light=True, separated_only=True, threshold=True, walls=True))


BUILDERS = {
    "normals": normals,
    "regimes_soft": lambda: regimes("soft"),
    "regimes_config3": lambda: regimes("config3"),
    "regimes_mu0": lambda: regimes("mu0"),
    "regimes_d0": lambda: regimes("d0"),
    "regimes_damped": lambda: regimes("damped"),
    "bodies": bodies,
    "occupancy": occupancy,
    "fringe": fringe,
}
NAMES = tuple(BUILDERS)
_CACHE = {}


def layout(name):
    if name not in _CACHE:
        _CACHE[name] = BUILDERS[name]()
    return _CACHE[name]


# ---- restatements --------------------------------------------------------------------------------------------------
def stencil(lay):
    """per contact: base cell (nc, 3), weights (nc, 27), dense node keys (nc, 27)"""
    b, fx, wt, keys = tl._stencil(lay["cp"]["pos"], lay["bits"])
    return b, wt, keys


def gather(wt, keys, gv, gm=None, eb=True):
    """sum w v_n per contact (over nodes with m > 1e-7 when gm is given) and its bound"""
    g = np.asarray(gv, np.float64).reshape(-1, 3)[keys]
    w = wt if gm is None else np.where(np.asarray(gm)[keys] > THRESH, wt, 0.0)
    v = np.einsum("cn,cnr->cr", w, g)
    return v, GATHER * np.einsum("cn,cnr->cr", w, np.abs(g))


def contact_terms(lay, P, v, vp, ev=None):
    """world-frame H (nc, 3, 3), G (nc, 3) of every contact at contact velocity v, lagged (particle) velocity vp;
    per-entry bounds eH, eG and magnitudes MH, MG (docstring); ev: a bound on the error of v (per contact)"""
    k, d, dt, mu = P
    cp = lay["cp"]
    n = -_unit(cp["normal"])
    rv = cp["rigid_v"].astype(np.float64)
    phi0 = -cp["dist"].astype(np.float64)
    u, u0 = v - rv, vp - rv
    vn, v0n = np.einsum("ci,ci->c", u, n), np.einsum("ci,ci->c", u0, n)
    with np.errstate(divide="ignore"):
        vhat = np.minimum(phi0 / dt, (1.0 / d) if d > 0 else np.inf)
    sep = v0n > vhat
    ut = u - vn[:, None] * n
    ts = np.sqrt(np.einsum("ci,ci->c", ut, ut) + EPSV * EPSV)
    tau = ut / ts[:, None]
    yn0 = np.maximum(k * dt * phi0 * (1.0 - d * v0n), 0.0)
    yn = k * dt * (phi0 - dt * vn) * (1.0 - d * vn)
    d2n = k * dt * (-dt - d * phi0 + 2.0 * d * dt * vn)
    co = -mu * yn0 / ts
    I3 = np.eye(3)[None]
    nn = np.einsum("ci,cj->cij", n, n)
    H = co[:, None, None] * (I3 - nn - np.einsum("ci,cj->cij", tau, tau)) + d2n[:, None, None] * nn
    G = -mu * yn0[:, None] * tau + yn[:, None] * n
    H[sep], G[sep] = 0.0, 0.0
    du = 8 * U32 * (np.abs(v).sum(1) + np.abs(rv).sum(1)) + (0.0 if ev is None else 3.0 * np.abs(ev).max(1))
    du0 = 8 * U32 * (np.abs(vp).sum(1) + np.abs(rv).sum(1))
    avn, av0n, aphi = np.abs(vn), np.abs(v0n), np.abs(phi0)
    e_yn = k * dt * ((dt * (1 + d * avn) + d * (aphi + dt * avn)) * du + 8 * U32 * (aphi + dt * avn) * (1 + d * avn))
    e_d2n = k * dt * (2 * d * dt * du + 8 * U32 * (dt + d * aphi + 2 * d * dt * avn))
    e_yn0 = k * dt * aphi * (d * du0 + 8 * U32 * (1 + d * av0n))
    e_tau = 3 * du / ts + 8 * U32
    e_co = mu * e_yn0 / ts + np.abs(co) * (3 * du / ts + 8 * U32)
    MH, MG = 2 * np.abs(co) + np.abs(d2n), mu * yn0 + np.abs(yn)
    eH = 2 * e_co + 3 * np.abs(co) * e_tau + e_d2n + 16 * U32 * MH
    eG = mu * (e_yn0 + yn0 * e_tau) + e_yn + 16 * U32 * MG
    for a in (eH, eG, MH, MG):
        a[sep] = 0.0
    # how far the separated test is from flipping: |v0_n - v_hat| against the error of v0_n and of v_hat
    sep_margin = np.abs(v0n - vhat) / (du0 + 4 * U32 * np.where(np.isfinite(vhat), np.abs(vhat), 0.0) + 1e-300)
    return dict(H=H, G=G, eH=eH, eG=eG, MH=MH, MG=MG, sep=sep, sep_margin=sep_margin, vn=vn, v0n=v0n, vhat=vhat,
                ut=np.linalg.norm(ut, axis=1), phi0=phi0, yn0=yn0, e_yn0=e_yn0, ts=ts, du=du)


def chain_lengths(keys, sequential=False, received=None):
    """L_n per node of `nodes` (docstring): segments = contacts of one base cell inside one tile of 64 contacts in the
    solve's order (ascending cell key, stable); the float oracle's sequential sums: N_n.  received: dense keys of the
    nodes whose sums take one more float addition (a partitioned domain adds the neighbour's sums there): L_n + 1"""
    base = keys[:, 0]
    order = np.argsort(base, kind="stable")
    sk = base[order]
    pos_in = np.empty(len(base), np.int64)
    pos_in[order] = np.arange(len(base))
    seg_id = np.zeros(len(base), np.int64)
    tile = np.arange(len(base)) // 64
    new = np.r_[True, (sk[1:] != sk[:-1]) | (tile[1:] != tile[:-1])]
    sid = np.cumsum(new) - 1
    seg_len = np.bincount(sid)
    seg_id[order] = sid
    nodes, inv = np.unique(keys, return_inverse=True)
    inv = inv.reshape(keys.shape)
    N = np.bincount(inv.reshape(-1), minlength=len(nodes)).astype(np.float64)
    more = 0.0 if received is None else np.isin(nodes, np.asarray(received)).astype(np.float64)
    if sequential:
        return nodes, inv, N + more, N
    longest = np.zeros(len(nodes))
    np.maximum.at(longest, inv.reshape(-1), np.repeat(seg_len[seg_id], 27).astype(np.float64))
    # segments per node: distinct (node, segment) pairs
    pairs = np.unique(inv.reshape(-1) * (sid.max() + 1) + np.repeat(seg_id, 27))
    nseg = np.bincount(pairs // (sid.max() + 1), minlength=len(nodes)).astype(np.float64)
    return nodes, inv, longest + 8 + nseg + 4 + more, N


def direction(lay, P, wt, keys, mass_c, T, gm, gv, gvs, relax=RELAX, sequential=False, ev_grid=0.0, received=None):
    """node sums, DoFs and the relaxed direction at the nodes that see contacts (dense keys `nodes`), with bounds;
    received: chain_lengths' (the nodes of a partitioned domain that add a neighbour's sums)"""
    nodes, inv, L, N = chain_lengths(keys, sequential, received)
    nn = len(nodes)
    m = np.asarray(mass_c, np.float64)[:, None]
    f = inv.reshape(-1)
    Hn = np.zeros((nn, 9))
    Gn = np.zeros((nn, 3))
    w2m = (m * wt * wt).reshape(-1)
    wm = (m * wt).reshape(-1)
    np.add.at(Hn, f, (w2m[:, None] * np.repeat(T["H"].reshape(-1, 9), 27, axis=0)))
    np.add.at(Gn, f, (wm[:, None] * np.repeat(T["G"], 27, axis=0)))
    eHn, eGn = np.zeros(nn), np.zeros(nn)
    Ln = np.repeat(L[inv], 1, axis=1)   # (nc, 27)
    np.add.at(eHn, f, (m * wt * wt * (T["eH"][:, None] + (Ln + 16) * U32 * T["MH"][:, None])).reshape(-1))
    np.add.at(eGn, f, (m * wt * (T["eG"][:, None] + (Ln + 16) * U32 * T["MG"][:, None])).reshape(-1))
    eHn *= K
    eGn *= K
    mn = np.asarray(gm, np.float64)[nodes]
    v = np.asarray(gv, np.float64).reshape(-1, 3)[nodes]
    vs = np.asarray(gvs, np.float64).reshape(-1, 3)[nodes]
    hF, gF = np.linalg.norm(Hn, axis=1), np.linalg.norm(Gn, axis=1)
    eHF, eGF = 3.0 * eHn + 20 * U32 * hF, np.sqrt(3.0) * eGn + 20 * U32 * gF
    dof = (mn > 0) & ((hF > THRESH) | (gF > THRESH))
    amb = (mn > 0) & ((np.abs(hF - THRESH) <= eHF) | (np.abs(gF - THRESH) <= eGF)) & \
        ~((hF - eHF > THRESH) | (gF - eGF > THRESH))
    A = Hn.reshape(-1, 3, 3) - mn[:, None, None] * np.eye(3)[None]
    o = v - vs
    b = Gn - mn[:, None] * o
    d = np.zeros((nn, 3))
    eD = np.zeros((nn, 3))
    if dof.any():
        Ai = np.linalg.inv(A[dof])
        d[dof] = np.einsum("nij,nj->ni", Ai, b[dof])
        aAi = np.abs(Ai)
        eA = eHn[dof][:, None, None] * np.ones((1, 3, 3)) + U32 * np.abs(mn[dof])[:, None, None] * np.eye(3)[None]
        eb = eGn[dof][:, None] + mn[dof][:, None] * (2 * U32 * (np.abs(v[dof]) + np.abs(vs[dof])) + ev_grid) + \
            2 * U32 * np.abs(b[dof])
        cond = np.einsum("nij,njk->nik", aAi, np.abs(A[dof])).sum(2).max(1)
        ad = np.abs(d[dof])
        ed = np.einsum("nij,nj->ni", aAi, np.einsum("nij,nj->ni", eA, ad) + eb) + 24 * U32 * cond[:, None] * ad.max(1, keepdims=True)
        eD[dof] = K * relax * ed + U32 * relax * ad
    return dict(nodes=nodes, inv=inv, Hn=Hn, Gn=Gn, eHn=eHn, eGn=eGn, dof=dof, amb=amb, D=relax * d, eD=eD,
                nd=float((d[dof & ~amb] ** 2).sum()), mn=mn, o=o, hF=hF, gF=gF, L=L, N=N)


def _cost(P, T, w, eW):
    """contact cost l per contact at relative world velocity w (= v - rigid_v), with its bound (docstring)"""
    k, d, dt, mu = P
    cp = T["n"]
    vn = np.einsum("ci,ci->c", w, cp)
    ut = w - vn[:, None] * cp
    aut = np.linalg.norm(ut, axis=1)
    ts = np.sqrt(aut ** 2 + EPSV * EPSV)
    lt = mu * T["yn0"] * (ts - EPSV)
    vnc = np.minimum(T["vhat"], vn)
    a, b, c = k * d * dt * dt, -(k * dt * (dt + d * T["phi0"])), k * dt * T["phi0"]
    ln = -(a / 3 * vnc ** 3 + b / 2 * vnc ** 2 + c * vnc)
    dw = 3 * np.abs(eW).max(1) + 8 * U32 * np.abs(w).sum(1)
    avn = np.abs(vnc)
    slope = np.abs(a) * avn ** 2 + np.abs(b) * avn + np.abs(c)
    e = mu * T["e_yn0"] * (ts - EPSV) + mu * T["yn0"] * (aut / ts * dw + 8 * U32 * (ts + EPSV)) + slope * dw + \
        8 * U32 * (np.abs(a) * avn ** 3 / 3 + np.abs(b) * avn ** 2 / 2 + np.abs(c) * avn) + \
        8 * U32 * np.where(np.isfinite(T["vhat"]), np.abs(T["vhat"]), 0.0) * slope * (vn > T["vhat"])
    return lt + ln, e, vn, aut, ts


def line_search(lay, P, wt, keys, mass_c, T, gm, gv, gvs, gD, nodes, alphas, derivs=False, sequential=False, vp=None):
    """E(alpha) for every alpha (and dE, d2E) on the engine's grid velocity gv and direction gD; bounds per alpha"""
    cp = lay["cp"]
    rv = cp["rigid_v"].astype(np.float64)
    ov, eov = gather(wt, keys, gv)
    dd, edd = gather(wt, keys, gD)
    m = np.asarray(mass_c, np.float64)
    mn = np.asarray(gm, np.float64)[nodes]
    v = np.asarray(gv, np.float64).reshape(-1, 3)[nodes]
    vs = np.asarray(gvs, np.float64).reshape(-1, 3)[nodes]
    D = np.asarray(gD, np.float64).reshape(-1, 3)[nodes]
    on = mn > 0
    o = v - vs
    out = []
    nc = len(m)
    seq = (nc + on.sum()) * U32 if sequential else 1e-14
    for al in alphas:
        w = ov - rv - al * dd
        eW = eov + al * edd + 2 * U32 * (np.abs(ov) + np.abs(rv) + al * np.abs(dd))
        l, e, vn, aut, ts = _cost(P, T, w, eW)
        Ec = m * l
        eC = m * e + 3 * U32 * np.abs(Ec)
        nv = o - al * D
        Ei = 0.5 * mn * (nv ** 2).sum(1)
        eI = mn * (np.abs(nv) * (U32 * np.abs(o) + 2 * U32 * (np.abs(nv) + al * np.abs(D)))).sum(1) + 2 * U32 * np.abs(Ei)
        E = Ec.sum() + Ei[on].sum()
        A = np.abs(Ec).sum() + np.abs(Ei[on]).sum()
        r = dict(alpha=al, E=E, A=A, eE=K * (eC.sum() + eI[on].sum()) + seq * A + U32 * abs(E))
        if derivs:
            Tn = contact_terms(lay, P, w + rv, vp, eW)
            dEc = m * np.einsum("ci,ci->c", Tn["G"], dd)
            d2Ec = m * np.einsum("ci,cij,cj->c", dd, Tn["H"], dd)
            dEi = -mn * (nv * D).sum(1)
            d2Ei = mn * (D * D).sum(1)
            add = np.abs(dd).sum(1)
            e_dE = m * (Tn["eG"] * add + Tn["MG"] * 3 * np.abs(edd).max(1)) + 4 * U32 * np.abs(dEc)
            e_dEi = mn * (np.abs(D) * (U32 * np.abs(o) + 2 * U32 * (np.abs(nv) + al * np.abs(D)))).sum(1) + 4 * U32 * np.abs(dEi)
            r.update(dE=dEc.sum() + dEi[on].sum(), d2E=d2Ec.sum() + d2Ei[on].sum(),
                     edE=K * (e_dE.sum() + e_dEi[on].sum()) + 1e-14 * (np.abs(dEc).sum() + np.abs(dEi[on]).sum()))
        out.append(r)
    return out


def impulses(lay, wt, keys, gm, gv0, gv, mass_c, quantum=0.0, sequential=False):
    """per body (f, tau) from the pre-solve grid gv0 and the final grid gv, with bounds (docstring)"""
    cp = lay["cp"]
    v0, ev0 = gather(wt, keys, gv0, gm)
    v, ev = gather(wt, keys, gv, gm)
    m = np.asarray(mass_c, np.float64)[:, None]
    x, p = cp["pos"].astype(np.float64), cp["p_WB"].astype(np.float64)
    l = m * (v0 - v)
    r = x - p
    h = np.cross(r, l)
    el = m * (ev0 + ev) + 3 * U32 * m * (np.abs(v0) + np.abs(v))
    er = U32 * (np.abs(x) + np.abs(p))
    ar, al_ = np.abs(r), np.abs(l)
    eh = np.stack([ar[:, 1] * el[:, 2] + ar[:, 2] * el[:, 1] + er[:, 1] * al_[:, 2] + er[:, 2] * al_[:, 1],
                   ar[:, 2] * el[:, 0] + ar[:, 0] * el[:, 2] + er[:, 2] * al_[:, 0] + er[:, 0] * al_[:, 2],
                   ar[:, 0] * el[:, 1] + ar[:, 1] * el[:, 0] + er[:, 0] * al_[:, 1] + er[:, 1] * al_[:, 0]], 1)
    eh += 3 * U32 * np.stack([ar[:, 1] * al_[:, 2] + ar[:, 2] * al_[:, 1], ar[:, 2] * al_[:, 0] + ar[:, 0] * al_[:, 2],
                              ar[:, 0] * al_[:, 1] + ar[:, 1] * al_[:, 0]], 1)
    nb = lay["n_bodies"]
    b = cp["body"].astype(np.int64)
    f, tau = np.zeros((nb, 3)), np.zeros((nb, 3))
    ef, et, Af, At = (np.zeros((nb, 3)) for _ in range(4))
    np.add.at(f, b, l)
    np.add.at(tau, b, h)
    np.add.at(ef, b, K * el + quantum / 2)
    np.add.at(et, b, K * eh + quantum / 2)
    np.add.at(Af, b, al_)
    np.add.at(At, b, np.abs(h))
    cnt = np.bincount(b, minlength=nb)[:, None]
    if sequential:
        ef += cnt * U32 * Af
        et += cnt * U32 * At
    ef += U32 * np.abs(f) + 1e-14 * Af
    et += U32 * np.abs(tau) + 1e-14 * At
    return dict(v0=v0, ev0=ev0, v=v, ev=ev, f=f, tau=tau, ef=ef, et=et, count=cnt[:, 0])


def prepare(lay, P, gm, gv, gvs, vp, mass_c, contact_v=None, ev=None):
    """everything of one Newton iteration's direction phase: stencil, contact terms at the contact velocity (the particle's
    in iteration 1), node sums and direction"""
    b, wt, keys = stencil(lay)
    T = contact_terms(lay, P, vp if contact_v is None else contact_v, vp, ev)
    T["n"] = -_unit(lay["cp"]["normal"])
    return b, wt, keys, T


def margin(err, bound):
    return tl.margin(err, bound)
