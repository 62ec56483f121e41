"""Finalize's rest state -- Dm^-1, the rest deformation gradient F0, the face particle, the volumes and the masses --
restated in float64 from the definition, the meshes on which it is compared face by face and vertex by vertex, and the
rounding bound of that comparison.  Used by tests/test_rest_meshes.py (CPU, against both builds of the oracle) and
tests/test_rest_state_gpu.py (the engine's k_init_faces, k_init_vertex_adjacency, k_init_vertex_volumes, k_init_masses,
the host half of mpm_finalize and the volume / mass downloads).

Restatement (rest_state).  The float32 vertex positions and velocities are exact inputs, promoted to float64.  Per face
(a, b, c):  D0 = xb - xa, D1 = xc - xa, n = D0 x D1;  q1 = D0 / |D0|, q3 = n / |n|, q2 = q3 x q1;  F0 = [q1 q2 q3];
r00 = |D0|, r01 = q1 . D1, r11 = q2 . D1;  Dm^-1 = (1 / r00, -r01 / (r00 r11), 0, 1 / r11);  the face particle's
position and velocity are the means of the corners';  its volume is |n| / 8 dx;  a vertex' volume is the sum of its
faces' volumes;  mass = volume x the density of the cloth.  This is NOT the Givens sequence of initialize_fem_state_kernel
(oracle/mpm_oracle.c: orc_initialize_fem_state, drake_amd/csrc/mpm_io.h: k_init_faces): three rotations with c >= 0 on
the diagonal give the QR with r00, r11 > 0 and det Q = +1, which the frame above is, whatever branch they take.

Conditioning.  kappa = sigma_max / sigma_min of the 3 x 2 matrix [D0 D1], and 1 / sigma_min = ||Dm^-1||_2 (Dm = R has
the singular values of [D0 D1]).  A backward-stable QR gives R exactly for a matrix within O(eps) ||Ds|| of the input;
the inverse and the orthogonalised columns amplify that by kappa.  Hence every bound is per face in units of

    u = 2^-24 kappa:     |F0 - F0_64| <= cQ u (entrywise)      |Dm^-1 - Dm^-1_64| <= cD u ||Dm^-1||_2
                         |vol - vol_64| <= cV u vol_64
    face position and velocity: 3 2^-24 max|corner component|  (two additions and a division; no kappa)
    vertex volume:  sum_f cV u_f vol_f  +  (valence - 1) 2^-24 sum_f vol_f

No face is excluded from any comparison: the bounds scale with kappa so that none has to be.

The constants are MEASURED on the float build of the oracle against the restatement, the worst ratio over all meshes of
this module (tests/test_rest_meshes.py asserts these values and that none exceeds 32):

    cQ = ORACLE_CQ = 2.23        cD = ORACLE_CD = 3.58        cV = ORACLE_CV = 1.40

(the worst faces are well-conditioned ones, kappa < 1.6, where u is one rounding and the entries carry a few; the bound
is loose where it is large: on the 346 slivers with kappa > 100 the ratios are 0.56, 0.38 and 0.28).
The engine is allowed ENGINE_FACTOR = 4 times each: it forms 1.f / sqrtf(q2) where the oracle rounds a double reciprocal
of sqrt(q2), and 4 is the factor tests/helpers.NOISE_FLOOR uses for "another float evaluation of the same formula".

Meshes (6-bit domain, dx = 1/64, every particle inside [0.15, 0.85]^3, kappa <= 3e4 from the float32 positions that
are uploaded; disjoint triangles have three vertices of their own):
  orientations  D0 exactly along +-x, +-y, +-z (along +-x the first rotation sees a = b = 0: its q2 == 0 branch, and along
                -x the second rotation has c = -1); D0 in each coordinate plane; D1 with one or two zero components;
                triangles lying in each coordinate plane with both windings; 500 uniformly random rotations
  slivers       kappa from 1 to 1e4, needles (one short edge) and caps (apex angle near 180 degrees), each triangle in
                its three cyclic corner orders (Dm depends on which corner is first), random orientation
  scales        edge lengths from 1e-3 dx to 0.3 in one mesh: face volumes over more than 8 decades, the case a maximum
                norm over the array cannot see
  valence       hubs with 1, 2, 7, 8, 9, 16, 17 and 40 faces, twice (petals with rim vertices of their own; fans that
                share them) and one vertex in no face; every hub's faces interleaved with the others' in face-id order;
                the petals' areas around one hub span more than 1e3, so that the float32 sum depends on its order; 325 vertices
                (beyond 256 and beyond 10 x VF_CHUNK), a hub of nine faces at vertex 255, the isolated vertex at 256, a
                hub of forty at the last id
  tails_N       a triangle strip of N in {1, 255, 256, 257} faces, N + 2 vertices

The q2 == 0 branches of the other two rotations (givens_branches) need |D0| = 0 or r11 = 0: a triangle of zero area.
Degenerate faces -- zero area, or an index repeated within a face -- are out of scope: the reference divides by zero
there too, and so does everything restated from it."""
import numpy as np

from tests.fem_regimes import _rot3

BITS = 6
DX = 1.0 / (1 << BITS)
U24 = 2.0 ** -24
LO, HI = 0.15, 0.85
KAPPA_MAX = 3e4
DENSITY = 2000.0          # mpm_default_material / orc_default_params
VF_CHUNK = 32             # drake_amd/csrc/mpm_device.h

ORACLE_CQ, ORACLE_CD, ORACLE_CV = 2.23, 3.58, 1.40
ENGINE_FACTOR = 4.0
C_LIMIT = 32.0            # a measured constant above this fails the CPU test instead of widening the GPU one

HUB_VALENCES = (1, 2, 7, 8, 9, 16, 17, 40)
TAILS = (1, 255, 256, 257)


class Mesh:
    def __init__(self, name, pos, vel, idx, **info):
        self.name = name
        self.pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
        self.vel = np.ascontiguousarray(vel, np.float32).reshape(-1, 3)
        self.idx = np.ascontiguousarray(idx, np.int32).reshape(-1, 3)
        self.nv, self.nf = len(self.pos), len(self.idx)
        self.info = info

    def sheet(self):
        """(pos, vel, indices) for add_qr_cloth"""
        return self.pos, self.vel, self.idx

    def faces(self, lo, hi):
        """faces lo .. hi - 1 of a mesh of disjoint triangles, as a mesh of their own"""
        assert np.array_equal(self.idx, np.arange(3 * self.nf).reshape(-1, 3))
        return Mesh(f"{self.name}[{lo}:{hi}]", self.pos[3 * lo:3 * hi], self.vel[3 * lo:3 * hi],
                    np.arange(3 * (hi - lo)).reshape(-1, 3))


def merged(meshes, name="merged"):
    """one mesh with the vertices and the faces of `meshes` in turn: what several add_qr_cloth calls amount to"""
    off = np.cumsum([0] + [m.nv for m in meshes])
    return Mesh(name, np.concatenate([m.pos for m in meshes]), np.concatenate([m.vel for m in meshes]),
                np.concatenate([m.idx + o for m, o in zip(meshes, off)]))


# ---- the restatement ---------------------------------------------------------------------------------------------
def rest_state(mesh, density=DENSITY, dx=DX):
    """Finalize's outputs for `mesh` in float64, particle arrays in original order (faces, then vertices):
    F0 (nf, 9) row-major, Dm (nf, 4), pos, vel (np, 3), vol, mass (np,); per face kappa, inv_smin = ||Dm^-1||_2, the
    largest |corner component| of position and velocity (xmax, vmax); per vertex its valence and its faces (ascending)"""
    x, v, idx = mesh.pos.astype(np.float64), mesh.vel.astype(np.float64), mesh.idx
    nf, nv = mesh.nf, mesh.nv
    xa, xb, xc = x[idx[:, 0]], x[idx[:, 1]], x[idx[:, 2]]
    D0, D1 = xb - xa, xc - xa
    n = np.cross(D0, D1)
    r00 = np.linalg.norm(D0, axis=1)
    area2 = np.linalg.norm(n, axis=1)
    q1, q3 = D0 / r00[:, None], n / area2[:, None]
    q2 = np.cross(q3, q1)
    r01, r11 = np.einsum("fi,fi->f", q1, D1), np.einsum("fi,fi->f", q2, D1)
    F0 = np.stack([q1, q2, q3], axis=2).reshape(nf, 9)
    Dm = np.stack([1.0 / r00, -r01 / (r00 * r11), np.zeros(nf), 1.0 / r11], axis=1)
    sv = np.linalg.svd(np.stack([D0, D1], axis=2), compute_uv=False) if nf else np.zeros((0, 2))
    volf = area2 / 8.0 * dx
    volv = np.zeros(nv)
    np.add.at(volv, idx.reshape(-1), np.repeat(volf, 3))
    corners_x, corners_v = x[idx], v[idx]
    vol = np.concatenate([volf, volv])
    vfaces = [[] for _ in range(nv)]
    for f in range(nf):
        for c in range(3):
            vfaces[idx[f, c]].append(f)
    return dict(F0=F0, Dm=Dm, pos=np.concatenate([corners_x.mean(axis=1).reshape(nf, 3), x]),
                vel=np.concatenate([corners_v.mean(axis=1).reshape(nf, 3), v]), vol=vol, mass=vol * float(np.float32(density)),
                kappa=sv[:, 0] / sv[:, 1], inv_smin=1.0 / sv[:, 1], xmax=np.abs(corners_x).reshape(nf, -1).max(axis=1),
                vmax=np.abs(corners_v).reshape(nf, -1).max(axis=1), valence=np.array([len(a) for a in vfaces]),
                vfaces=vfaces, D0=D0, D1=D1, nf=nf, nv=nv)


def unit_ratios(got, ref):
    """|got - ref| of F0, Dm and the face volumes in units of u, u ||Dm^-1||_2 and u vol: per face, the largest over the
    components.  The worst of each over a set of meshes is the constant cQ, cD, cV of whatever computed `got`.
    got: dict of F0 (nf, 9), Dm (nf, 4), pos, vel (np, 3), vol (np,) in original order"""
    nf = ref["nf"]
    u = U24 * ref["kappa"]
    g = {k: np.asarray(got[k], np.float64) for k in ("F0", "Dm", "vol")}
    return dict(F0=np.abs(g["F0"] - ref["F0"]).max(axis=1) / u if nf else np.zeros(0),
                Dm=np.abs(g["Dm"] - ref["Dm"]).max(axis=1) / (u * ref["inv_smin"]) if nf else np.zeros(0),
                volf=np.abs(g["vol"][:nf] - ref["vol"][:nf]) / (u * ref["vol"][:nf]))


def bound_ratios(got, ref, cQ, cD, cV):
    """error / allowed of every field under the module's bound with constants cQ, cD, cV: F0, Dm, volf, xf, vf per face,
    volv per vertex (the isolated vertex: 0 where its volume is exactly 0, inf otherwise)"""
    nf = ref["nf"]
    r = unit_ratios(got, ref)
    out = dict(F0=r["F0"] / cQ, Dm=r["Dm"] / cD, volf=r["volf"] / cV)
    for k, m in (("pos", "xmax"), ("vel", "vmax")):
        d = np.abs(np.asarray(got[k], np.float64)[:nf] - ref[k][:nf]).max(axis=1) if nf else np.zeros(0)
        out["xf" if k == "pos" else "vf"] = d / (3.0 * U24 * ref[m])
    u = U24 * ref["kappa"]
    volf, face_part = ref["vol"][:nf], cV * u * ref["vol"][:nf]
    allowed = np.array([face_part[fs].sum() + (max(len(fs), 1) - 1) * U24 * volf[fs].sum() for fs in ref["vfaces"]])
    err = np.abs(np.asarray(got["vol"], np.float64)[nf:] - ref["vol"][nf:])
    with np.errstate(divide="ignore", invalid="ignore"):
        out["volv"] = np.where(allowed > 0, err / np.where(allowed > 0, allowed, 1.0), np.where(err == 0, 0.0, np.inf))
    for k, a in out.items():   # (a NaN or an infinity in `got` is a failure of that face, not a silent pass)
        out[k] = np.where(np.isfinite(a), a, np.inf)
    return out


def givens_branches(mesh):
    """How many faces take each q2 == 0 branch of the three rotations of the QR of [D0 D1] (rows (1, 2) of column 0,
    rows (0, 1) of column 0, rows (1, 2) of column 1), from the float32 edges as the kernels form them.  The first has
    a = D0y, b = D0z; it is split by the sign of c = D0x / |D0x| in the second.  The other two have q2 = |D0|^2 and
    r11^2: reachable by degenerate faces only, which no mesh here has."""
    x = mesh.pos
    D0 = (x[mesh.idx[:, 1]] - x[mesh.idx[:, 0]]).astype(np.float32)
    first = (D0[:, 1] * D0[:, 1] + D0[:, 2] * D0[:, 2]) == 0
    ref = rest_state(mesh)
    return dict(first_c_plus=int((first & (D0[:, 0] > 0)).sum()), first_c_minus=int((first & (D0[:, 0] < 0)).sum()),
                second=int((np.einsum("fi,fi->f", D0, D0) == 0).sum()),
                third=int((~(np.linalg.norm(np.cross(ref["D0"], ref["D1"]), axis=1) > 0)).sum()))


def f32_sum_ascending(volf32, vfaces):
    """the float32 sum of every vertex' faces' volumes in ascending face id, starting from 0.f (k_init_vertex_volumes;
    orc_initialize_fem_state adds them in the same order)"""
    out = np.zeros(len(vfaces), np.float32)
    for k, fs in enumerate(vfaces):
        s = np.float32(0)
        for f in fs:
            s = np.float32(s + np.float32(volf32[f]))
        out[k] = s
    return out


# ---- the meshes --------------------------------------------------------------------------------------------------
def _vel(rng, n):
    return rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)


def _disjoint(name, corners, rng, **info):
    corners = np.asarray(corners, np.float32).reshape(-1, 3)
    return Mesh(name, corners, _vel(rng, len(corners)), np.arange(len(corners)).reshape(-1, 3), **info)


def _placed(rng, local, extent):
    """local (n, 3, 3) triangles about their own origin, each moved to a random centre that keeps `extent` clear of
    [LO, HI]^3's faces"""
    extent = np.broadcast_to(np.asarray(extent, np.float64), (len(local),))[:, None]
    cen = LO + extent + rng.random((len(local), 3)) * (HI - LO - 2 * extent)
    return cen[:, None, :] + local


def orientations(seed=11):
    rng = np.random.default_rng(seed)
    tris, tags = [], []
    E = np.eye(3)

    def length():
        return rng.uniform(0.5, 2.0) * DX

    def generic():
        return rng.uniform(0.3, 1.5, 3) * rng.choice((-1.0, 1.0), 3) * DX

    def add(tag, d0, d1):
        # (float32 sums: a zero component of d0 or d1 leaves that coordinate of the corner BIT-EQUAL to xa's, so the
        # edge xb - xa that the kernels form has an exact zero there)
        xa = rng.uniform(0.3, 0.7, 3).astype(np.float32)
        tris.append([xa, xa + np.asarray(d0, np.float32), xa + np.asarray(d1, np.float32)])
        tags.append(tag)

    for ax in range(3):
        for sg in (1.0, -1.0):
            d0 = sg * length() * E[ax]
            for _ in range(4):
                add(f"D0 along {'+-'[sg < 0]}{'xyz'[ax]}", d0, generic())
            for z in range(3):                      # D1 with one zero component
                d1 = generic()
                d1[z] = 0.0
                add(f"D0 along {'+-'[sg < 0]}{'xyz'[ax]}", d0, d1)
            for o in range(3):                      # D1 along another axis
                if o != ax:
                    for so in (1.0, -1.0):
                        add(f"D0 along {'+-'[sg < 0]}{'xyz'[ax]}", d0, so * length() * E[o])
    for z in range(3):
        for _ in range(8):
            d0 = generic()
            d0[z] = 0.0
            add(f"D0 in the plane {'xyz'[z]} = 0", d0, generic())
    for z in range(3):
        for _ in range(4):
            d1 = generic()
            d1[z] = 0.0
            add("D1 with one zero component", generic(), d1)
        for sg in (1.0, -1.0):
            for _ in range(2):
                add("D1 with two zero components", generic(), sg * length() * E[z])
    for z in range(3):
        for _ in range(8):
            d0, d1 = generic(), generic()
            d0[z] = d1[z] = 0.0
            if abs(d0[(z + 1) % 3] * d1[(z + 2) % 3] - d0[(z + 2) % 3] * d1[(z + 1) % 3]) < 0.05 * DX * DX:
                d1[(z + 1) % 3] = -d1[(z + 1) % 3]
            add(f"in the plane {'xyz'[z]} = const", d0, d1)
            add(f"in the plane {'xyz'[z]} = const, other winding", d1, d0)
    n_fixed = len(tris)
    L0, L1 = rng.uniform(0.5, 2.0, 500) * DX, rng.uniform(0.5, 2.0, 500) * DX
    th = rng.uniform(np.radians(40), np.radians(140), 500)
    local = np.zeros((500, 3, 3))
    local[:, 1, 0] = L0
    local[:, 2, 0], local[:, 2, 1] = L1 * np.cos(th), L1 * np.sin(th)
    local = np.einsum("fij,fcj->fci", _rot3(rng, 500), local - local.mean(axis=1, keepdims=True))
    corners = np.concatenate([np.asarray(tris, np.float32).reshape(-1, 3, 3),
                              _placed(rng, local, 2.0 * DX).astype(np.float32)])
    return _disjoint("orientations", corners, rng, tags=tags + ["random rotation"] * 500, n_fixed=n_fixed)


def slivers(seed=12, n_each=110):
    rng = np.random.default_rng(seed)
    local, kind = [], []
    for shape in ("needle", "cap"):
        r = 10.0 ** rng.uniform(0.0, 3.9, n_each)
        r[0], r[-1] = 1.0, 10.0 ** 3.9
        L = rng.uniform(0.1, 0.25, n_each)
        t = np.zeros((n_each, 3, 3))
        t[:, 1, 0] = L
        t[:, 2, 0] = L if shape == "needle" else 0.5 * L
        t[:, 2, 1] = L / r
        t = np.einsum("fij,fcj->fci", _rot3(rng, n_each), t - t.mean(axis=1, keepdims=True))
        t = _placed(rng, t, L).astype(np.float32)
        for order in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
            local.append(t[:, order, :])
            kind += [f"{shape} {order}"] * n_each
    return _disjoint("slivers", np.concatenate(local), rng, kind=kind)


def scales(seed=13, n=600):
    rng = np.random.default_rng(seed)
    e = 10.0 ** rng.uniform(np.log10(1e-3 * DX), np.log10(0.3), n)
    e[0], e[-1] = 1e-3 * DX, 0.3
    t = np.zeros((n, 3, 3))
    t[:, 1, 0] = e
    t[:, 2, 0], t[:, 2, 1] = e * rng.uniform(0.3, 0.7, n), e * rng.uniform(0.5, 0.7, n)
    t = np.einsum("fij,fcj->fci", _rot3(rng, n), t - t.mean(axis=1, keepdims=True))
    return _disjoint("scales", _placed(rng, t, 0.7 * e), rng, edge=e)


def valence(seed=14):
    rng = np.random.default_rng(seed)
    pos, hubs = [], []           # hubs: (valence, kind, hub vertex, its faces in order)
    cells = [(i, j) for i in range(4) for j in range(4)]
    for h, (k, kind) in enumerate([(k, kind) for kind in ("petals", "fan") for k in HUB_VALENCES]):
        c = np.array([0.275 + 0.15 * cells[h][0], 0.275 + 0.15 * cells[h][1], rng.uniform(0.4, 0.6)])
        hub = len(pos)
        pos.append(c)
        faces = []
        if kind == "petals":
            r = 0.07 * DX * 48.0 ** (rng.permutation(k) / max(k - 1, 1))    # areas ~ r^2: a span above 1e3 from k = 2 on
            for i in range(k):
                th, dl = rng.uniform(0, 2 * np.pi), rng.uniform(np.radians(40), np.radians(80))
                a, b = len(pos), len(pos) + 1
                pos.append(c + r[i] * np.array([np.cos(th), np.sin(th), rng.uniform(-0.4, 0.4)]))
                pos.append(c + r[i] * np.array([np.cos(th + dl), np.sin(th + dl), rng.uniform(-0.4, 0.4)]))
                faces.append((hub, a, b))
        else:
            step = min(np.radians(60), np.radians(340) / k)
            rim = []
            for i in range(k + 1):
                rr = DX * rng.uniform(0.5, 2.0)
                rim.append(len(pos))
                pos.append(c + rr * np.array([np.cos(i * step), np.sin(i * step), rng.uniform(-0.3, 0.3)]))
            faces = [(hub, rim[i], rim[i + 1]) for i in range(k)]
        # (the hub is the first, the second or the third corner of its faces in turn)
        hubs.append((k, kind, hub, [tuple(np.roll(f, i % 3)) for i, f in enumerate(faces)]))
    isolated = len(pos)
    pos.append(np.array([0.5, 0.5, 0.3]))
    # faces of all hubs interleaved: a hub's faces ascend in face id but are never neighbours
    idx, queues = [], [list(h[3]) for h in hubs]
    while any(queues):
        for q in queues:
            if q:
                idx.append(q.pop(0))
    nv = len(pos)
    # vertex ids shuffled, then three of them pinned (see the module docstring)
    new_of = rng.permutation(nv)

    def pin(v, target):
        other = int(np.flatnonzero(new_of == target)[0])
        new_of[other], new_of[v] = new_of[v], target

    nine = [h for h in hubs if h[0] == 9][0][2]
    forty = [h for h in hubs if h[0] == 40][-1][2]
    pin(nine, 255)
    pin(isolated, 256)
    pin(forty, nv - 1)
    p = np.zeros((nv, 3))
    p[new_of] = np.asarray(pos)
    return Mesh("valence", p, _vel(rng, nv), new_of[np.asarray(idx)], isolated=int(new_of[isolated]),
                hubs=[(k, kind, int(new_of[v])) for k, kind, v, _ in hubs])


def tails(nf, seed=15):
    rng = np.random.default_rng(seed + nf)
    nv = nf + 2
    step = min(0.6 / nv, DX)
    i = np.arange(nv)
    p = np.stack([0.2 + i * step, 0.5 + (i % 2) * DX + rng.uniform(-0.1, 0.1, nv) * DX,
                  0.5 + rng.uniform(-0.3, 0.3, nv) * DX], axis=1)
    idx = [(k, k + 1, k + 2) if k % 2 == 0 else (k + 1, k, k + 2) for k in range(nf)]
    return Mesh(f"tails_{nf}", p, _vel(rng, nv), idx)


_CACHE = {}


def meshes():
    """{name: (Mesh, rest_state(Mesh))} of every mesh of the module, made once"""
    if not _CACHE:
        for m in [orientations(), slivers(), scales(), valence()] + [tails(n) for n in TAILS]:
            _CACHE[m.name] = (m, rest_state(m))
    return _CACHE


def three_cloths():
    """slivers (as two cloths, cut at a face) and valence: the cloths of the metamorphic tests, and their merged mesh"""
    sl, va = meshes()["slivers"][0], meshes()["valence"][0]
    parts = [sl.faces(0, 300), sl.faces(300, sl.nf), va]
    return parts, merged(parts, "slivers + valence")


def original_order(F, Dm, pos, vel, vol, pids, mass=None):
    """downloads un-permuted to original particle order (fem_regimes.original_order's convention); dtypes kept"""
    def un(a):
        o = np.empty_like(a)
        o[pids] = a
        return o
    out = dict(F0=np.asarray(F), Dm=np.asarray(Dm), pos=un(pos), vel=un(vel), vol=un(vol))
    if mass is not None:
        out["mass"] = un(mass)
    return out


def of_oracle(o):
    return original_order(o.F, o.DmInv, o.pos, o.vel, o.vol, o.pids)


def of_engine(g, masses=False):
    from drake_amd import ARR as A
    return original_order(*(g.download(a) for a in (A.DEFORMATION_GRADIENTS, A.DM_INVERSES, A.POSITIONS, A.VELOCITIES,
                                                     A.VOLUMES, A.PIDS)), mass=g.download(A.MASSES) if masses else None)
