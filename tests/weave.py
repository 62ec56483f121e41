"""Woven cloth (mpm_set_weave; drake_amd/csrc/mpm_weave.h) on the CPU: the model restated in numpy float64 from its
definition, a float32 restatement of the kernel's arithmetic, three deliberately wrong restatements, the scenes, axis
cases and states of the tests, and their bound.  Geometry (meshes, deformed states) is tests/bending.py's.

The model.  Per face with corners 0, 1, 2, rest Dm^-1 = [Dm0 Dm1; 0 Dm3], rest volume vol, coefficients
(ka, kb, kab, 2G) and warp a = (c, s), weft b = (-s, c) in the face's rest frame (e1 along the rest edge 0 -> 1, e2 the
in-plane perpendicular towards corner 2):
    F2 = [x1 - x0, x2 - x0] Dm^-1 (3 x 2)      E = 1/2 (F2^T F2 - I)      Eaa = a^T E a, Ebb = b^T E b, Eab = a^T E b
    Psi = 1/2 ka Eaa^2 + 1/2 kb Ebb^2 + kab Eaa Ebb + 2 G Eab^2
    Saa = ka Eaa + kab Ebb, Sbb = kb Ebb + kab Eaa, Sab = 2 G Eab      S = Saa a a^T + Sbb b b^T + Sab (a b^T + b a^T)
    P = F2 S      G_rec = vol P grad_N,  grad_N = Dm^-T [[-1, 1, 0], [-1, 0, 1]]      (vertex force = -sum G_rec)

The bound.  `record_bound` is the same expression as `records64` with every term replaced by its absolute value -- the
atoms are the edge differences x_j - x_0, whose own rounding is relative to themselves; the 1 of F2^T F2 - I is a term
(|E00| stands for 1/2 (|C00| + 1)): the difference cancels at the rest shape and the bound must not --, per record
component; a vertex's bound is the sum over its (face, corner) pairs.  The engine's records must lie within
R 2^-24 bound of records64, R = 28 = rounding_count(): the 27 first-order roundings counted from weave_face in
mpm_weave.h plus one for the second-order terms.  A vertex force, the float sum of n records in ascending face id, gets
R + n.  It is a rounding bound, not a fit: tests/test_weave.py pushes records32 through it on every scene x axis case x
state, and shows that the three wrong models do not fit on any strained state."""
import numpy as np

from tests import bending as bd
from tests import damping as dp

U = 2.0 ** -24
H0 = bd.H0
CENTER = bd.CENTER
THICKNESS = dp.THICKNESS
UP = np.array([0.0, 0.0, 0.05], np.float32)      # the second cloth of a pair lies this much above the first

rest_records = dp.rest_records
corners = dp.corners
vertex_sum = dp.vertex_sum
valence = dp.valence
margin = dp.margin


def rounding_count():
    """R of mpm_weave.h (27 first-order roundings of a record component) + 1 for the second-order terms"""
    return 28.0


WRONG = ("neg_theta", "swapped", "half_shear")


# ---- the constants -------------------------------------------------------------------------------------------------------
def coefficients(E_warp, E_weft, nu, G):
    """(ka, kb, kab, 2G) float32: formed in double from the float constants, rounded once"""
    Ea, Eb, nu, G = (float(np.float32(a)) for a in (E_warp, E_weft, nu, G))
    D = 1.0 - nu * nu * Eb / Ea if Ea > 0 else 1.0
    assert D > 0 and (Ea > 0 or nu == 0)
    return np.array([Ea / D, Eb / D, nu * Eb / D if Ea > 0 else 0.0, 2.0 * G], np.float64).astype(np.float32)


def kmax(coef):
    """the larger of 2G and the larger eigenvalue of [[ka, kab], [kab, kb]], per row of coef (n, 4)"""
    c = np.asarray(coef, np.float64).reshape(-1, 4)
    ev = 0.5 * (c[:, 0] + c[:, 1]) + np.sqrt(0.25 * (c[:, 0] - c[:, 1]) ** 2 + c[:, 2] ** 2)
    return np.maximum(ev, c[:, 3])


# ---- axes ----------------------------------------------------------------------------------------------------------------
def axes64(X, T, dirs):
    """((c, s) (nf, 2) float64, |projection| / |d| (nf,)) of the rest-space directions dirs (nf, 3) or (3,) on the faces'
    rest frames: e1 = (X1 - X0) / |X1 - X0|, n = e1 x (X2 - X0) normalised, e2 = n x e1"""
    Xc = corners(T, np.asarray(X, np.float32)).astype(np.float64)
    d = np.broadcast_to(np.asarray(dirs, np.float32).astype(np.float64), (len(Xc), 3))
    e1 = Xc[:, 1] - Xc[:, 0]
    e1 = e1 / np.linalg.norm(e1, axis=1)[:, None]
    n = np.cross(e1, Xc[:, 2] - Xc[:, 0])
    n = n / np.linalg.norm(n, axis=1)[:, None]
    e2 = np.cross(n, e1)
    p = np.stack([np.einsum("fd,fd->f", d, e1), np.einsum("fd,fd->f", d, e2)], axis=1)
    lp, ld = np.linalg.norm(p, axis=1), np.linalg.norm(d, axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return p / lp[:, None], np.where(ld > 0, lp / ld, 0.0)


# ---- the model in float64 ------------------------------------------------------------------------------------------------
_B = dp._B


def _parts(dm, vol, coef, cs, xc, wrong=None, absolute=False):
    xc = np.asarray(xc, np.float64)
    nf = len(xc)
    A = np.abs if absolute else (lambda a: a)
    M = A(dp._dminv(dm))
    vol = A(np.broadcast_to(np.asarray(vol, np.float64), (nf,)))
    k = A(np.broadcast_to(np.asarray(coef, np.float64), (nf, 4))).copy()
    cs = np.broadcast_to(np.asarray(cs, np.float64), (nf, 2))
    c, s = cs[:, 0], cs[:, 1]
    if wrong == "neg_theta":
        s = -s
    if wrong == "swapped":
        k[:, [0, 1]] = k[:, [1, 0]]
    if wrong == "half_shear":
        k[:, 3] = 0.5 * k[:, 3]
    a, b = A(np.stack([c, s], 1)), A(np.stack([-s, c], 1))
    e = A(xc[:, 1:] - xc[:, :1])                                      # (nf, 2, 3): [edge][component]
    F = np.einsum("fbd,fba->fda", e, M)                               # (nf, 3, 2)
    C = np.einsum("fda,fdb->fab", F, F)
    E = 0.5 * (C + np.eye(2)) if absolute else 0.5 * (C - np.eye(2))
    Eaa, Ebb, Eab = (np.einsum("fa,fab,fb->f", p, E, q) for p, q in ((a, a), (b, b), (a, b)))
    Saa, Sbb, Sab = k[:, 0] * Eaa + k[:, 2] * Ebb, k[:, 1] * Ebb + k[:, 2] * Eaa, k[:, 3] * Eab
    S = (Saa[:, None, None] * np.einsum("fa,fb->fab", a, a) + Sbb[:, None, None] * np.einsum("fa,fb->fab", b, b) +
         Sab[:, None, None] * (np.einsum("fa,fb->fab", a, b) + np.einsum("fa,fb->fab", b, a)))
    P = np.einsum("fda,fab->fdb", F, S)
    gN = np.einsum("fba,bc->fac", M, np.abs(_B) if absolute else _B)
    G = vol[:, None, None] * np.einsum("fda,fac->fcd", P, gN)
    psi = 0.5 * k[:, 0] * Eaa ** 2 + 0.5 * k[:, 1] * Ebb ** 2 + k[:, 2] * Eaa * Ebb + k[:, 3] * Eab ** 2     # (k3 = 2G)
    return G, np.stack([Eaa, Ebb, Eab], 1), vol * psi


def records64(dm, vol, coef, cs, xc, wrong=None):
    """the corner records G_rec (nf, 3, 3) [face][corner][component] in float64 from float inputs; coef (4,) or (nf, 4) =
    (ka, kb, kab, 2G), cs (2,) or (nf, 2), xc (nf, 3, 3) corner positions.  wrong: one of WRONG"""
    return _parts(dm, vol, coef, cs, xc, wrong)[0]


def strain64(dm, cs, xc):
    """(Eaa, Ebb, Eab) (nf, 3)"""
    return _parts(dm, 1.0, np.zeros(4), cs, xc)[1]


def energy64(dm, vol, coef, cs, xc):
    """vol Psi per face (nf,)"""
    return _parts(dm, vol, coef, cs, xc)[2]


def record_bound(dm, vol, coef, cs, xc):
    return _parts(dm, vol, coef, cs, xc, absolute=True)[0]


def energy_bound(dm, vol, coef, cs, xc):
    """vol Psi with every term absolute, per face"""
    return _parts(dm, vol, coef, cs, xc, absolute=True)[2]


def guard64(T, dm, vol, coef_f, mass_v):
    """mpm_weave_max_stable_dt restated: 2 / sqrt(max_i (1 / m_i) sum_{f around i} vol_f kmax_f |g_i| (|g_0| + |g_1| +
    |g_2|)), g_j the columns of grad_N = Dm^-T [[-1, 1, 0], [-1, 0, 1]]; coef_f (nf, 4) per face, mass_v per vertex"""
    dm, vol = np.asarray(dm, np.float64), np.asarray(vol, np.float64)
    gn = np.stack([np.hypot(dm[:, 0], dm[:, 1] + dm[:, 2]), np.hypot(dm[:, 0], dm[:, 1]), np.abs(dm[:, 2])], 1)
    w = vol * kmax(coef_f) * gn.sum(axis=1)
    K = np.zeros(len(mass_v))
    np.add.at(K, np.asarray(T).reshape(-1), (w[:, None] * gn).reshape(-1))
    rate = (K / np.asarray(mass_v, np.float64))[K > 0]
    return 2.0 / np.sqrt(float(rate.max())) if rate.size else np.inf


# ---- the kernel's arithmetic in float32 ----------------------------------------------------------------------------------
def _f(a):
    return np.asarray(a, np.float32)


def _fma(a, b, c):
    """float32 fma, exact: the product of two floats is exact in double; the double sum s = fl(p + c) and its error
    (TwoSum) are known; rounding s to float is the fma's result unless s sits exactly on a tie between two floats while
    the exact sum does not -- then s is nudged one double towards the exact sum first.  (No overflow, no denormals here.)"""
    p, c8 = np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64), np.asarray(c, np.float32).astype(np.float64)
    s = p + c8
    bb = s - p
    err = (p - (s - bb)) + (c8 - bb)
    r = s.astype(np.float32)
    d = s - r.astype(np.float64)
    other = np.nextafter(r, np.where(d > 0, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)).astype(np.float64)
    tie = (d != 0) & (np.abs(other - s) == np.abs(d))
    nudged = np.where(err > 0, np.nextafter(s, np.inf), np.nextafter(s, -np.inf))
    return np.where(tie & (err != 0), nudged, s).astype(np.float32)


def records32(dm, vol, coef, cs, xc):
    """weave_face of mpm_weave.h, statement by statement, in numpy float32 -> (records (nf, 3, 3), strains (nf, 3),
    energies (nf,))"""
    xc, dm = _f(xc), _f(dm)
    nf = len(xc)
    vol = np.broadcast_to(_f(vol), (nf,)).copy()
    k = np.broadcast_to(_f(coef), (nf, 4)).copy()
    cs = np.broadcast_to(_f(cs), (nf, 2)).copy()
    c, s = cs[:, 0], cs[:, 1]
    Dm0, Dm1, Dm3 = dm[:, 0], dm[:, 1], dm[:, 2]
    half, one, two = np.float32(0.5), np.float32(1.0), np.float32(2.0)
    F = [[None, None] for _ in range(3)]
    for d in range(3):
        e0, e1 = xc[:, 1, d] - xc[:, 0, d], xc[:, 2, d] - xc[:, 0, d]
        F[d][0], F[d][1] = e0 * Dm0, _fma(e0, Dm1, e1 * Dm3)
    C00 = _fma(F[2][0], F[2][0], _fma(F[1][0], F[1][0], F[0][0] * F[0][0]))
    C11 = _fma(F[2][1], F[2][1], _fma(F[1][1], F[1][1], F[0][1] * F[0][1]))
    C01 = _fma(F[2][0], F[2][1], _fma(F[1][0], F[1][1], F[0][0] * F[0][1]))
    E00, E11, E01 = half * (C00 - one), half * (C11 - one), half * C01
    cc, ss, sc = c * c, s * s, c * s
    t, q = two * sc, cc - ss
    Eaa = _fma(ss, E11, _fma(cc, E00, t * E01))
    Ebb = _fma(cc, E11, _fma(ss, E00, -(t * E01)))
    Eab = _fma(sc, E11, _fma(-sc, E00, q * E01))
    Saa, Sbb, Sab = _fma(k[:, 0], Eaa, k[:, 2] * Ebb), _fma(k[:, 1], Ebb, k[:, 2] * Eaa), k[:, 3] * Eab
    S00 = _fma(cc, Saa, _fma(ss, Sbb, -(t * Sab)))
    S11 = _fma(ss, Saa, _fma(cc, Sbb, t * Sab))
    S01 = _fma(sc, Saa, _fma(-sc, Sbb, q * Sab))
    g00, g10 = -Dm0, -Dm1 - Dm3
    G = np.zeros((nf, 3, 3), np.float32)
    for d in range(3):
        P0 = vol * _fma(F[d][0], S00, F[d][1] * S01)
        P1 = vol * _fma(F[d][0], S01, F[d][1] * S11)
        G[:, 0, d] = _fma(P0, g00, P1 * g10)
        G[:, 1, d] = _fma(P0, Dm0, P1 * Dm1)
        G[:, 2, d] = P1 * Dm3
    energy = vol * _fma(Sab, Eab, half * _fma(Saa, Eaa, Sbb * Ebb))
    return G, np.stack([Eaa, Ebb, Eab], 1), energy


# ---- scenes: name -> (mesh names, per-cloth material overrides or None, weave constants per cloth or None: no weave) -----
def _sheet54():
    return bd.sheet(5, 4, alternate=True)


def _big():
    return bd.sheet(21, 21, alternate=True, jitter=0.2, seed=4)      # 800 faces: more than 3 x 256, no multiple of 256


DENIM = (2.0e5, 2.0e4, 0.3, 1.0e3)          # E_warp, E_weft, nu, G in Pa: E_warp = 10 E_weft, G two orders below
TWILL = (6.0e4, 1.5e5, 0.15, 4.0e2)
SHEAR_ONLY = (0.0, 0.0, 0.0, 1.0e4)         # yarns without stiffness, a shear modulus alone (the wrong-model test)
MATS = (dict(youngs_modulus=2.5e4, poisson_ratio=0.25), dict(youngs_modulus=6e4, density=1300.0))
SCENES = {
    "triangle": (("triangle",), None, (DENIM,)),
    "strip": (("strip",), None, (DENIM,)),
    "fan": (("fan",), None, (TWILL,)),
    "sheet54": (("sheet54",), None, (DENIM,)),
    "pair_multi": (("jittered", "regular"), MATS, (None, DENIM)),
    "big": (("big",), None, (TWILL,)),
}
ANGLES = {"0": 0.0, "90": 90.0, "30": 30.0, "130": 130.0}
OBLIQUE = ("30", "130")


def meshes(scene):
    out = []
    for k, name in enumerate(SCENES[scene][0]):
        X, T = _big() if name == "big" else (_sheet54() if name == "sheet54" else bd.mesh(name))
        out.append(((X + k * UP).astype(np.float32), T))
    return out


def axis_cases(scene):
    """the names of the scene's axis cases: the four angles of ANGLES through warp_dir; `radial` (fan: a radial field
    through face_dirs); `bias45` (pair_multi: face_dirs at 45 degrees on every second face of the woven cloth, the others
    fall back to warp_dir at 0)"""
    return list(ANGLES) + {"fan": ["radial"], "pair_multi": ["bias45"]}.get(scene, [])


def scene(name):
    """dict: meshes, X / T of all vertices / faces, cof (cloth of face), first (vertex offsets), weaves [(E_warp, E_weft,
    nu, G) or None], coef (n_cloths, 4) float32"""
    ms = meshes(name)
    first = np.cumsum([0] + [len(X) for X, _ in ms])
    X = np.concatenate([X for X, _ in ms])
    T = np.concatenate([T + o for (_, T), o in zip(ms, first)])
    cof = np.concatenate([np.full(len(T), c) for c, (_, T) in enumerate(ms)])
    weaves = SCENES[name][2]
    coef = np.stack([coefficients(*w) if w else np.zeros(4, np.float32) for w in weaves])
    return dict(name=name, meshes=ms, mats=SCENES[name][1], X=X, T=T, cof=cof, first=first, weaves=weaves, coef=coef)


def axis_case(s, case):
    """(table (n_cloths,) for mpm_set_weave as rows (E_warp, E_weft, nu, G, dx, dy, dz), face_dirs (nf, 3) float32 or
    None, dirs (nf, 3) float32: the direction in force on every face)"""
    nf = len(s["T"])
    ang = np.deg2rad(ANGLES.get(case, 0.0))
    d = np.array([np.cos(ang), np.sin(ang), 0.0], np.float32)
    table = np.array([(w or (0, 0, 0, 0)) + tuple(d) for w in s["weaves"]], np.float32)
    fd = None
    if case == "radial":
        cen = corners(s["T"], s["X"]).astype(np.float64).mean(axis=1)
        fd = (cen - CENTER).astype(np.float32)
        fd[:, 2] = 0.0
    if case == "bias45":
        fd = np.zeros((nf, 3), np.float32)
        woven = np.nonzero(s["cof"] == 1)[0][::2]
        fd[woven] = np.array([np.sqrt(0.5), np.sqrt(0.5), 0.0], np.float32)
    dirs = np.broadcast_to(d, (nf, 3)).copy()
    if fd is not None:
        use = np.any(fd != 0, axis=1)
        dirs[use] = fd[use]
    return table, fd, dirs


# ---- states --------------------------------------------------------------------------------------------------------------
def _rotation(X):
    Q = np.linalg.qr(np.random.default_rng(11).normal(size=(3, 3)))[0]
    Q = Q * np.sign(np.linalg.det(Q))
    return (np.asarray(X, np.float64) - CENTER) @ Q.T + CENTER


def _stretch3(X):
    """3 % along x, -2 % along y, then the rotation"""
    return _rotation((np.asarray(X, np.float64) - CENTER) * np.array([1.03, 0.98, 1.0]) + CENTER)


STATES = dict(bd.STATES)
STATES.update(rest=lambda X: np.asarray(X, np.float64), rotation=_rotation, stretch3=_stretch3)
UNSTRAINED = ("rest", "rotation")          # every model agrees there by construction: the strain vanishes


def state(name, s):
    """float32 positions of all vertices of scene dict s"""
    return np.concatenate([STATES[name](X) for X, _ in s["meshes"]]).astype(np.float32)
