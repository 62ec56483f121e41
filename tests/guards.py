"""What the dt guards bound, on the CPU: every guarded force's operators K = -df/dx and D = -df/dv as dense float64
(3n, 3n) matrices, assembled from the float64 references of tests/ alone, the true stability limit of the documented
integrator for such a pair, and the step that is sufficient when several guards are in force at once.  Engine-free: no
GPU, no import of the product.

The integrator: v' = v + dt M^-1 (-K x - D v), x' = x + dt v' -- symplectic Euler, the damping explicit.
Its one-step matrix in the mass-weighted coordinates y = M^1/2 x, u = M^1/2 v, with Ks = M^-1/2 K M^-1/2 and Ds alike:
    [y']   [I - dt^2 Ks    dt (I - dt Ds)] [y]
    [u'] = [  -dt Ks           I - dt Ds  ] [u]
A step is stable while the spectral radius of that matrix is at most 1.  The rigid modes (K x = 0, D v = 0) give a
defective eigenvalue 1 -- x' = x + dt v --, which a nonsymmetric eigenvalue solver returns as 1 +- 1e-8, so the
condition of this module is radius <= 1 + RADIUS_TOL = 1 + 1e-6: a condition, not a measurement.

The assembly.  Linear forces are assembled from their matrix (tests/bending.py's Q) or by applying the reference to unit
vectors (exact: the damping forces are linear in v).  The nonlinear elastic forces (shell, weave) are differenced
centrally with the step FD_STEP = 2^-12 H0: the truncation error is (h / H0)^2 = 6e-8 of K, the rounding error of the
float64 force over h about 2^-53 2^12 = 5e-13.  The references of links and anchors round their inputs to float32, so
they are not differenced at all: K and D are assembled from the law itself -- a spring at l == L gives k n n^T, a seam
k I, the damping c n n^T and c I -- and `spring_operators` gives the exact Hessian of a spring away from l == L.

K and D are NOT reduced to a common modal basis: they do not commute for links, anchors or the shell with its damper
(per-link damping unrelated to the stiffness; beta per cloth on hinges of different stiffness shares K's vectors only
cloth by cloth).  What is exploited is the sparsity alone: the spectrum of a block-diagonal matrix is the union of its
blocks', so `spectral_radius` works component by component of the graph of K and D."""
import math

import numpy as np

from tests import bending as bd
from tests import damping as dp
from tests import shell_bending as sb
from tests import shell_damping as sd
from tests import weave as wv

H0 = bd.H0
FD_STEP = 2.0 ** -12 * H0
RADIUS_TOL = 1e-6
SANITY = 1e-6            # |K - K^T| <= SANITY |K|, and no eigenvalue below -SANITY |K|


# ---- masses -----------------------------------------------------------------------------------------------------------
def masses(X, T, seed=0, density=1000.0, thickness=dp.THICKNESS):
    """made-up vertex masses: area-lumped, times a factor between 0.4 and 2.5 (log-uniform), with both ends of that range
    taken by some vertex of every face-bearing mesh, so that a guard formed on a neighbour's mass is off by up to 6;
    seed None: area-lumped alone, the kind of masses the engine gives a cloth of one density"""
    X, T = np.asarray(X, np.float64), np.asarray(T).reshape(-1, 3)
    area = 0.5 * np.linalg.norm(np.cross(X[T[:, 1]] - X[T[:, 0]], X[T[:, 2]] - X[T[:, 0]]), axis=1)
    m = np.zeros(len(X))
    np.add.at(m, T.reshape(-1), np.repeat(area / 3.0, 3))
    m = np.where(m > 0, m, area.mean() / 3.0) * density * thickness
    if seed is None:
        return m
    r = np.random.default_rng(seed)
    s = np.exp(r.uniform(np.log(0.4), np.log(2.5), len(X)))
    i, j = r.choice(len(X), 2, replace=False)
    s[i], s[j] = 0.4, 2.5
    return m * s


def spread(m):
    """m with its lightest entry halved and its heaviest doubled while they differ by less than 4 x (the few vertices a
    scene of links or anchors is cut down to may have missed both ends of the range)"""
    m = np.array(m, np.float64)
    while m.max() < 4.0 * m.min():
        m[np.argmin(m)] *= 0.5
        m[np.argmax(m)] *= 2.0
    return m


# ---- assembly ---------------------------------------------------------------------------------------------------------
def kron3(Q):
    """a scalar (n, n) operator acting on every component alike, as (3n, 3n) in the order [vertex][component]"""
    return np.kron(np.asarray(Q, np.float64), np.eye(3))


def from_linear(force, n):
    """-d force / d z of a force (n, 3) that is LINEAR in z (n, 3), applied to the unit vectors: exact"""
    A = np.zeros((3 * n, 3 * n))
    z = np.zeros((n, 3))
    for j in range(3 * n):
        z.flat[j] = 1.0
        A[:, j] = -np.asarray(force(z), np.float64).reshape(-1)
        z.flat[j] = 0.0
    return A


def from_differences(force, x, h=FD_STEP):
    """-d force / d x at x by central differences of step h (a power of two times H0)"""
    x = np.asarray(x, np.float64).copy()
    n = len(x)
    A = np.zeros((3 * n, 3 * n))
    for j in range(3 * n):
        x0 = x.flat[j]
        x.flat[j] = x0 + h
        fp = np.asarray(force(x), np.float64).reshape(-1)
        x.flat[j] = x0 - h
        fm = np.asarray(force(x), np.float64).reshape(-1)
        x.flat[j] = x0
        A[:, j] = -(fp - fm) / (2.0 * h)
    return A


def sanity(A, what="operator", psd=True):
    """The assembly's own check: symmetric to SANITY |A|, positive semidefinite to the same.  Returns the symmetric part
    with its negative eigenvalues (at most SANITY |A|, asserted) set to zero.  They are the differences' truncation error
    and the stress that a float32 psibar leaves at the rest shape, both of order 1e-7 |A|; a direction of K with the
    eigenvalue -e grows by 1 + dt sqrt(e / m) per step at EVERY dt, which is no matter of the step size and would make
    the condition radius <= 1 + 1e-6 fail for all of them."""
    scale = float(np.abs(A).max())
    assert np.abs(A - A.T).max() <= SANITY * scale, (what, float(np.abs(A - A.T).max()), scale)
    S = 0.5 * (A + A.T)
    if psd and scale > 0:
        w, V = np.linalg.eigh(S)
        assert w[0] >= -SANITY * scale, (what, float(w[0]), scale)
        S = (V * np.maximum(w, 0.0)) @ V.T
    return S


def bending_K(k, X, T):
    """k Q (x) I_3 of tests/bending.py's hinge operator (linear: the same at every state)"""
    H = bd.hinges(X, T)
    return kron3(float(np.float32(k)) * bd.q_dense(len(X), H)[0]), H


def shell_K(x, H, kc, psibar, h=FD_STEP):
    return from_differences(lambda y: sb.force64(y, H, kc, psibar), x, h)


def shell_D(x, H, bkc):
    return from_linear(lambda v: sd.force64(x, v, H, bkc), len(x))


def weave_K(x, T, dm, vol, coef_f, cs, h=FD_STEP):
    n = len(x)
    return from_differences(lambda y: wv.vertex_sum(T, n, wv.records64(dm, vol, coef_f, cs, wv.corners(T, y))), x, h)


def membrane_D(x, T, dm, vol, mu, lam, beta):
    n = len(x)
    xc = dp.corners(T, x)
    return from_linear(lambda v: dp.vertex_sum(T, n, dp.records64(dm, vol, mu, lam, beta, xc, dp.corners(T, v))), n)


def _unit(d):
    d = np.asarray(d, np.float64)
    l = float(np.linalg.norm(d))
    return d / l if l > 0 else np.array([0.0, 0.0, 1.0])       # coincident ends: any direction; the guard counts the link


def link_operators(links, x, n):
    """(K, D) of tests/links.py's law with every spring at l == L along its direction in x: k n n^T, a seam k I; c alike.
    Every link is taken to act (a slack cord is at l == L too)."""
    K, D = np.zeros((3 * n, 3 * n)), np.zeros((3 * n, 3 * n))
    x = np.asarray(x, np.float64)
    for q in links:
        a, b = int(q["a"]), int(q["b"])
        nn = _unit(x[b] - x[a])
        P = np.outer(nn, nn) if float(q["rest_length"]) > 0 else np.eye(3)
        ia, ib = slice(3 * a, 3 * a + 3), slice(3 * b, 3 * b + 3)
        for A, s in ((K, float(q["stiffness"])), (D, float(q["damping"]))):
            A[ia, ia] += s * P
            A[ib, ib] += s * P
            A[ia, ib] -= s * P
            A[ib, ia] -= s * P
    return K, D


def anchor_operators(anchors, x, y, n):
    """(K, D) of tests/anchors.py's law at l == L: the far end y (n_anchors, 3) is prescribed, so only the vertex's own
    block is touched"""
    K, D = np.zeros((3 * n, 3 * n)), np.zeros((3 * n, 3 * n))
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    for i, q in enumerate(anchors):
        v = int(q["vertex"])
        nn = _unit(y[i] - x[v])
        P = np.outer(nn, nn) if float(q["rest_length"]) > 0 else np.eye(3)
        iv = slice(3 * v, 3 * v + 3)
        K[iv, iv] += float(q["stiffness"]) * P
        D[iv, iv] += float(q["damping"]) * P
    return K, D


def spring_operators(k, L, c, d):
    """the exact 3 x 3 blocks (K, D) of one spring with L > 0 at the separation d, l != L allowed: K = k n n^T +
    k (1 - L / l) (I - n n^T), D = c n n^T (the velocity-dependent part of K vanishes at v = 0)"""
    l = float(np.linalg.norm(d))
    nn = np.asarray(d, np.float64) / l
    P = np.outer(nn, nn)
    return k * P + k * (1.0 - L / l) * (np.eye(3) - P), c * P


# ---- the true limit ---------------------------------------------------------------------------------------------------
def _weighted(A, m):
    s = 1.0 / np.sqrt(np.repeat(np.asarray(m, np.float64), 3))
    return A * s[:, None] * s[None, :]


def lambda_max(A, m):
    """(the largest eigenvalue lambda of M^-1/2 A M^-1/2, the vector phi (n, 3) with A phi = lambda M phi, phi^T M phi = 1)"""
    w, V = np.linalg.eigh(_weighted(0.5 * (A + A.T), m))
    phi = V[:, -1] / np.sqrt(np.repeat(np.asarray(m, np.float64), 3))
    return float(w[-1]), phi.reshape(-1, 3)


def components(K, D):
    """the index sets of the connected components of the graph of K and D (degrees of freedom that neither touches are
    left out: they only carry the eigenvalue 1)"""
    P = (K != 0) | (D != 0)
    P = P | P.T
    n = len(P)
    seen, out = np.zeros(n, bool), []
    for s in np.flatnonzero(P.any(axis=1)):
        if seen[s]:
            continue
        comp, todo = [], [s]
        seen[s] = True
        while todo:
            i = todo.pop()
            comp.append(i)
            for j in np.flatnonzero(P[i] & ~seen):
                seen[j] = True
                todo.append(j)
        out.append(np.array(sorted(comp)))
    return out


def spectral_radius(K, D, m, dt, comps=None):
    """of the one-step matrix at dt (the module's docstring), component by component; K or D may be None (zero)"""
    K = np.zeros_like(D) if K is None else K
    D = np.zeros_like(K) if D is None else D
    Ks, Ds = _weighted(K, m), _weighted(D, m)
    r = 1.0
    for c in (components(K, D) if comps is None else comps):
        k, d = Ks[np.ix_(c, c)], Ds[np.ix_(c, c)]
        I = np.eye(len(c))
        A = np.block([[I - dt * dt * k, dt * (I - dt * d)], [-dt * k, I - dt * d]])
        r = max(r, float(np.abs(np.linalg.eigvals(A)).max()))
    return r


def stable(K, D, m, dt, comps=None):
    return spectral_radius(K, D, m, dt, comps) <= 1.0 + RADIUS_TOL


def true_limit(K, D, m, start=None, rtol=1e-3):
    """The largest stable dt of the integrator for the operators K, D and the vertex masses m.
    * D None or zero: 2 / sqrt(lambda_max(M^-1/2 K M^-1/2)), by eigvalsh.
    * K None or zero: 2 / lambda_max(M^-1/2 D M^-1/2), by eigvalsh -- v' = (I - dt M^-1 D) v alone decides.
    * both: the largest dt with spectral radius <= 1 + 1e-6, by bisection upward from `start` (a guard): dt grows by a
      quarter until a step is unstable, then the bracket is halved until it is narrower than rtol; the stable end is
      returned, so the value is below the limit by at most rtol of it.  If `start` itself is unstable the bisection runs
      between 0 and start."""
    hasK = K is not None and np.any(K)
    hasD = D is not None and np.any(D)
    if not hasK and not hasD:
        return math.inf
    if not hasD:
        return 2.0 / math.sqrt(lambda_max(K, m)[0])
    if not hasK:
        return 2.0 / lambda_max(D, m)[0]
    comps = components(K, D)
    if start is None or not math.isfinite(start):
        start = 1.0 / (lambda_max(D, m)[0] + math.sqrt(lambda_max(K, m)[0]))
    if stable(K, D, m, start, comps):
        lo, hi = start, 1.25 * start
        while stable(K, D, m, hi, comps):
            lo, hi = hi, 1.25 * hi
    else:
        lo, hi = 0.0, start
    while hi - lo > rtol * hi:
        mid = 0.5 * (lo + hi)
        if stable(K, D, m, mid, comps):
            lo = mid
        else:
            hi = mid
    return lo


# ---- several guards at once -------------------------------------------------------------------------------------------
def composed_limit(guards):
    """1 / sum_f (1 / g_f) over the finite guards: a step that is sufficient when several guards are in force at once.
    Each guard g_f is the positive root of its feature's load W_f dt^2 + 2 G_f dt = 4 (W_f, G_f the largest row rates of
    the feature's K and D).  The load is convex in dt, zero at 0 and 4 at g_f, so it is at most 4 dt / g_f below g_f;
    row sums of a sum of operators are at most the sums of the rows' sums, so at dt = 1 / sum (1 / g_f) the total load
    is at most 4.  Use it when any guard in the set has a damping part (links, anchors, damping, the shell with its
    damper) or when that is not known."""
    g = [float(q) for q in guards if math.isfinite(q)]
    if not g:
        return math.inf
    return 1.0 / sum(1.0 / q for q in g) if all(q > 0 for q in g) else 0.0


def composed_limit_elastic(guards):
    """1 / sqrt(sum_f 1 / g_f^2): the tighter form for guards known to be purely elastic (bending, the weave, the shell
    without its damper, links and anchors without damping): there g_f = 2 / sqrt(W_f), and W = sum W_f = sum 4 / g_f^2."""
    g = [float(q) for q in guards if math.isfinite(q)]
    if not g:
        return math.inf
    return 1.0 / math.sqrt(sum(1.0 / (q * q) for q in g)) if all(q > 0 for q in g) else 0.0
