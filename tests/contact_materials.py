"""Per-body contact materials (mpm_set_body_contact_materials) on the layouts of tests/contact_layouts.py: the table of the
tests, the resolution of every contact's (mu, stiffness, damping), and the float64 restatements of contact_layouts with
the parameters read per contact.  CPU only: nothing here imports the engine, and contact_layouts is used as it is.

The table is defined on contact_layouts.layout("bodies") (40 bodies, a third of the particles in contact with two or
three of them, so one cell and one segment of a tile hold contacts of different parameters): body b takes entry b % 7 of
TABLE, so that the bodies 0 - 31 (k_ct_impulse's LDS accumulators) and 32 - 39 (its atomics) both get a mix.

Resolution (include/mpm_hip.h): per field, the entry of the contact's body where the table has one (body < n) and the
field is >= 0, else the scalar of the solving call.  A select: the resolved value is one or the other bit for bit.

Restatements.  Every contact term of contact_layouts (contact_terms, _cost) is per contact, so a parameter set P =
(k, d, dt, mu) whose k, d and mu are arrays over the contacts is restated by calling contact_layouts.contact_terms once per
group of equal triples and merging the rows (contact_terms); contact_layouts._cost takes the arrays as they are (its
arithmetic broadcasts, operation for operation what it does with scalars); line_search restates
contact_layouts.line_search over those two.  direction and impulses do not read P: they are contact_layouts' own.  The
bounds are the module's own formulas, k, d and mu read per contact.  With a uniform table all of this is what
contact_layouts returns for the scalar set, exactly (tests/test_contact_materials.py)."""
import numpy as np

from tests import contact_layouts as cl

INHERIT = -1.0
# (friction_mu, stiffness, damping); a field < 0 inherits the call's scalar
TABLE = np.array([
    (INHERIT, INHERIT, INHERIT),   # 0 inherit all
    (0.5, 1e5, 1e-3),              # 1
    (1.0, 1e6, 1e-5),              # 2
    (0.0, 1e5, 1e-3),              # 3 frictionless
    (0.5, 1e5, 0.0),               # 4 undamped
    (0.5, 1e5, 1.0),               # 5 damped
    (0.25, INHERIT, INHERIT),      # 6 mu only; stiffness and damping inherited
], np.float32)
LAYOUT = "bodies"

gather, stencil, direction, impulses, margin = cl.gather, cl.stencil, cl.direction, cl.impulses, cl.margin


def entry_of_body(n_bodies=40):
    return np.arange(n_bodies) % len(TABLE)


def table(n_bodies=40):
    """the table of the tests: (n_bodies, 3) float32"""
    return TABLE[entry_of_body(n_bodies)].copy()


def uniform_table(call, n_bodies=40):
    """every body's entry = the scalars of `call` = (k, d, dt, mu) as contact_layouts orders them"""
    k, d, dt, mu = call
    return np.tile(np.array([mu, k, d], np.float32), (n_bodies, 1))


def resolve(tab, body, call):
    """(mu, k, d) per contact as float32 (nc, 3): the select of the header, on the float32 values the engine holds"""
    k, d, dt, mu = call
    scal = np.array([mu, k, d], np.float32)
    tab = np.asarray(tab, np.float32).reshape(-1, 3)
    body = np.asarray(body, np.int64)
    has = body < len(tab)
    ent = np.full((len(body), 3), INHERIT, np.float32)
    ent[has] = tab[body[has]]
    return np.where(ent < 0, scal[None, :], ent)


def params(lay, tab, call=None):
    """P = (k, d, dt, mu) with k, d, mu float64 arrays over the contacts (of float32 values), dt the call's"""
    call = cl.params32(lay["params"]) if call is None else call
    r = resolve(tab, lay["cp"]["body"], call).astype(np.float64)
    return r[:, 1], r[:, 2], call[2], r[:, 0]


def groups(P):
    """-> (distinct (k, d, mu) rows, group index per contact)"""
    k, d, dt, mu = P
    rows, inv = np.unique(np.stack([k, d, mu], 1), axis=0, return_inverse=True)
    return rows, inv.reshape(-1)


def contact_terms(lay, P, v, vp, ev=None):
    """contact_layouts.contact_terms with per-contact parameters: one call per group of equal triples, rows merged"""
    rows, g = groups(P)
    out = None
    for i, (k, d, mu) in enumerate(rows):
        T = cl.contact_terms(lay, (float(k), float(d), P[2], float(mu)), v, vp, ev)
        if out is None:
            out = {key: np.array(val, copy=True) for key, val in T.items()}
        else:
            sel = g == i
            for key, val in T.items():
                out[key][sel] = val[sel]
    return out


def prepare(lay, P, gm, gv, gvs, vp, mass_c, contact_v=None, ev=None):
    """contact_layouts.prepare with per-contact parameters"""
    b, wt, keys = cl.stencil(lay)
    T = contact_terms(lay, P, vp if contact_v is None else contact_v, vp, ev)
    T["n"] = -cl._unit(lay["cp"]["normal"])
    return b, wt, keys, T


def line_search(lay, P, wt, keys, mass_c, T, gm, gv, gvs, gD, nodes, alphas, derivs=False, sequential=False, vp=None):
    """contact_layouts.line_search with per-contact parameters (same sums, same bounds; the contact cost and, for the
    derivatives, the contact terms read k, d and mu per contact)"""
    U32, K = cl.U32, cl.K
    cp = lay["cp"]
    rv = cp["rigid_v"].astype(np.float64)
    ov, eov = cl.gather(wt, keys, gv)
    dd, edd = cl.gather(wt, keys, gD)
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
        l, e, vn, aut, ts = cl._cost(P, T, w, eW)
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


def uniform_nodes(P, keys):
    """per distinct (k, d, mu): the dense keys of the grid nodes whose contacts ALL resolve to that triple (from the
    stencils: a node is reached by the contacts that have it among their 27).  -> list of ((k, d, mu), node keys)"""
    rows, g = groups(P)
    nodes, inv = np.unique(keys, return_inverse=True)
    inv = inv.reshape(keys.shape)
    gc = np.repeat(g, keys.shape[1])
    lo = np.full(len(nodes), len(rows), np.int64)
    hi = np.full(len(nodes), -1, np.int64)
    np.minimum.at(lo, inv.reshape(-1), gc)
    np.maximum.at(hi, inv.reshape(-1), gc)
    return [(tuple(float(x) for x in rows[i]), nodes[(lo == i) & (hi == i)]) for i in range(len(rows))]
