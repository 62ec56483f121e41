"""The contact layouts of tests/contact_layouts.py on the CPU: every layout reaches what it claims, the float64
restatements of the contact solve's phases agree with the double build of the oracle (1e-12 of each quantity's natural
scale), and the bounds are real rounding bounds: the float build of the oracle, which adds every sum sequentially, stays
within them (L_n = N_n)."""
import numpy as np
import pytest

from tests import contact_layouts as cl
from tests import harness as hs
from tests import transfer_layouts as tl

ALPHAS = [2.0 ** -j for j in range(8)]


def run_oracle(lay, real, iters=1, exact=False, relax=None):
    """the layout in an oracle (density 1, volumes = the masses, no FEM forces): P2G, UpdateGrid, the pairs, one solve.
    -> (oracle, pre-solve grid (m, v, v*), solve result)"""
    from oracle import oracle as orc
    k, d, dt, mu = cl.params32(lay["params"])
    o = orc.OracleMpm(lay["bits"], real=real)
    o.p.gravity_axis = lay["gravity_axis"]
    o.p.density = 1.0
    for rest, vel, idx in lay["cloths"]:
        o.add_qr_cloth(rest, vel, idx)
    o.finalize()
    for name, key in (("pos", "pos"), ("vel", "vel"), ("C", "C"), ("vol", "mass")):
        setattr(o, name, np.ascontiguousarray(np.asarray(lay[key], np.float32), dtype=real))
    o.taus[:] = 0
    o.forces[:] = 0
    o.particle_to_grid(dt)
    o.update_grid(-1)
    pre = (o.g_m.copy(), o.g_mv.copy(), o.g_vstar.copy())
    cp = lay["cp"]
    o.reallocate_external_bodies(lay["n_bodies"])
    # (the double build gets the float normals normalised in double: its frame is then orthonormal to the last bit, and
    # the world-frame restatement has no frame to match; the float build gets them as the engine does)
    nrm = cl._unit(cp["normal"]) if real is np.float64 else cp["normal"]
    o.copy_contact_pairs(orc.ContactPairs(cp["particle"], cp["body"], cp["dist"], nrm, cp["pos"], cp["rigid_v"], cp["p_WB"],
                                          real=real))
    if relax is not None:
        o.set_contact_relax(relax)
    try:
        r = o.update_contact(dt, mu, k, d, exact_line_search=exact, max_iters=iters)
    finally:
        if relax is not None:
            o.set_contact_relax(0.3)
    return o, pre, r


def restate(lay, o, pre, sequential, relax=cl.RELAX, received=None):
    """every restated phase of one Newton iteration on the oracle's inputs (received: cl.chain_lengths')"""
    P = cl.params32(lay["params"])
    gm, gv, gvs = pre
    cp = lay["cp"]
    vp = np.asarray(o.vel, np.float64)[cp["particle"]]
    mass_c = lay["mass"][cp["particle"]].astype(np.float64)
    b, wt, keys, T = cl.prepare(lay, P, gm, gv, gvs, vp, mass_c)
    vel0, e0 = cl.gather(wt, keys, gv, gm)
    dr = cl.direction(lay, P, wt, keys, mass_c, T, gm, gv, gvs, relax=relax, sequential=sequential, received=received)
    return dict(P=P, vp=vp, mass_c=mass_c, wt=wt, keys=keys, T=T, vel0=vel0, e0=e0, dr=dr)


@pytest.mark.parametrize("name", cl.NAMES)
def test_layout_reaches_what_it_claims(name):
    lay = cl.layout(name)
    cl_ = lay["claims"]
    cp = lay["cp"]
    bits = lay["bits"]
    hi = (1 << bits) - 3
    t = tl.f32(lay["pos"]).astype(np.float64) * (1 << bits) - 0.5
    assert (t >= 0).all() and (t < hi + 1).all()
    assert (cp["dist"] < 0).all() and np.array_equal(cp["pos"], lay["pos"][cp["particle"]])
    assert np.allclose(np.linalg.norm(cp["normal"].astype(np.float64), axis=1), 1.0, atol=1e-6)
    P = cl.params32(lay["params"])
    vp = lay["vel"][cp["particle"]].astype(np.float64)
    b, wt, keys = cl.stencil(lay)
    T = cl.contact_terms(lay, P, vp, vp)
    # no separated test within its rounding of v_hat
    assert T["sep_margin"].min() > 10.0, T["sep_margin"].min()
    if "normals" in cl_:
        n = cp["normal"].astype(np.float64)
        a = np.sort(np.abs(n), axis=1)
        assert (np.isclose(a[:, 2], 1.0) & (a[:, 1] == 0)).sum() >= 6                     # axes
        assert (np.abs(a[:, 0] - a[:, 2]) < 1e-6).sum() >= 8                               # diagonals
        assert ((np.abs(a[:, 0] - a[:, 1]) < 1e-7) & (a[:, 2] - a[:, 1] > 0.1)).sum() >= 6   # ties of the two smallest
        ang = np.arccos(np.clip(a[:, 2], -1, 1))
        assert ((ang > 5e-5) & (ang < 1.1e-3)).sum() >= 12                                 # near an axis
        assert len(n) >= 400
    if "regimes" in cl_:
        app = ~T["sep"]
        sliding = app & (T["ut"] >= 100 * cl.EPSV)
        sticking = app & (T["ut"] <= 0.01 * cl.EPSV)
        trans = app & (T["ut"] > 0.1 * cl.EPSV) & (T["ut"] < 10 * cl.EPSV)
        for what, sel in (("separating", T["sep"]), ("sliding", sliding), ("sticking", sticking), ("transitional", trans)):
            assert sel.sum() >= 100, (what, int(sel.sum()))
        assert (T["vn"][app] < 0).all()
        if lay["params"] == "damped":
            d = P[1]
            side = T["phi0"] / P[2] > 1.0 / d
            assert side.sum() >= 100 and (~side).sum() >= 100
    if "bodies" in cl_:
        body = cp["body"]
        assert set(body.tolist()) == set(range(40))
        assert (body >= 32).sum() >= 16
        dist = np.linalg.norm(cp["pos"].astype(np.float64) - cp["p_WB"], axis=1) * (1 << bits)
        assert dist.min() > 10.0
        per_particle = np.bincount(cp["particle"])
        assert (per_particle == 2).sum() > 20 and (per_particle == 3).sum() > 20
        # the rigid velocity varies from contact to contact within one body
        rv0 = cp["rigid_v"][body == 0]
        assert np.ptp(rv0, axis=0).max() > 0.1
    if "runs" in cl_:
        base = keys[:, 0]
        cnt = dict(zip(*np.unique(base, return_counts=True)))
        for want, cell in cl_["runs"].items():
            assert cnt.get(int(tl.cell_key(*cell))) == want, (want, cell)
        # segments per tile in the solve's order (ascending cell key: active blocks are numbered in ascending order)
        sk = np.sort(base, kind="stable")
        nseg = [len(np.unique(sk[i:i + 64])) for i in range(0, len(sk), 64)]
        for lo, hi_ in ((1, 1), (2, 8), (9, 16), (17, 64)):
            assert any(lo <= s <= hi_ for s in nseg), (lo, hi_, nseg)
        # a node reached from all 27 base cells
        node = int(tl.cell_key(*cl_["all27"]))
        reach = {int(b_) for b_, row in zip(base, keys) if node in row}
        assert len(reach) == 27
    if cl_.get("light"):
        gm = tl.p2g64(lay["pos"], lay["vel"], lay["C"], lay["mass"], np.zeros((len(lay["pos"]), 9)),
                      np.zeros((len(lay["pos"]), 3)), bits, 2)["m"]
        m = gm[np.unique(keys)]
        assert ((m > 0) & (m <= cl.THRESH)).sum() > 50 and (m > cl.THRESH).sum() > 50
        assert (np.abs(m / cl.THRESH - 1.0) > 1e-4).all()          # clear of the gathers' threshold
        mass_c = lay["mass"][cp["particle"]].astype(np.float64)
        dr = cl.direction(lay, P, wt, keys, mass_c, T, gm, np.zeros((len(gm), 3)), np.zeros((len(gm), 3)))
        live = dr["mn"] > 0
        below = live & ~dr["dof"] & ~dr["amb"]
        assert below.sum() > 20 and (live & dr["dof"] & ~dr["amb"]).sum() > 100
        # nodes that see separated contacts only
        sep_only = np.ones(len(dr["nodes"]), bool)
        np.logical_and.at(sep_only, dr["inv"].reshape(-1), np.repeat(T["sep"], 27))
        assert (sep_only & live).sum() > 50
        assert (np.abs(dr["Hn"][sep_only]).max() == 0) and (np.abs(dr["Gn"][sep_only]).max() == 0)
        assert (b == 0).any(axis=0).all() and (b == hi).any(axis=0).all()


def _check(lay, o, pre, r, R, sequential, tag):
    """restatement R against oracle `o` after one iteration: 1e-12 of natural scale (double) or the bound (float)"""
    P, wt, keys, dr, T = R["P"], R["wt"], R["keys"], R["dr"], R["T"]
    gm, gv, gvs = pre
    worst = {}
    rel = 1e-12

    def cmp(field, err, bound, scale):
        err = np.abs(np.asarray(err, np.float64))
        if sequential:
            w = cl.margin(err, bound)
        else:
            w = cl.margin(err, rel * np.asarray(scale, np.float64) + 1e-300)
        worst[field] = w

    cmp("vel0", o.c_vel0 - R["vel0"], R["e0"], R["e0"] / cl.GATHER)
    nodes = dr["nodes"]
    gD = np.asarray(o.g_D, np.float64)
    ok = dr["dof"] & ~dr["amb"]
    cmp("Dir", gD[nodes][ok] - dr["D"][ok], dr["eD"][ok], dr["eD"][ok] / cl.U32)
    off = ~dr["dof"] & ~dr["amb"]
    assert not np.abs(gD[nodes][off]).any(), (tag, "a direction where the restatement has no DoF")
    assert dr["dof"][~dr["amb"]].sum() <= r["dofs"] <= dr["dof"].sum() + dr["amb"].sum()
    if not dr["amb"].any():
        assert r["dofs"] == dr["dof"].sum()
        cmp("|Dir|^2", [r["norm_dir_sq"] - dr["nd"]], [2 * (np.abs(dr["D"]) * dr["eD"]).sum() / cl.RELAX ** 2 + 1e-300],
            [2 * (np.abs(dr["D"]) * dr["eD"]).sum() / cl.RELAX ** 2 / cl.U32 + 1e-300])
    # line search on the oracle's own direction
    gDd = np.asarray(o.g_D, np.float64)
    ls = cl.line_search(lay, P, wt, keys, R["mass_c"], T, gm, gv, gvs, gDd, nodes, [0.0] + ALPHAS)
    E0 = ls[0]
    cmp("E0", [r["E0"] - E0["E"]], [E0["eE"]], [E0["A"]])
    acc = [a for a in ls[1:] if a["E"] <= E0["E"]]
    al = acc[0]["alpha"] if acc else None
    if al is not None and r["alpha"] == al:
        a = acc[0]
        cmp("E(alpha)", [r["E1"] - a["E"]], [a["eE"] + E0["eE"]], [a["A"]])
    if not sequential:
        assert r["alpha"] == al, (tag, r["alpha"], al)
    else:
        # the float oracle's step: acceptable within the bound, every larger one rejected within the bound
        for a in ls[1:]:
            if a["alpha"] > r["alpha"]:
                assert a["E"] - E0["E"] >= -(a["eE"] + E0["eE"]), (tag, a["alpha"])
            elif a["alpha"] == r["alpha"]:
                assert a["E"] - E0["E"] <= a["eE"] + E0["eE"], (tag, a["alpha"])
    # contact velocities after the step and the impulses
    gv1 = np.asarray(o.g_mv, np.float64)
    q = 0.0
    imp = cl.impulses(lay, wt, keys, gm, gv, gv1, R["mass_c"], q, sequential)
    cmp("contact vel", o.c_vel - imp["v"], imp["ev"], imp["ev"] / cl.GATHER)
    cmp("F_f", o.F_f - imp["f"], imp["ef"], imp["ef"] / cl.U32)
    cmp("F_tau", o.F_tau - imp["tau"], imp["et"], imp["et"] / cl.U32)
    return worst


@pytest.mark.parametrize("name", cl.NAMES)
def test_restatements_match_the_double_oracle(name):
    lay = cl.layout(name)
    o, pre, r = run_oracle(lay, np.float64)
    R = restate(lay, o, pre, sequential=False)
    worst = _check(lay, o, pre, r, R, False, name)
    assert all(v <= 1.0 for v in worst.values()), worst


@pytest.mark.parametrize("name", cl.NAMES)
def test_float_oracle_within_the_bounds(name):
    lay = cl.layout(name)
    o, pre, r = run_oracle(lay, np.float32)
    R = restate(lay, o, pre, sequential=True)
    worst = _check(lay, o, pre, r, R, True, name)
    for k, v in worst.items():
        hs.record(f"float oracle within the contact bound: {name} {k}", v)
    assert all(v <= 1.0 for v in worst.values()), worst


def test_exact_search_root_of_the_restated_slope():
    """the double oracle's exact line search ends where the restated dE/dalpha vanishes (sign and scale of dE)"""
    lay = cl.layout("regimes_soft")
    o, pre, r = run_oracle(lay, np.float64, exact=True)
    R = restate(lay, o, pre, sequential=False)
    gm, gv, gvs = pre
    ls = cl.line_search(lay, R["P"], R["wt"], R["keys"], R["mass_c"], R["T"], gm, gv, gvs, np.asarray(o.g_D, np.float64),
                        R["dr"]["nodes"], [0.0, r["alpha"], 1.0], derivs=True, vp=R["vp"])
    assert ls[0]["dE"] < 0
    a = ls[1]
    assert abs(a["dE"]) <= 1e-6 * abs(ls[0]["dE"]) + 1e-8 or (r["alpha"] == 1.0 and ls[2]["dE"] < 0), (a, ls[0])


def test_restatement_sees_a_one_node_slip():
    """the direction bound is tight enough to see one contact's stencil moved by one node"""
    lay = cl.layout("normals")
    o, pre, r = run_oracle(lay, np.float64)
    R = restate(lay, o, pre, sequential=False)
    keys2 = R["keys"].copy()
    keys2[3] = np.roll(keys2[3], 1)
    dr2 = cl.direction(lay, R["P"], R["wt"], keys2, R["mass_c"], R["T"], *pre)
    dr = R["dr"]
    common, i1, i2 = np.intersect1d(dr["nodes"], dr2["nodes"], return_indices=True)
    ok = dr["dof"][i1] & dr2["dof"][i2]
    assert cl.margin(np.abs(dr["D"][i1][ok] - dr2["D"][i2][ok]), dr["eD"][i1][ok]) > 100
