"""The partition of tests/cut_layouts.py on the CPU: every layout reaches what it claims across the cut, the split accounts
for every contact and every node once, the per-rank float64 node sums add up to the union's (1e-12 of scale), what a rank
holds after the exchange -- fl(own + neighbour's) -- lies inside the bound widened by one addition, and so does the
float build of the oracle on the union (sequential sums, L_n = N_n + 1 where a neighbour's sums arrive)."""
import numpy as np
import pytest

from tests import contact_layouts as cl
from tests import cut_layouts as ct
from tests import transfer_layouts as tl
from tests.test_contact_layouts import _check, restate, run_oracle

IDS = [ct.case_id(c) for c in ct.CASES]
# cl's layouts were not built around a cut: these three have fewer than 100 nodes that see contacts of both ranks of the
# cut at block 8 (their contacts next to cell 32 lie on one side); the counts are pinned here, `cut` covers the cases
SHARED_NODES_BELOW_100 = {"regimes_mu0": 64, "occupancy": 0, "fringe": 0}


def _restated(lay):
    """stencil, contact terms at the particle velocities and a unit-mass grid at rest: the node sums do not depend on it"""
    P = cl.params32(lay["params"])
    cp = lay["cp"]
    vp = lay["vel"][cp["particle"]].astype(np.float64)
    mass_c = lay["mass"][cp["particle"]].astype(np.float64)
    b, wt, keys, T = cl.prepare(lay, P, None, None, None, vp, mass_c)
    ncell = 1 << (3 * lay["bits"])
    grid = (np.ones(ncell), np.zeros((ncell, 3)), np.zeros((ncell, 3)))
    return P, vp, mass_c, b, wt, keys, T, grid


@pytest.mark.parametrize("case", ct.CASES, ids=IDS)
def test_split_accounts_for_every_contact_and_node_once(case):
    name, cuts, Z = case
    lay = ct.layout(name)
    parts = ct.split(lay, cuts, Z)
    nc = len(lay["cp"]["particle"])
    seen = np.concatenate([p["sel"] for p in parts])
    assert len(seen) == nc and np.array_equal(np.sort(seen), np.arange(nc))
    owners = sum(p["owned"].astype(np.int64) for p in parts)
    assert (owners == 1).all()
    assert (ct.particle_owner(lay, cuts) >= 0).all()
    b, wt, keys = cl.stencil(lay)
    for p in parts:       # a contact's rank is the rank of its base cell; its nodes lie at most two cells into a neighbour's slab
        lo, hi = p["own"]
        bx = b[p["sel"], 0]
        assert ((bx >= lo) & (bx < hi)).all()
        x = ct.node_x(p["flags"])
        assert len(x) == 0 or (x.min() >= lo and x.max() <= hi + 1)
        for s, (blo, bhi) in p["zones"].items():      # ... inside the zone it shares with that neighbour
            beyond = x[(x >= hi)] if s > p["rank"] else x[x < lo]
            assert ((beyond >> 2 >= blo) & (beyond >> 2 <= bhi)).all()
    lists = ct.node_lists(parts)
    union = np.unique(keys)
    for p, l in zip(parts, lists):
        assert np.isin(p["flags"], l).all() and np.isin(l, union).all()
    # every node that sees a contact is listed on its owner (the global sums take it from there)
    for p, l in zip(parts, lists):
        assert np.isin(union[p["owned"][union]], l).all()


@pytest.mark.parametrize("name", cl.NAMES)
def test_the_cut_at_block_8_goes_through_the_contact_layouts(name):
    lay = ct.layout(name)
    parts = ct.split(lay, ct.TWO, 1)
    assert all(len(p["sel"]) >= 50 for p in parts), [len(p["sel"]) for p in parts]
    both = np.intersect1d(parts[0]["flags"], parts[1]["flags"])
    if name in SHARED_NODES_BELOW_100:
        assert len(both) == SHARED_NODES_BELOW_100[name]
    else:
        assert len(both) >= 100, len(both)


def test_further_cuts_go_through_regimes_mu0_and_fringe():
    """block 7 through regimes_mu0: more than 100 shared nodes; block 11 through fringe's masses over six decades: the
    most a block boundary gives there (83 shared nodes, pinned); both ranks with 50 contacts and more"""
    want = {"regimes_mu0": 205, "fringe": 83}
    for name, cuts, Z in ct.MORE:
        parts = ct.split(ct.layout(name), cuts, Z)
        assert all(len(p["sel"]) >= 50 for p in parts)
        both = np.intersect1d(parts[0]["flags"], parts[1]["flags"])
        assert len(both) == want[name], (name, len(both))
        assert len(ct.received(parts, ct.node_lists(parts))) == len(both)
    assert want["regimes_mu0"] >= 100


@pytest.mark.parametrize("Z", (1, 2))
def test_cut_reaches_what_it_claims(Z):
    lay = ct.layout("cut")
    assert lay["claims"]["cut_cases"] == ("a", "b", "c", "d", "e", "f")
    P, vp, mass_c, b, wt, keys, T, grid = _restated(lay)
    assert T["sep_margin"].min() > 10.0
    parts = ct.split(lay, ct.TWO, Z)
    lists = ct.node_lists(parts)
    rec = ct.received(parts, lists)
    un = cl.direction(lay, P, wt, keys, mass_c, T, *grid, received=rec)
    dof = np.zeros(1 << (3 * lay["bits"]), bool)
    dof[un["nodes"][un["dof"] & ~un["amb"]]] = True
    # base cells in every column from cut - 4 to cut + 3, on the rank that owns the column
    for c in range(ct.CUT - 4, ct.CUT + 4):
        r = int(c >= ct.CUT)
        assert (b[parts[r]["sel"], 0] == c).sum() >= 40, c
    # a. listed through the flag exchange alone: nodes the rank owns (it counts their DoFs) and nodes it does not
    for p, l in zip(parts, lists):
        only = np.setdiff1d(l, p["flags"])
        assert (~p["owned"][only] & dof[only]).sum() >= 10, p["rank"]
    only1 = np.setdiff1d(lists[1], parts[1]["flags"])
    assert (parts[1]["owned"][only1] & dof[only1]).sum() >= 10
    assert set(ct.node_x(only1[parts[1]["owned"][only1]]).tolist()) == {ct.CUT, ct.CUT + 1}
    # b. nodes reached by both ranks' contacts in every regime
    app = ~T["sep"]
    reg = {"separating": T["sep"], "sliding": app & (T["ut"] >= 100 * cl.EPSV), "sticking": app & (T["ut"] <= 0.01 * cl.EPSV),
           "transitional": app & (T["ut"] > 0.1 * cl.EPSV) & (T["ut"] < 10 * cl.EPSV)}
    assert set(reg) == set(cl.REGIMES)
    for what, m in reg.items():
        per = [np.unique(keys[p["sel"][m[p["sel"]]]]) for p in parts]
        assert len(np.intersect1d(per[0], per[1])) >= 10, what
    assert len(rec) >= 100
    # c. a zone block that holds an owned contact of the sender and lies more than two blocks (the reach of a particle's
    #    27 active blocks, and one more) from every particle the receiver holds
    hb = ct.held(lay, ct.TWO, Z)
    base = tl.base_cells(lay["pos"], lay["bits"])[0] >> 2
    for s, r in ((0, 1), (1, 0)):
        blo, bhi = parts[s]["zones"][r]
        cb = np.unique(b[parts[s]["sel"]] >> 2, axis=0)
        near = np.unique(base[hb[r]], axis=0)
        found = 0
        for blk in cb:
            act = blk[None] + np.stack(np.meshgrid(*[np.arange(-1, 2)] * 3, indexing="ij"), -1).reshape(-1, 3)
            act = act[(act[:, 0] >= blo) & (act[:, 0] <= bhi)]
            for a in act:
                found += int(np.abs(near - a[None]).max(axis=1).min() > 2)
        assert found >= 1, (s, r)
    # d. listed nodes whose own sums are exactly zero: the nodes of a, and in the second solve nodes that had own sums
    nodes, sums = ct.rank_sums(lay, P, wt, keys, mass_c, T, grid, parts)
    lay2 = ct.sub_layout(lay, lay["second_pairs"])
    P2, vp2, mass2, b2, wt2, keys2, T2, _ = _restated(lay2)
    parts2 = ct.split(lay2, ct.TWO, Z)
    lists2 = ct.node_lists(parts2)
    nodes2, sums2 = ct.rank_sums(lay2, P2, wt2, keys2, mass2, T2, grid, parts2)
    had = nodes[np.abs(sums[1][0]).sum(1) + np.abs(sums[1][1]).sum(1) > 0]
    zero2 = nodes2[np.abs(sums2[1][0]).sum(1) + np.abs(sums2[1][1]).sum(1) == 0]
    now_zero = np.intersect1d(np.intersect1d(had, zero2), lists2[1])
    assert len(now_zero) >= 20 and len(parts2[1]["sel"]) >= 50
    # e. below the DoF threshold on each rank, above it in total, clear of the bounds
    common, per, un_e = ct._e_nodes(lay, parts)
    at = np.searchsorted(un_e["nodes"], common)
    below = np.ones(len(common), bool)
    for hF, gF, eHF, eGF in per:
        below &= (hF + eHF < cl.THRESH) & (gF + eGF < cl.THRESH) & ((hF > 0) | (gF > 0))
    above = un_e["dof"][at] & ~un_e["amb"][at]
    assert (below & above).sum() >= 1
    assert np.isin(common[below & above], rec).all()
    # f. contacts in the zone's outermost blocks
    for p, blk in zip(parts, (ct.CUT_BLOCK - Z, ct.CUT_BLOCK + Z - 1)):
        assert ((b[p["sel"], 0] >> 2) == blk).sum() >= 50


@pytest.mark.parametrize("name", ("three", "three_empty"))
def test_three_reaches_what_it_claims(name):
    lay = ct.layout(name)
    P, vp, mass_c, b, wt, keys, T, grid = _restated(lay)
    cuts, Z = ct.THREE, 1
    assert cuts[2] - cuts[1] == 2 * Z            # the middle slab is exactly two zones wide: its zones abut
    parts = ct.split(lay, cuts, Z)
    assert parts[1]["zones"] == {0: (6, 7), 2: (8, 9)}
    lists = ct.node_lists(parts)
    counts = [len(p["sel"]) for p in parts]
    empty = lay["claims"]["empty_rank"]
    assert all(n >= 100 for r, n in enumerate(counts) if r != empty), counts
    assert len(np.intersect1d(parts[0]["flags"], parts[1]["flags"])) >= 50
    un = cl.direction(lay, P, wt, keys, mass_c, T, *grid)
    dof = np.zeros(1 << (3 * lay["bits"]), bool)
    dof[un["nodes"][un["dof"] & ~un["amb"]]] = True
    if empty is None:
        assert len(np.intersect1d(parts[1]["flags"], parts[2]["flags"])) >= 50
    else:
        # the rank without a contact owns DoFs that its neighbour's contacts make: it has to take part
        assert counts[empty] == 0
        assert (parts[empty]["owned"][lists[empty]] & dof[lists[empty]]).sum() >= 20


@pytest.mark.parametrize("case", ct.CASES, ids=IDS)
def test_partition_sums_add_up_to_the_union(case):
    """sum over the ranks of the float64 node sums = the union's, 1e-12 of the sum of magnitudes; and fl(own + neighbour's)
    of the sums rounded to float lies inside the bound of L_n + 1"""
    name, cuts, Z = case
    lay = ct.layout(name)
    P, vp, mass_c, b, wt, keys, T, grid = _restated(lay)
    parts = ct.split(lay, cuts, Z)
    lists = ct.node_lists(parts)
    rec = ct.received(parts, lists)
    un = cl.direction(lay, P, wt, keys, mass_c, T, *grid, received=rec)
    plain = cl.direction(lay, P, wt, keys, mass_c, T, *grid)
    nodes, sums = ct.rank_sums(lay, P, wt, keys, mass_c, T, grid, parts)
    assert np.array_equal(nodes, un["nodes"])
    # the widened bound differs from cl's exactly at the nodes that receive, and is larger there
    at = np.isin(nodes, rec)
    assert np.array_equal(un["L"], plain["L"] + at) and (un["eHn"][at] >= plain["eHn"][at]).all() and (not at.any() or (un["eHn"][at] > plain["eHn"][at]).any())
    assert np.array_equal(un["eHn"][~at], plain["eHn"][~at])
    f = un["inv"].reshape(-1)
    m = mass_c[:, None]
    AH, AG = np.zeros(len(nodes)), np.zeros(len(nodes))
    np.add.at(AH, f, (m * wt * wt * T["MH"][:, None]).reshape(-1))
    np.add.at(AG, f, (m * wt * T["MG"][:, None]).reshape(-1))
    H = sum(s[0] for s in sums)
    G = sum(s[1] for s in sums)
    assert cl.margin(np.abs(H - un["Hn"]), 1e-12 * AH[:, None] + 1e-300) <= 1.0
    assert cl.margin(np.abs(G - un["Gn"]), 1e-12 * AG[:, None] + 1e-300) <= 1.0
    for p, l in zip(parts, lists):
        on = np.isin(nodes, l)
        nb = [sums[s] for s in p["zones"]]
        H32 = ct.held32(sums[p["rank"]][0], [x[0] for x in nb]).astype(np.float64)
        G32 = ct.held32(sums[p["rank"]][1], [x[1] for x in nb]).astype(np.float64)
        assert cl.margin(np.abs(H32 - un["Hn"])[on], un["eHn"][on][:, None]) <= 1.0
        assert cl.margin(np.abs(G32 - un["Gn"])[on], un["eGn"][on][:, None]) <= 1.0
        # both ranks of a cut hold the same bits at the nodes they share
        for s in p["zones"]:
            sh = on & np.isin(nodes, lists[s])
            Hs = ct.held32(sums[s][0], [sums[q][0] for q in parts[s]["zones"]])
            assert np.array_equal(Hs[sh].view(np.uint32), tl.f32(H32)[sh].view(np.uint32))


@pytest.mark.parametrize("case", [c for c in ct.CASES if c[0] in ct.NAMES and c[2] == 1] + [("bodies", ct.TWO, 1)],
                         ids=lambda c: ct.case_id(c))
def test_float_oracle_within_the_widened_bounds(case):
    """the float build of the oracle on the union, adding sequentially: L_n = N_n + 1 where a neighbour's sums arrive"""
    name, cuts, Z = case
    lay = ct.layout(name)
    parts = ct.split(lay, cuts, Z)
    rec = ct.received(parts, ct.node_lists(parts))
    o, pre, r = run_oracle(lay, np.float32)
    R = restate(lay, o, pre, sequential=True, received=rec)
    assert np.array_equal(R["dr"]["L"], R["dr"]["N"] + np.isin(R["dr"]["nodes"], rec))
    worst = _check(lay, o, pre, r, R, True, name)
    assert all(v <= 1.0 for v in worst.values()), worst
    o64, pre64, r64 = run_oracle(lay, np.float64)
    worst = _check(lay, o64, pre64, r64, restate(lay, o64, pre64, sequential=False, received=rec), False, name)
    assert all(v <= 1.0 for v in worst.values()), worst
