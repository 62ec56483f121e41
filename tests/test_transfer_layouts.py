"""The transfer layouts of tests/transfer_layouts.py on the CPU: every layout reaches what it claims, the float64
restatements of ParticleToGrid, UpdateGrid and GridToParticle agree with the double build of the oracle, and the
per-node / per-particle bounds are real rounding bounds (the float build of the oracle stays within them)."""
import numpy as np
import pytest

from tests import harness as hs
from tests import transfer_layouts as tl


@pytest.mark.parametrize("name", tl.NAMES)
def test_layout_reaches_what_it_claims(name):
    lay = tl.layout(name)
    cl = lay["claims"]
    n = lay["nf"] + lay["nv"]
    assert lay["pos"].shape == (n, 3) and lay["C"].shape == (n, 9) and lay["vol"].shape == (n,)
    bn = tl.binning(lay)
    hi = (1 << lay["bits"]) - 3
    # every particle inside the domain (t in [0, hi + 1)) and inside its tile (no MPM_ERR_DRIFT)
    t = tl.f32(lay["pos"]).astype(np.float64) * (1 << lay["bits"]) - 0.5
    assert (t >= 0).all() and (t < hi + 1).all()
    assert ((bn["r"] >= 0) & (bn["r"] <= 7)).all()
    if "runs" in cl:
        runs = tl.run_lengths(lay)
        homes = set()
        for want, cell in cl["runs"].items():
            key = int(tl.cell_key(*cell))
            assert runs.get(key) == want, (want, cell, runs.get(key))
            homes.add(tuple(np.asarray(cell) >> 2))
        assert len(homes) == len(tl.RUNS)
        assert {r % 4 for r in tl.RUNS} == {0, 1, 2, 3}
        # and the particles of every such cell are binned to that cell's block
        b, _ = tl.base_cells(bn["x"], lay["bits"])
        for cell in cl["runs"].values():
            sel = (b == np.asarray(cell)).all(axis=1)
            assert (bn["block"][sel] == np.asarray(cell) >> 2).all()
    if "split_block" in cl:
        blk, lo, hi_items = cl["split_block"]
        counts = tl.home_counts(lay)
        assert sum(counts[blk]) > 16 * 64
        items = tl.work_items(lay)
        assert lo <= items[blk] <= hi_items, items[blk]
        assert tl.work_items(lay, tl.ITEM_GROUPS_SMALL)[blk] >= 2
    if "free_zone_classes" in cl:
        assert bn["margin"].min() >= tl.BIN_MARGIN
        classes = {tuple(c) for c in bn["cls"]}
        assert classes == {(a, b, c) for a in range(4) for b in range(4) for c in range(4)}
        # faces and vertices both reach every class
        for part in (slice(0, lay["nf"]), slice(lay["nf"], None)):
            assert len({tuple(c) for c in bn["cls"][part]}) == 64
    if "walls" in cl:
        bits = lay["bits"]
        N = 1 << bits
        b, fx = tl.base_cells(lay["pos"], bits)
        for d in range(3):
            assert (b[:, d] == 0).any() and (b[:, d] == hi).any()
            u = tl.f32(lay["pos"][:, d]).astype(np.float64) * N
            assert (u - 0.5 == 0).any() and (u - 0.5 == 1).any() and (u - 0.5 == hi).any()
            top = u[u - 0.5 < hi + 1].max()
            assert top - 0.5 > hi + 1 - 1e-5 and np.nextafter(np.float32(top / N), np.float32(1)) * N - 0.5 >= hi + 1
            # wall nodes reached, with velocities into and out of the wall on both sides
            low, high = b[:, d] < tl.WALL, b[:, d] + 2 >= N - tl.WALL
            v = lay["vel"][:, d]
            assert (v[low] < 0).any() and (v[low] > 0).any() and (v[high] > 0).any() and (v[high] < 0).any()
    if cl.get("face_only"):
        counts = tl.home_counts(lay)
        assert any(f > 0 and v == 0 for f, v in counts.values())
        assert any(f == 0 and v > 0 for f, v in counts.values())
    if cl.get("mixed_cells") or cl.get("shared_cells"):
        b, _ = tl.base_cells(bn["x"], lay["bits"])
        key = tl.cell_key(b[:, 0], b[:, 1], b[:, 2])
        if cl.get("mixed_cells"):
            assert np.intersect1d(key[:lay["nf"]], key[lay["nf"]:]).size > 0
        if cl.get("shared_cells"):
            nf0 = len(lay["cloths"][0][2])
            f0 = np.r_[key[:nf0], key[lay["nf"]:lay["nf"] + 3 * nf0]]
            f1 = np.r_[key[nf0:lay["nf"]], key[lay["nf"] + 3 * nf0:]]
            assert np.intersect1d(f0, f1).size > 20
            assert len(set(lay["mass"][:nf0].tolist()) & set(lay["mass"][nf0:lay["nf"]].tolist())) == 0
    if "vol_decades" in cl:
        assert np.log10(lay["vol"].max() / lay["vol"].min()) > 5.5
        sp = np.linalg.norm(lay["vel"][lay["nf"]:], axis=1)
        assert sp.min() < 3e-3 and sp.max() > 5.0
        cm = np.abs(lay["C"]).max(axis=1)
        assert cm.min() < 3e-3 and cm.max() > 5.0
    # the state is far from the fixed-point range (over-range is tested elsewhere)
    r = tl.p2g64(lay["pos"], lay["vel"], lay["C"], lay["mass"], lay["taus"], lay["forces"], lay["bits"], lay["gravity_axis"])
    q_m, q_p = tl.fixed_quanta(lay["mass"])
    assert np.abs(r["mv"]).max() / q_p < 2.0 ** 55


def _oracle(lay, real):
    """the layout in an oracle (density 1, volumes = the masses), its state set directly: the transfers are under test"""
    from oracle import oracle as orc
    o = orc.OracleMpm(lay["bits"], real=real)
    o.p.gravity_axis = lay["gravity_axis"]
    o.p.density = 1.0
    for rest, vel, idx in lay["cloths"]:
        o.add_qr_cloth(rest, vel, idx)
    o.finalize()
    for name, key in (("pos", "pos"), ("vel", "vel"), ("C", "C"), ("vol", "mass"), ("taus", "taus"), ("forces", "forces")):
        setattr(o, name, np.ascontiguousarray(np.asarray(lay[key], np.float32), dtype=real))
    return o


def _transfers(o):
    """P2G, grid update and G2P of oracle `o` with the restatement of each phase on the oracle's own inputs"""
    lay_bits, gax = o.domain_bits, int(o.p.gravity_axis)
    x0, v0, C0, m0, tau0, f0 = (np.asarray(getattr(o, a), np.float64).copy() for a in ("pos", "vel", "C", "vol", "taus", "forces"))
    o.particle_to_grid(tl.DT32)
    r = tl.p2g64(x0, v0, C0, m0, tau0, f0, lay_bits, gax)
    gm, gmv = o.g_m.copy(), o.g_mv.copy()
    flags = o.g_flags.copy()
    o.update_grid(-1)
    gv = o.g_mv.copy()
    o.grid_to_particle(tl.DT32)
    g = tl.g2p64(x0, gv, lay_bits)
    return r, (gm, gmv, flags), gv, g


@pytest.mark.parametrize("name", tl.NAMES)
def test_restatements_match_the_double_oracle(name):
    lay = tl.layout(name)
    o = _oracle(lay, np.float64)
    r, (gm, gmv, flags), gv, g = _transfers(o)
    assert np.array_equal(flags, r["flags"])
    for what, a, b, A in (("mass", gm, r["m"], r["A_m"]), ("momentum", gmv, r["mv"], r["A_mv"])):
        err = np.abs(a - b)
        assert (err <= 1e-12 * A + 1e-300).all(), (what, float((err / (A + 1e-300)).max()))
    # the grid update: the same correctly rounded division of the same sums
    v64 = tl.grid64(gm, gmv, lay["bits"])
    assert np.array_equal(v64, gv)
    # G2P against the same grid velocities
    s = tl.K * (tl.K_G2P_L + 16) * tl.U32
    for what, a, b, A in (("v", o.vel, g["v"], g["bv"] / s), ("C", o.C, g["C"], g["bC"] / s),
                          ("x", o.pos, g["x"], np.abs(g["x"]) + tl.DT32 * g["bv"] / s)):
        err = np.abs(np.asarray(a, np.float64) - b)
        assert (err <= 1e-12 * A + 1e-300).all(), (what, float((err / (A + 1e-300)).max()))


@pytest.mark.parametrize("name", tl.NAMES)
def test_float_oracle_within_the_rounding_bounds(name):
    """the bounds hold for an independent float32 evaluation of the same transfers: the float oracle, whose node sums
    are sequential over the particles (L_n replaced by the contributor count N_n, no fixed point)"""
    lay = tl.layout(name)
    o = _oracle(lay, np.float32)
    r, (gm, gmv, flags), gv, g = _transfers(o)
    assert np.array_equal(flags, r["flags"])
    bm, bmv = tl.p2g_bounds(r, None, L=r["N"])
    worst = {}
    worst["p2g mass"] = tl.margin(np.abs(gm - r["m"]), bm)
    worst["p2g momentum"] = tl.margin(np.abs(gmv - r["mv"]), bmv)
    worst["g2p v"] = tl.margin(np.abs(o.vel - g["v"]), g["bv"])
    worst["g2p C"] = tl.margin(np.abs(o.C - g["C"]), g["bC"])
    worst["g2p x"] = tl.margin(np.abs(o.pos - g["x"]), g["bx"])
    for k, v in worst.items():
        hs.record(f"float oracle within the transfer bound: {name} {k}", v)
    assert all(v <= 1.0 for v in worst.values()), worst
    # (and the float grid update is the float32 quotient of its own sums)
    assert np.array_equal(tl.grid32(gm, gmv, lay["bits"]), gv)


def test_restatement_sees_a_one_node_slip():
    """the bound is tight enough to see a one-node slip: one particle's stencil moved by one node breaks it by far"""
    lay = tl.layout("dense")
    args = (lay["pos"], lay["vel"], lay["C"], lay["mass"], lay["taus"], lay["forces"], lay["bits"], lay["gravity_axis"])
    r = tl.p2g64(*args)
    bm, bmv = tl.p2g_bounds(r, tl.fixed_quanta(lay["mass"]))
    pos = lay["pos"].copy()
    pos[5, 0] += 1.0 / (1 << lay["bits"])
    r2 = tl.p2g64(pos, *args[1:])
    assert tl.margin(np.abs(r2["m"] - r["m"]), bm) > 100
    assert tl.margin(np.abs(r2["mv"] - r["mv"]), bmv) > 100
