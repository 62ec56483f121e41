"""The halo layouts of tests/halo_layouts.py on the CPU: every layout reaches what it claims, the restatements of the
pack, the add, the buffer layout and the split update's two passes hold together, and a node sum formed in two float32
halves stays inside the bound that tests/test_halo_exchange_gpu.py uses for two ranks against their union."""
import numpy as np
import pytest

from tests import halo_layouts as hl
from tests import transfer_layouts as tl


def _p2g(lay, stress=True):
    z = np.zeros_like(lay["taus"]), np.zeros_like(lay["forces"])
    taus, forces = (lay["taus"], lay["forces"]) if stress else z
    return tl.p2g64(lay["pos"], lay["vel"], lay["C"], lay["mass"], taus, forces, hl.BITS, lay["gravity_axis"])


def _zone_ids(act, lo=hl.ZLO, hi=hl.ZHI):
    bx = hl.block_coords(act)[0]
    return set(np.asarray(act)[(bx >= lo) & (bx <= hi)].tolist())


def test_morton_ids_restate_the_cell_keys():
    g = np.stack(np.meshgrid(*(np.arange(hl.NB),) * 3, indexing="ij"), -1).reshape(-1, 3)
    ids = hl.block_id(g[:, 0], g[:, 1], g[:, 2])
    assert np.array_equal(np.sort(ids), np.arange(hl.NBLOCKS))
    assert np.array_equal(ids, tl.cell_key(4 * g[:, 0], 4 * g[:, 1], 4 * g[:, 2]) >> 6)
    bx, by, bz = hl.block_coords(ids)
    assert np.array_equal(np.stack([bx, by, bz], -1), g)
    assert int(hl.block_id(1, 0, 0)) == 4 and int(hl.block_id(0, 1, 0)) == 2 and int(hl.block_id(0, 0, 1)) == 1


def test_buffer_layout_round_trip():
    for cap in (1, 3, 4, 143, 256):
        assert hl.buffer_bytes(cap) % 16 == 0 and hl.buffer_bytes(cap) >= 16 + 4 * cap + 1024 * cap
        rng = np.random.default_rng(cap)
        ent = [(int(i), rng.normal(size=(64, 4)).astype(np.float32)) for i in rng.permutation(4096)[:max(cap - 1, 1)]]
        w = hl.write_buffer(cap, ent, extra_words=8)
        n, ids, data, tail = hl.read_buffer(w, cap)
        assert n == len(ent) and (tail == hl.FILL).all() and len(tail) == 8
        assert ids[:n].tolist() == [i for i, _ in ent] and (ids[n:] == hl.FILL).all()
        assert all(np.array_equal(data[k], hl.words(d)) for k, (_, d) in enumerate(ent))
        assert (data[n:] == hl.FILL).all()


def test_pack_and_add_restatements_on_a_small_case():
    act = np.sort(hl.block_id(np.array([5, 6, 9, 10, 9]), np.array([0, 15, 3, 3, 15]), np.array([2, 15, 0, 3, 7])))
    raw = np.zeros((hl.NCELLS, 4), np.float32)
    rng = np.random.default_rng(0)
    for a in act:
        raw[a * 64:(a + 1) * 64] = rng.normal(size=(64, 4))
    ref = hl.pack_ref(act, raw, 6, 9, 0)
    assert set(ref) == {int(hl.block_id(6, 15, 15)), int(hl.block_id(9, 3, 0)), int(hl.block_id(9, 15, 7))}
    assert hl.zone_blocks(act, 6, 9) == 3
    sh = hl.pack_ref(act, raw, 6, 9, +7)    # 9 + 7 leaves [0, 16)
    assert set(sh) == {int(hl.block_id(13, 15, 15))}
    assert np.array_equal(sh[int(hl.block_id(13, 15, 15))], raw[int(hl.block_id(6, 15, 15)) * 64:][:64])
    # the add: listed and active blocks only, in float32
    other = int(hl.block_id(7, 7, 7))
    out = hl.add_ref(raw, act, [(other, np.ones((64, 4), np.float32)), (int(act[0]), np.full((64, 4), 0.1, np.float32))])
    want = raw.copy()
    want[act[0] * 64:(act[0] + 1) * 64] += np.float32(0.1)
    assert np.array_equal(hl.words(out), hl.words(want))
    assert not out[other * 64:(other + 1) * 64].any()


def test_the_two_passes_of_the_split_update_cover_every_block_once_and_in_order():
    bx = np.arange(hl.NB)
    for zones in ([(6, 9)], [(2, 5), (6, 9)], [(0, 1), (14, 15)], [(4, 7), (8, 11)], []):
        g0, g1 = hl.selected(bx, zones, 0), hl.selected(bx, zones, 1)
        p0, p1 = hl.selected_pm1(bx, zones, 0), hl.selected_pm1(bx, zones, 1)
        assert (g0 ^ g1).all() and (p0 ^ p1).all()          # every block in exactly one pass
        assert hl.selected(bx, zones, -1).all() and hl.selected_pm1(bx, zones, -1).all()
        # GridToParticle before the exchange gathers from blocks that the update before the exchange has finished:
        # none of the three x layers a home block's stencils reach lies in a zone
        for b in bx[p0]:
            assert all(g0[n] for n in (b - 1, b, b + 1) if 0 <= n < hl.NB)
        assert (g1 <= p1).all()                              # a zone block's own particles wait for the exchange


@pytest.mark.parametrize("name", hl.NAMES)
def test_layout_reaches_what_it_claims(name):
    L = hl.layout(name)
    u, le, ri = L["union"], L["left"], L["right"]
    cl = L["claims"]
    # the sides partition the union and carry its state
    both = np.r_[le["orig"], ri["orig"]]
    assert np.array_equal(np.sort(both), np.arange(u["nf"] + u["nv"]))
    for s in (le, ri):
        for k in ("pos", "vel", "C", "vol", "mass"):
            assert np.array_equal(s[k], u[k][s["orig"]])
        assert s["pos"].shape == (s["nf"] + s["nv"], 3) and s["nf"] * 3 == s["nv"]
        # a face at the centroid of its corners, as the engine's re-sort forms it
        c = s["pos"][s["nf"]:].reshape(-1, 3, 3)
        assert np.array_equal(s["pos"][:s["nf"]], ((c[:, 0] + c[:, 1]) + c[:, 2]) / np.float32(3))
    hi = (1 << hl.BITS) - 3
    r = {}
    for key, s in (("left", le), ("right", ri), ("union", u)):
        t = tl.f32(s["pos"]).astype(np.float64) * (1 << hl.BITS) - 0.5
        assert (t >= 0).all() and (t < hi + 1).all()
        bn = tl.binning(s)
        assert ((bn["r"] >= 0) & (bn["r"] <= 7)).all() and bn["margin"].min() >= hl.BIN_MARGIN
        r[key] = _p2g(s)
    # a rank keeps its stencils inside the zone: outside it no node is reached from both sides
    xyz = tl.key_coords(hl.BITS)
    outside = ~hl.in_zone(xyz[:, 0] >> 2, [(hl.ZLO, hl.ZHI)])
    assert not ((r["left"]["N"] > 0) & (r["right"]["N"] > 0) & outside).any()
    assert ((r["left"]["N"] > 0) & (r["right"]["N"] > 0)).any() or name == "empty"
    # the right set in a frame of its own: the move is exact in float32 (relabel's right set reaches x = 0: pitch 0 only)
    if name != "relabel":
        sh = hl.side(name, "right", hl.PITCH)
        assert np.array_equal(sh["pos"][:, 0].astype(np.float64) + hl.PITCH / 16.0, ri["pos"][:, 0].astype(np.float64))
        assert np.array_equal(sh["pos"][:, 1:], ri["pos"][:, 1:]) and (sh["pos"][:, 0] > 0).all()
        assert np.array_equal(sh["cloths"][0][0][:, 0].astype(np.float64) + hl.PITCH / 16.0,
                              ri["cloths"][0][0][:, 0].astype(np.float64))
        bx, by, bz = hl.block_coords(hl.active_ref(sh))
        assert np.array_equal(hl.active_ref(ri), np.sort(hl.block_id(bx + hl.PITCH, by, bz)))
    act = {k: hl.active_ref(s) for k, s in (("left", le), ("right", ri))}
    zl, zr = _zone_ids(act["left"]), _zone_ids(act["right"])
    if "both_reach" in cl:
        lo, hi_c = cl["both_reach"]
        for s in (le, ri):
            b, _ = tl.base_cells(s["pos"], hl.BITS)
            assert set(range(lo, hi_c + 1)) <= set(b[:, 0].tolist())
        for k in ("left", "right"):   # ... so both reach every node column of the zone
            cols = set(xyz[r[k]["N"] > 0, 0].tolist())
            assert set(range(4 * hl.ZLO, 4 * hl.ZHI + 4)) <= cols
        assert len(zl) >= cl["zone_active_min"] and len(zr) >= cl["zone_active_min"]
        assert len(zl & zr) >= cl["zone_active_min"]
    if cl.get("one_sided"):
        assert len(zl - zr) > 20 and len(zr - zl) > 20 and len(zl & zr) > 20
        # and the blocks of one side only hold mass there
        for mine, other in (("left", zr), ("right", zl)):
            touched = set(np.flatnonzero(r[mine]["flags"]).tolist())
            assert len((touched & _zone_ids(act[mine])) - other) >= 4 * 2     # four x layers, two z blocks
    if cl.get("corners"):
        for z in (zl, zr):
            _, by, bz = hl.block_coords(np.array(sorted(z)))
            assert {0, hl.NB - 1} <= set(by.tolist()) and {0, hl.NB - 1} <= set(bz.tolist())
            assert max(z) >= int(hl.block_id(8, hl.NB - 1, hl.NB - 1))      # the highest bit of every triple
        for k in ("left", "right"):   # nodes in the wall band hold mass
            on = r[k]["N"] > 0
            assert (on & (xyz[:, 1] < tl.WALL)).any() and (on & (xyz[:, 2] >= 64 - tl.WALL)).any()
        assert (r["right"]["N"][xyz[:, 0] < tl.WALL] > 0).any() and (r["right"]["N"][xyz[:, 0] >= 64 - tl.WALL] > 0).any()
        raw = hl.raw_dense(r["right"]["m"], r["right"]["mv"])
        seen = set()
        for lo, hi_z, shift in L["packs"]:
            ref = hl.pack_ref(act["right"], raw, lo, hi_z, shift)
            n = hl.zone_blocks(act["right"], lo, hi_z)
            bx = hl.block_coords(np.array(sorted(_zone_ids(act["right"], lo, hi_z)), np.int64))[0]
            assert len(ref) == int(((bx + shift >= 0) & (bx + shift < hl.NB)).sum())
            seen.add("all" if len(ref) == n and n else "none" if not ref and n else "some" if ref else "empty zone")
            if ref:
                nbx = hl.block_coords(np.array(sorted(ref)))[0]
                assert nbx.min() >= max(lo + shift, 0) and nbx.max() <= min(hi_z + shift, hl.NB - 1)
        assert {"all", "none", "some"} <= seen, seen
    if "vol_decades" in cl:
        assert np.log10(u["vol"].max() / u["vol"].min()) > 5.5
        # opposite momenta: without stress the two halves cancel to rounding on the axes without gravity
        a, b = _p2g(le, stress=False), _p2g(ri, stress=False)
        ax = [d for d in range(3) if d != u["gravity_axis"]]
        both_n = (a["N"] > 0) & (b["N"] > 0)
        s, mag = np.abs(a["mv"] + b["mv"])[:, ax], (np.abs(a["mv"]) + np.abs(b["mv"]))[:, ax]
        cancel = both_n[:, None] & (mag > 0) & (s <= 1e-5 * mag)
        assert cancel.any(axis=1).sum() > 50
        nf = u["nf"]
        for pa, pb in cl["pairs"]:
            assert np.array_equal(u["pos"][pa], u["pos"][pb]) and np.array_equal(u["mass"][pa], u["mass"][pb])
            assert np.array_equal(u["C"][pa], -u["C"][pb])
            assert np.array_equal(u["pos"][nf + 3 * pa:nf + 3 * pa + 3], u["pos"][nf + 3 * pb:nf + 3 * pb + 3])
        # rest shape = shape
        assert np.array_equal(u["cloths"][0][0], u["pos"][nf:])
        # node rows of one side only, inside blocks that are active on both
        for x, y_l, y_r, z in cl["rows"]:
            k_l, k_r = int(tl.cell_key(x, y_l, z)), int(tl.cell_key(x, y_r, z))
            assert k_l >> 6 == k_r >> 6 and (k_l >> 6) in (zl & zr)
            assert a["N"][k_l] > 0 and b["N"][k_l] == 0 and a["N"][k_r] == 0 and b["N"][k_r] > 0
    if cl.get("left_zone_empty"):
        assert len(zl) == 0 and len(zr) > 20
        assert not (set(act["left"].tolist()) & set(act["right"].tolist()))


@pytest.mark.parametrize("name", hl.NAMES)
def test_a_sum_in_two_float32_halves_stays_inside_the_union_bound(name):
    """f32(f32(S_L) + f32(S_R)) against the float64 sum over the union, per node: inside tl's P2G bound for the union
    plus 3 u A_n (halo_layouts docstring) -- here without the fixed-point term, which only widens it"""
    from tests.helpers import MARGINS
    L = hl.layout(name)
    a, b, r = _p2g(L["left"]), _p2g(L["right"]), _p2g(L["union"])
    bm, bmv = hl.union_bounds(r, None)
    m = tl.f32(a["m"]) + tl.f32(b["m"])
    mv = tl.f32(a["mv"]) + tl.f32(b["mv"])
    assert m.dtype == np.float32 and mv.dtype == np.float32
    wm = tl.margin(np.abs(m - r["m"]), bm)
    wmv = tl.margin(np.abs(mv - r["mv"]), bmv)
    for what, w in (("mass", wm), ("momentum", wmv)):
        MARGINS.append((w, f"halo layouts: two float32 halves against the union, {name} {what}", 1.0, w, w))
    assert wm <= 1.0 and wmv <= 1.0, (wm, wmv)
    # ... and the 3 u A_n alone (no kernel, no chain of L_n roundings) already covers this host evaluation
    assert tl.margin(np.abs(m - r["m"]), 3.0 * tl.U32 * r["A_m"] + 1e-13 * r["A_m"]) <= 1.0
    assert tl.margin(np.abs(mv - r["mv"]), 3.0 * tl.U32 * r["A_mv"] + 1e-13 * r["A_mv"]) <= 1.0
    # the halves' terms add up to the union's: what makes the union's bound cover each half
    assert np.allclose(a["A_m"] + b["A_m"], r["A_m"], rtol=1e-12, atol=0)
    assert np.array_equal(a["N"] + b["N"], r["N"]) and (np.maximum(a["L"], b["L"]) <= r["L"]).all()
    assert tl.fixed_quanta(L["left"]["mass"])[1] <= tl.fixed_quanta(L["union"]["mass"])[1]
    assert tl.fixed_quanta(L["right"]["mass"])[1] <= tl.fixed_quanta(L["union"]["mass"])[1]
