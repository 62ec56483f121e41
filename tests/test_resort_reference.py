"""CPU checks of tests/resort_reference.py (no GPU): the integer layer against a brute-force construction in plain
Python loops that shares no helper with it, the claims of the layouts and sequences the GPU table tests run, the
rounding bound of the quiet time against a float32 restatement, and the (n, bits) grid of the radix sort test against a
Python copy of the sort's cost model."""
import numpy as np
import pytest

from tests import resort_reference as rr
from tests import transfer_layouts as tl


# ---- brute force: plain loops, its own Morton code -------------------------------------------------------------------
def _bf_block_id(x, y, z):
    b = 0
    for i in range(10):
        b |= ((x >> i) & 1) << (3 * i + 2) | ((y >> i) & 1) << (3 * i + 1) | ((z >> i) & 1) << (3 * i)
    return b


def _bf_block_xyz(b):
    x = y = z = 0
    for i in range(10):
        x |= ((b >> (3 * i + 2)) & 1) << i
        y |= ((b >> (3 * i + 1)) & 1) << i
        z |= ((b >> (3 * i)) & 1) << i
    return x, y, z


def _bf_nbr(b, o, nb):
    x, y, z = _bf_block_xyz(b)
    x, y, z = x + o // 9 - 1, y + (o // 3) % 3 - 1, z + o % 3 - 1
    if min(x, y, z) < 0 or max(x, y, z) >= nb:
        return -1
    return _bf_block_id(x, y, z)


def _brute(pkey, nf_in, nv_in, prm):
    Nf, nb = prm["Nf"], prm["nb"]
    parts = [(0, s) for s in range(nf_in)] + [(1, Nf + s) for s in range(nv_in)]
    live = [(t, s, int(pkey[s])) for t, s in parts if int(pkey[s]) != 0xFFFFFFFF]
    homes = sorted({k >> 6 for _, _, k in live})
    out = dict(home_block=homes, home_range=[], blkstart=[], groups=[], ngroups=[], goff=[], prefix=[])
    # canonical destinations: faces then vertices, by block, by cell, by previous slot
    dst = {s: -1 for _, s in parts}
    seg = {}
    run = [0, 0]
    for h, b in enumerate(homes):
        begin = list(run)
        pre = [[0] * 64, [0] * 64]
        merged = []
        for cell in range(64):
            for t in (0, 1):
                pre[t][cell] = run[t] - begin[t]
                mine = sorted(s for tt, s, k in live if tt == t and k == b * 64 + cell)
                lo = t * Nf + run[t]
                for s in mine:
                    dst[s] = t * Nf + run[t]
                    run[t] += 1
                    merged.append(t)
                for s in mine:
                    seg[s] = (lo, t * Nf + run[t])
        out["blkstart"].append(begin)
        out["prefix"].append(pre)
        rg = (begin[0], run[0], Nf + begin[1], Nf + run[1])
        out["home_range"].append(rg)
        ng = (len(merged) + 63) // 64
        gl = []
        for g in range(ng):
            f0 = sum(1 for t in merged[:64 * g] if t == 0)
            f1 = sum(1 for t in merged[:64 * g + 64] if t == 0)
            v0, v1 = min(64 * g, len(merged)) - f0, min(64 * g + 64, len(merged)) - f1
            gl.append((rg[0] + f0, rg[0] + f1, rg[2] + v0, rg[2] + v1))
        out["groups"].append(gl)
        out["ngroups"].append(ng)
        out["goff"].append(((rg[0] + rg[2] - Nf) >> 6) + h)
    out.update(dst=dst, seg=seg, nfa=run[0], nva=run[1])
    held_groups = (run[0] + run[1] + 63) // 64
    ig = prm["item_groups"]
    if held_groups < prm["item_small_below"]:
        ig = min(ig, prm["item_groups_small"])
    items, home_items = [], []
    for h, ng in enumerate(out["ngroups"]):
        ni = -(-ng // ig)
        home_items.append((len(items), ni))
        for k in range(ni):
            items.append((h, k * ng // ni, (k + 1) * ng // ni, 0))
    out.update(items=items, home_items=home_items, ig=ig)
    act = sorted({n for b in homes for n in (_bf_nbr(b, o, nb) for o in range(27)) if n >= 0})
    out["act_block"] = act
    lh = {b: h for h, b in enumerate(homes)}
    la = {b: a for a, b in enumerate(act)}
    out["lut_home"] = [lh.get(b, -1) for b in range(prm["nblocks"])]
    out["lut_act"] = [la.get(b, -1) for b in range(prm["nblocks"])]
    out["home_nbr_act"] = [[la.get(_bf_nbr(b, o, nb), -1) for o in range(27)] for b in homes]
    out["act_nbr_home"] = [[lh.get(_bf_nbr(b, o, nb), -1) for o in range(27)] for b in act]
    out["act_nbr_items"] = [[-1 if h < 0 else home_items[h][0] | (min(home_items[h][1], 127) << 24) for h in row]
                            for row in out["act_nbr_home"]]
    return out


def _random_case(seed):
    rng = np.random.default_rng(seed)
    bits = (4, 5, 6)[seed % 3]
    nb = 1 << (bits - 2)
    n = int(rng.choice([1, 2, 3, 17, 64, 65, 200, 1000, 5000])) if seed % 5 else int(rng.integers(1, 5001))
    # blocks: every face, edge and corner of the grid among them
    ends = [0, nb - 1]
    pool = [(x, y, z) for x in ends for y in ends for z in ends]                                   # corners
    pool += [tuple(int(v) for v in np.roll([e1, e2, int(rng.integers(0, nb))], r)) for e1 in ends for e2 in ends for r in range(3)]
    pool += [tuple(int(v) for v in np.roll([e1, int(rng.integers(0, nb)), int(rng.integers(0, nb))], r)) for e1 in ends for r in range(3)]
    pool += [tuple(int(v) for v in rng.integers(0, nb, 3)) for _ in range(6)]
    nblk = int(rng.integers(1, min(len(pool), max(2, n // 3 + 1)) + 1))
    blocks = [pool[i] for i in rng.choice(len(pool), nblk, replace=False)]
    mode = seed % 4                          # 0: mixed types, 1: faces only, 2: vertices only, 3: mixed with dropped ones
    n_f = {0: n // 3, 1: n, 2: 0, 3: n // 2}[mode]
    n_v = n - n_f
    Nf, Nv = n_f + int(rng.integers(0, 5)), n_v + int(rng.integers(0, 5))
    pkey = rng.integers(0, 1 << 30, Nf + Nv).astype(np.int64)        # (unlisted slots hold rubbish)
    slots = rr.listed_slots(Nf, n_f, n_v)
    heavy = rng.random() < 0.5                 # half the cases pile most particles into one block, few cells
    for s in slots:
        b = blocks[0] if heavy and rng.random() < 0.8 else blocks[int(rng.integers(0, nblk))]
        cell = int(rng.integers(0, 4 if heavy else 64))
        pkey[s] = _bf_block_id(*b) * 64 + cell
    if mode == 3:
        pkey[slots[rng.random(len(slots)) < 0.2]] = rr.SENTINEL
    prm = dict(Nf=Nf, Np=Nf + Nv, bits=bits, nb=nb, nblocks=nb ** 3, item_groups=int(rng.choice([3, 5, 48])),
               item_groups_small=int(rng.choice([1, 2, 4, 16])), item_small_below=int(rng.choice([0, 10, 6500])))
    return pkey, n_f, n_v, prm


@pytest.mark.parametrize("seed", range(36))
def test_integer_layer_against_brute_force(seed):
    pkey, n_f, n_v, prm = _random_case(seed)
    ref = rr.integer_layer(pkey, n_f, n_v, prm)
    bf = _brute(pkey, n_f, n_v, prm)
    eq = lambda a, b, what: np.testing.assert_array_equal(np.asarray(a, np.int64), np.asarray(b, np.int64).reshape(np.shape(a)), what)
    nh = len(bf["home_block"])
    eq(ref["home_block"], bf["home_block"], "home_block")
    eq(ref["home_range"], np.array(bf["home_range"]).reshape(nh, 4), "home_range")
    eq(ref["blkstart"], np.array(bf["blkstart"]).reshape(nh, 2), "blkstart")
    assert (ref["nfa_new"], ref["nva_new"]) == (bf["nfa"], bf["nva"])
    eq(ref["cell_prefix"], np.array(bf["prefix"]).reshape(nh, 2, 64), "cell prefixes")
    eq(ref["dst"], [bf["dst"][int(s)] for s in ref["slots"]], "canonical destinations")
    for s, lo, hi in zip(ref["slots"], ref["seg_lo"], ref["seg_hi"]):
        assert (int(lo), int(hi)) == bf["seg"].get(int(s), (-1, -1)), ("segment of slot", s)
    eq(ref["home_ngroups"], bf["ngroups"], "home_ngroups")
    eq(ref["group_offset"], bf["goff"], "group pool offsets")
    for h in range(nh):
        eq(ref["groups"][h], np.array(bf["groups"][h]).reshape(-1, 4), f"groups of home {h}")
    assert ref["ig"] == bf["ig"]
    eq(ref["home_items"], np.array(bf["home_items"]).reshape(nh, 2), "home_items")
    eq(ref["item_desc"], np.array(bf["items"]).reshape(-1, 4), "item_desc")
    eq(ref["act_block"], bf["act_block"], "act_block")
    eq(ref["lut_home"], bf["lut_home"], "lut_home")
    eq(ref["lut_act"], bf["lut_act"], "lut_act")
    eq(ref["home_nbr_act"], np.array(bf["home_nbr_act"]).reshape(nh, 27), "home_nbr_act")
    eq(ref["act_nbr_home"], np.array(bf["act_nbr_home"]).reshape(-1, 27), "act_nbr_home")
    eq(ref["act_nbr_items"], np.array(bf["act_nbr_items"]).reshape(-1, 27), "act_nbr_items")
    # the wave groups tile every block's slots, 64 particles each but the last
    for h in range(nh):
        g = ref["groups"][h]
        size = (g[:, 1] - g[:, 0]) + (g[:, 3] - g[:, 2])
        assert np.all(size[:-1] == 64) and 0 < size[-1] <= 64
        assert np.array_equal(g[1:, 0], g[:-1, 1]) and np.array_equal(g[1:, 2], g[:-1, 3])
        assert tuple(g[0, [0, 2]]) == tuple(ref["home_range"][h, [0, 2]]) and tuple(g[-1, [1, 3]]) == tuple(ref["home_range"][h, [1, 3]])


def test_brute_force_cases_cover_what_they_claim():
    seen = dict(corner=False, edge=False, face=False, dropped=False, no_faces=False, no_verts=False, split=False,
                uneven=False, small=False, large=False, bits=set())
    for seed in range(36):
        pkey, n_f, n_v, prm = _random_case(seed)
        ref = rr.integer_layer(pkey, n_f, n_v, prm)
        nb = prm["nb"]
        onb = ((rr.block_coords(ref["home_block"]) == 0) | (rr.block_coords(ref["home_block"]) == nb - 1)).sum(axis=1)
        seen["corner"] |= bool((onb == 3).any())
        seen["edge"] |= bool((onb == 2).any())
        seen["face"] |= bool((onb == 1).any())
        seen["dropped"] |= bool((ref["seg_lo"] < 0).any())
        seen["no_faces"] |= ref["nfa_new"] == 0
        seen["no_verts"] |= ref["nva_new"] == 0
        seen["split"] |= bool((ref["home_items"][:, 1] > 1).any())
        seen["uneven"] |= bool(((ref["home_ngroups"] % np.maximum(ref["home_items"][:, 1], 1)) != 0).any())
        seen["small"] |= ref["ig"] < prm["item_groups"]
        seen["large"] |= ref["ig"] == prm["item_groups"]
        seen["bits"].add(prm["bits"])
    assert seen["bits"] == {4, 5, 6}
    assert all(v for k, v in seen.items() if k != "bits"), seen


def test_item_order_check_rejects_what_it_should():
    desc = np.array([(0, 0, 3, 0), (0, 3, 5, 0), (1, 0, 1, 0), (2, 0, 70, 0), (3, 0, 64, 0)], np.int64)
    rr.check_item_order([3, 4, 0, 1, 2], desc)
    rr.check_item_order([4, 3, 0, 1, 2], desc)      # (70 and 64 groups share the bucket of 63 and more)
    for bad in ([3, 4, 1, 0, 2], [3, 4, 0, 1, 1], [3, 4, 0, 1]):
        with pytest.raises(AssertionError):
            rr.check_item_order(bad, desc)


# ---- claims of the layouts ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rr.STATIC_NAMES)
@pytest.mark.parametrize("fast", (False, True))
def test_no_static_particle_is_ambiguous(name, fast):
    lay = rr.layout(name)
    bn = rr.layout_binning(lay, fem_fast=fast)
    assert not bn["ambiguous"].any(), (name, int(bn["ambiguous"].sum()), float(bn["dist"].min()))
    # the same blocks as the binning of transfer_layouts (its float64 restatement of the same kernel)
    if name in tl.NAMES and not fast:
        assert np.array_equal(bn["cell"] >> 2, tl.binning(lay)["block"])


def _static_reference(name, item_groups_small=None):
    lay = rr.layout(name)
    bn = rr.layout_binning(lay)
    prm = rr.layout_params(lay, item_groups_small)
    return lay, bn, prm, rr.integer_layer(bn["key"], lay["nf"], lay["nv"], prm)


@pytest.mark.parametrize("n_cells", (2, 8))
def test_interleaved_layouts_interleave(n_cells):
    lay = rr.layout(f"interleaved{n_cells}")
    nf, nv = lay["nf"], lay["nv"]
    # Finalize's sort: every particle alone in its cell -> the previous order is known; the vertices' is the id order
    prev = rr.finalize_order(lay)
    assert np.array_equal(prev[nf:], nf + np.arange(nv))
    # the uploaded state, in that order: inside one 64-slot window every cell comes in at least 8 separate runs
    key = rr.layout_binning(lay)["key"]
    for t, part in (("faces", key[prev[:nf]]), ("vertices", key[prev[nf:]])):
        assert len(part) >= 64
        win = part[:64]
        heads = np.flatnonzero(np.concatenate([[True], win[1:] != win[:-1]]))
        cells, runs = np.unique(win[heads], return_counts=True)
        assert len(cells) >= (2 if n_cells == 2 else 4) and runs.min() >= 8, (t, dict(zip(cells.tolist(), runs.tolist())))
    blocks = np.unique(key >> 6)
    assert len(np.unique(key[nf:])) == n_cells and len(blocks) == (1 if n_cells == 2 else 4)


def test_shrinking_sequence_moves_to_fewer_other_blocks():
    lay, second = rr.shrink_states()
    a = np.unique(rr.layout_binning(lay)["key"] >> 6)
    b = np.unique(rr.layout_binning(second)["key"] >> 6)
    assert len(b) < len(a) and len(a) >= 8 and not np.intersect1d(a, b).size
    assert not rr.layout_binning(lay)["ambiguous"].any() and not rr.layout_binning(second)["ambiguous"].any()
    # ... and not even the active lists overlap: every entry of the first re-sort's look-up tables has to go
    ra = rr.integer_layer(rr.layout_binning(lay)["key"], lay["nf"], lay["nv"], rr.layout_params(lay))
    rb = rr.integer_layer(rr.layout_binning(second)["key"], lay["nf"], lay["nv"], rr.layout_params(lay))
    assert not np.intersect1d(ra["act_block"], rb["act_block"]).size and len(rb["act_block"]) < len(ra["act_block"])


def test_heavy_layouts_split_into_items():
    for igs, least in ((16, 2), (4, 7), (1, 25)):
        _, _, _, ref = _static_reference("heavy", igs)
        assert ref["home_items"][:, 1].max() >= least, (igs, ref["home_items"])
        assert ref["ig"] == igs
    _, _, _, ref = _static_reference("heavy_items")
    assert ref["home_items"][:, 1].max() >= 7


def test_some_layout_splits_a_block_unevenly():
    hit = []
    for name, igs in (("heavy", 16), ("heavy", 4), ("dense", None)):
        _, _, _, ref = _static_reference(name, igs)
        ng, ni = ref["home_ngroups"], ref["home_items"][:, 1]
        if ((ni > 1) & (ng % ni != 0)).any():
            hit.append((name, igs))
    assert hit


def test_static_layouts_keep_every_particle_in_its_free_zone():
    """the finish checker's last assertion holds for the reference binning itself"""
    for name in rr.STATIC_NAMES:
        lay, bn, prm, ref = _static_reference(name)
        rel = bn["t"] - (4 * (bn["cell"] >> 2) - rr.FREE_ZONE)
        assert ((rel >= rr.GUARD) & (rel < rr.TOP)).all(), name


# ---- quiet time -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rr.STATIC_NAMES)
def test_quiet_time_bound_holds_for_float32(name):
    lay = rr.layout(name)
    bn = rr.layout_binning(lay)
    valid = np.ones(len(bn["key"]), bool)
    args = (bn["x"], bn["v"], bn["cell"], lay["bits"], tl.GRAVITY, lay["gravity_axis"], valid)
    ref = rr.quiet_time(*args)
    got = rr.quiet_time_f32(*args)
    assert ref[1] <= ref[0] <= ref[2] and ref[0] > 0
    r = rr.quiet_ratio(got, ref)
    assert r <= 1.0, (name, got, ref, r)
    # the bound is tight enough to say something: a few float32 ulps of the value
    assert np.isfinite(ref[0]) and ref[2] - ref[1] <= 1e-3 * ref[0], (name, ref)


def test_quiet_ratio_rejects_a_longer_time():
    lay = rr.layout("dense")
    bn = rr.layout_binning(lay)
    ref = rr.quiet_time(bn["x"], bn["v"], bn["cell"], lay["bits"], tl.GRAVITY, lay["gravity_axis"], np.ones(len(bn["key"]), bool))
    assert rr.quiet_ratio(ref[0] * 1.01, ref) > 1.0 and rr.quiet_ratio(ref[0] * 0.99, ref) > 1.0
    assert rr.quiet_ratio(float(np.float32(ref[0])), ref) <= 1.0


# ---- the radix sort's grid ------------------------------------------------------------------------------------------
def test_sort_grid_reaches_every_path_of_the_cost_model():
    plans = {(n, b): rr.sort_plan(n, b) for n in rr.SORT_N for b in rr.SORT_BITS}
    assert {p["digit_bits"] for p in plans.values()} == {8, 9, 10, 11}, "move the grid with the cost model"
    assert {p["passes"] for p in plans.values()} == {1, 2, 3, 4}
    assert {p["items"] for p in plans.values()} == {16, 64}
    assert {p["in_b"] for p in plans.values()} == {False, True}
    # the 9-bit template at the widths the issue names, at the contact solve's sizes
    assert all(rr.sort_plan(4097, b)["digit_bits"] == 9 for b in (9, 17, 25))
    # what runs at the sizes around 2^18: every digit width and both tile sizes stay covered by the reduced set
    assert rr.SORT_LARGE == min(n for n in rr.SORT_N if n > 4097) and set(rr.SORT_DISTS_LARGE) <= set(rr.SORT_DISTS)
    large = [plans[(n, b)] for n in rr.SORT_N if n >= rr.SORT_LARGE for b in rr.SORT_BITS]
    assert {p["items"] for p in large} == {16, 64} and len({p["tiles"] for p in large}) >= 3


@pytest.mark.parametrize("dist", rr.SORT_DISTS)
def test_sort_key_distributions(dist):
    for n, bits in ((65, 1), (4097, 9), (4097, 22), (2 ** 18 + 1, 31)):
        k = rr.sort_keys(dist, n, bits)
        assert k.dtype == np.uint32 and k.shape == (n,) and int(k.max()) < (1 << bits)
        pl = rr.sort_plan(n, bits)
        if dist == "top_digit" and pl["passes"] > 1:
            low = k & np.uint32((1 << ((pl["passes"] - 1) * pl["digit_bits"])) - 1)
            assert len(np.unique(low)) == 1 and len(np.unique(k)) > 1
        if dist == "one_tile" and pl["tiles"] > 2:
            tile = 64 * pl["items"]
            t = pl["tiles"] // 2
            assert len(np.unique(k[t * tile:(t + 1) * tile])) == 1 and len(np.unique(k[:tile])) > 1
