"""The conditional re-sort (drake_amd/csrc/mpm_rebuild.h: k_rb_count, k_rb_tables, k_rb_scatter, k_rb_canon,
k_rb_finish) restated in numpy, table by table, plus the layouts and sequences the table tests run.  CPU only: nothing
here imports the engine; the GPU tests hand over what they downloaded (drake_amd.capi.RT names, lower case).

Binning layer (floating point: the one place with a tolerance)
---------------------------------------------------------------
binning(...) restates k_rb_count's key in float64 from the float32 inputs: t = x dxinv - 1/2 per axis, the anticipatory
shift clamp(v anticip, -1.75, 1.75) cells, cell = clamp(floor(t + shift), 0, hi), key = cell_key(cell).  The WHOLE key
follows the shifted position (k_rb_count: "the cell part of the key follows the shifted position too"), so the
boundaries that can change a key are the integers 1 .. hi of the shifted t -- which contain the multiples of 4 that
change the block and the clamps at 0 and hi --, and the saturation of the shift at +-1.75 cells.  (The integers of the
unshifted t decide nothing in the key: a particle sitting exactly on one, as the `edges` layouts place them, is binned
by a shifted t well inside a cell.)  A particle closer than 2^(bits - 21) cells to such a boundary -- eight float32 ulps
of x dxinv at the far end of the grid -- is AMBIGUOUS: the kernel is compiled with contraction, a last-bit difference
from numpy is legitimate there, and either neighbouring cell is accepted on that axis (accepted_keys).  Everywhere else
the engine's pkey must equal the reference key.  A face is binned at the float32 centroid and mean velocity of its
corners, formed as k_fem forms them: (a + b + c) / 3, or (a + b + c) * (1/3) with fast math; in a partitioned domain
every particle is binned by its own position record, without a shift.

quiet_time(...) is Ctl::quiet_time of a single domain in float64: the minimum over the valid particles and the three
axes of the two time_to_travel values (to the top and to the bottom of the tile of the block the particle was binned
to, guard band included), with a rounding bound per candidate (u = 2^-24, K = 2 as in tests/transfer_layouts.py):
    t    = x dxinv - 1/2 - origin   one fused rounding at the magnitude of the absolute coordinate, one at t:
                                     e_t = u (|x dxinv - 1/2| + |t|), carried as an absolute error of t
    d    = top - t  or  t - guard   e_d = e_t + u |d|
    disc = v v + 2 a d              e_disc = 2 u (v v + |2 a d|) + 2 |a| e_d     (v dxinv, a dxinv: exact, powers of two)
    s    = sqrt(disc)  (hardware)   2^-23 relative, on the interval of disc
    den  = v + s                    u |den|, on the intervals of s
    T    = 2 d rcp(den) (hardware)  2^-23 + u relative, on the intervals of d and den
Each error times K widens its quantity to an interval, the intervals are carried through the formula (a candidate whose
branch d > 0, disc >= 0 or den > 0 can flip inside its interval takes 0 or infinity as that end), and the engine's
minimum must lie in [min_i lower_i, min_i upper_i].  The float32 restatement quiet_time_f32 stays inside on every
layout (tests/test_resort_reference.py), where the interval is also shown to be narrow: below 1e-3 of the value.

Integer layer (exact)
---------------------
integer_layer(pkey, nf_in, nv_in, prm) is a pure function of the engine's OWN pkey in previous-slot order, the listed
slots [0, nf_in) and [Nf, Nf + nv_in) and the engine's parameters; it returns every table k_rb_tables and k_rb_scatter
derive from the keys (see its docstring).  check_tables compares an engine's download with it, check_finish asserts
the state k_rb_finish must leave behind.
"""
import numpy as np

from tests import transfer_layouts as tl

SENTINEL = 0xFFFFFFFF
FREE_ZONE = 2
TILE_W = 10
GUARD = 0.125
TOP = (TILE_W - 2) - GUARD
SAT = 1.75
U32 = 2.0 ** -24
K = 2.0


# ---- Morton ids ------------------------------------------------------------------------------------------------------
def _compact3(v):
    """every third bit of v (inverse of tl._expand_bits)"""
    v = np.asarray(v, np.uint64) & np.uint64(0x49249249)
    v = (v | (v >> np.uint64(2))) & np.uint64(0xC30C30C3)
    v = (v | (v >> np.uint64(4))) & np.uint64(0x0F00F00F)
    v = (v | (v >> np.uint64(8))) & np.uint64(0xFF0000FF)
    v = (v | (v >> np.uint64(16))) & np.uint64(0x000003FF)
    return v.astype(np.int64)


def block_coords(b):
    """(n, 3) block coordinates of block ids (mpm_math.h: block_id = spread(x) 4 + spread(y) 2 + spread(z))"""
    b = np.asarray(b, np.uint64)
    return np.stack([_compact3(b >> np.uint64(2)), _compact3(b >> np.uint64(1)), _compact3(b)], -1)


def block_id(c):
    c = np.asarray(c, np.int64)
    return (tl.cell_key(4 * c[..., 0], 4 * c[..., 1], 4 * c[..., 2]) >> 6).astype(np.int64)


def key_cells(key):
    """(n, 3) cell coordinates of cell keys"""
    key = np.asarray(key, np.int64)
    lo = key & 63
    return 4 * block_coords(key >> 6) + np.stack([(lo >> 4) & 3, (lo >> 2) & 3, lo & 3], -1)


def neighbours(blocks, nb):
    """(n, 27) ids of the blocks around `blocks` in the order of off_index (x slowest), -1 outside the grid"""
    c = block_coords(blocks)
    o = np.arange(27)
    off = np.stack([o // 9 - 1, (o // 3) % 3 - 1, o % 3 - 1], -1)
    n = c[:, None, :] + off[None]
    ok = ((n >= 0) & (n < nb)).all(axis=-1)
    return np.where(ok, block_id(np.clip(n, 0, nb - 1)), -1)


# ---- binning layer -----------------------------------------------------------------------------------------------------
def binned_state(pos, vel, nf, corners=None, fem_fast=False):
    """float32 (x, v) every particle is binned by, in the order of pos / vel (faces first): a face's centroid and mean
    velocity of its corners (`corners`: (nf, 3) indices into pos / vel) as k_rb_count forms them, or -- corners None, a
    partitioned domain -- every particle's own position and no velocity"""
    pos, vel = tl.f32(pos).copy(), tl.f32(vel).copy()
    if corners is None:
        return pos, np.zeros_like(vel)
    c = np.asarray(corners)

    def mean3(a):
        s = (a[c[:, 0]] + a[c[:, 1]]) + a[c[:, 2]]
        return s * (np.float32(1) / np.float32(3)) if fem_fast else s / np.float32(3)
    x, v = pos.copy(), vel.copy()
    x[:nf], v[:nf] = mean3(pos), mean3(vel)
    return x, v


def binning(x32, v32, bits, anticip, valid=None):
    """-> dict(key (n,) int64 with SENTINEL where not valid, cell (n, 3), tp (n, 3) the shifted t, t (n, 3),
    dist (n,) cells to the nearest boundary that could change the key, ambiguous (n,) bool)"""
    dxinv = float(1 << bits)
    hi = (1 << bits) - 3
    x, v = np.asarray(x32, np.float64), np.asarray(v32, np.float64)
    t = x * dxinv - 0.5
    raw = v * float(anticip)
    tp = t + np.clip(raw, -SAT, SAT)
    cell = np.clip(np.floor(tp), 0, hi).astype(np.int64)
    key = tl.cell_key(cell[:, 0], cell[:, 1], cell[:, 2])
    near = np.clip(np.round(tp), 1, hi)                 # the nearest integer whose crossing changes floor's clamp
    dist = np.abs(tp - near)
    if anticip:
        dist = np.minimum(dist, np.abs(np.abs(raw) - SAT))
    dist = dist.min(axis=1)
    if valid is not None:
        key = np.where(valid, key, SENTINEL)
        dist = np.where(valid, dist, np.inf)
    thr = 2.0 ** (bits - 21)
    return dict(key=key, cell=cell, tp=tp, t=t, dist=dist, ambiguous=dist < thr, thr=thr)


def accepted_keys(bn, bits, engine_key):
    """per particle: True where the engine's key is the reference key, or -- ambiguous particles -- where each of its
    cell coordinates is one of floor(tp -+ thr) clamped"""
    hi = (1 << bits) - 3
    engine_key = np.asarray(engine_key, np.int64)
    ok = engine_key == bn["key"]
    amb = bn["ambiguous"] & (bn["key"] != SENTINEL) & (engine_key != SENTINEL)
    if amb.any():
        lo_c = np.clip(np.floor(bn["tp"][amb] - bn["thr"]), 0, hi).astype(np.int64)
        hi_c = np.clip(np.floor(bn["tp"][amb] + bn["thr"]), 0, hi).astype(np.int64)
        got = key_cells(engine_key[amb])
        ok[amb] = ((got == lo_c) | (got == hi_c)).all(axis=1)
    return ok


def _ttt64(d, v, a, e_d):
    """time_to_travel in float64 and the ends of the interval its float32 evaluation lies in (interval arithmetic with
    the errors of the module docstring, each times K) -> (T, lower end, upper end)"""
    with np.errstate(all="ignore"):
        disc = v * v + 2.0 * a * d
        den = v + np.sqrt(np.maximum(disc, 0.0))
        T = np.where(d > 0, np.where((disc >= 0) & (den > 0), 2.0 * d / den, np.inf), 0.0)
        d_lo, d_hi = d - K * e_d, d + K * e_d
        e_disc = K * (2.0 * U32 * (v * v + np.abs(2.0 * a * d)) + 2.0 * np.abs(a) * e_d)
        disc_lo, disc_hi = disc - e_disc, disc + e_disc
        s_lo = np.sqrt(np.maximum(disc_lo, 0.0)) * (1.0 - K * 2.0 ** -23)
        s_hi = np.sqrt(np.maximum(disc_hi, 0.0)) * (1.0 + K * 2.0 ** -23)
        den_lo = v + s_lo - K * U32 * np.abs(v + s_lo)
        den_hi = v + s_hi + K * U32 * np.abs(v + s_hi)
        rel = K * (2.0 ** -23 + U32)
        hi = np.where((disc_lo < 0) | (den_lo <= 0), np.inf, 2.0 * d_hi / den_lo * (1.0 + rel))
        lo = np.where((disc_hi < 0) | (den_hi <= 0), np.inf, 2.0 * d_lo / den_hi * (1.0 - rel))
        lo = np.where(d_lo <= 0, 0.0, lo)
        hi = np.where(d_hi <= 0, 0.0, hi)
    return T, lo, hi


def quiet_time(x32, v32, cells, bits, gravity, gravity_axis, valid):
    """-> (T, lower, upper): Ctl::quiet_time in float64 and the ends of the interval the engine's float32 minimum must
    lie in.  cells: (n, 3) the cell every particle was binned to (its block's tile is the frame)."""
    dxinv = float(1 << bits)
    x, vel = np.asarray(x32, np.float64), np.asarray(v32, np.float64)
    origin = (np.asarray(cells, np.int64) & ~3) - FREE_ZONE
    tabs = x * dxinv - 0.5
    t = tabs - origin
    e_t = U32 * (np.abs(tabs) + np.abs(t))
    v = vel * dxinv
    a = np.zeros(3)
    a[gravity_axis] = float(np.float32(gravity)) * dxinv
    a = np.broadcast_to(a, v.shape)
    up, dn = TOP - t, t - GUARD
    out = []
    for d, vv, aa in ((up, v, a), (dn, -v, -a)):
        out.append(_ttt64(d, vv, aa, e_t + U32 * np.abs(d)))
    sel = np.asarray(valid, bool)
    if not sel.any():
        return np.inf, np.inf, np.inf
    T = min(float(o[0][sel].min()) for o in out)
    lo = min(float(o[1][sel].min()) for o in out)
    hi = min(float(o[2][sel].min()) for o in out)
    return T, lo, hi


def quiet_time_f32(x32, v32, cells, bits, gravity, gravity_axis, valid):
    """k_rb_count's own float32 arithmetic in numpy (IEEE square root and division for the hardware's): the CPU check
    that the bound of quiet_time is a bound"""
    f = np.float32
    dxinv = f(1 << bits)
    x, vel = tl.f32(x32), tl.f32(v32)
    origin = ((np.asarray(cells, np.int64) & ~3) - FREE_ZONE).astype(np.float32)
    t = (x * dxinv - f(.5)) - origin
    v = vel * dxinv
    a = np.zeros(3, np.float32)
    a[gravity_axis] = f(gravity) * dxinv
    best = np.inf
    with np.errstate(all="ignore"):
        for d, vv, aa in ((f(TOP) - t, v, a), (t - f(GUARD), -v, -a)):
            disc = vv * vv + f(2) * aa * d
            den = vv + np.sqrt(disc)
            T = np.where(d > 0, np.where((disc >= 0) & (den > 0), f(2) * d / den, np.inf), 0.0)
            T = np.where(np.isnan(T), np.inf, T)
            best = min(best, float(T[np.asarray(valid, bool)].min()))
    return best


def quiet_ratio(got, ref):
    """how far the engine's quiet time is from the float64 value, in units of the allowed distance on that side"""
    T, lo, hi = ref
    if got == T:
        return 0.0
    if not np.isfinite(got) or not np.isfinite(T):
        return 0.0 if (got > T and hi == np.inf) or (got < T and lo <= got) else np.inf
    if got > T:
        return 0.0 if hi == np.inf else (got - T) / max(hi - T, 1e-300)
    return (T - got) / max(T - lo, 1e-300)


# ---- integer layer -----------------------------------------------------------------------------------------------------
def listed_slots(Nf, nf_in, nv_in):
    return np.concatenate([np.arange(nf_in), Nf + np.arange(nv_in)]).astype(np.int64)


def integer_layer(pkey, nf_in, nv_in, prm):
    """Everything the re-sort derives from the keys.  pkey: (Np,) the engine's keys by previous slot; listed slots
    [0, nf_in) (faces) and [Nf, Nf + nv_in) (vertices); prm: the engine's parameters (RT.PARAMS).  Returns
        home_block (nh,) ascending; blkcnt, blkstart (nh, 2) per type; home_range (nh, 4); nfa_new, nva_new
        cell_prefix (nh, 2, 64) exclusive prefixes of the (type, cell) counts inside every home block
        slots (m,) the listed slots, seg_lo / seg_hi (m,) the (type, cell) segment each one lands in (-1: dropped),
        dst (m,) its destination when every segment keeps the previous order (deterministic mode), -1: dropped
        home_ngroups (nh,), group_offset (nh,) pool offsets, groups: list of (ng, 4) arrays per home block
        ig, home_items (nh, 2), item_desc (n_items, 4), n_items
        act_block (na,) ascending; lut_home, lut_act (nblocks,) with -1 at every other block
        home_nbr_act (nh, 27), act_nbr_home (na, 27), act_nbr_items (na, 27)"""
    Nf, nb, nblocks = prm["Nf"], prm["nb"], prm["nblocks"]
    pkey = np.asarray(pkey, np.int64)
    slots = listed_slots(Nf, nf_in, nv_in)
    typ = (slots >= Nf).astype(np.int64)
    key = pkey[slots]
    live = key != SENTINEL
    blk = key >> 6
    home_block = np.unique(blk[live])
    nh = len(home_block)
    hidx = np.searchsorted(home_block, np.where(live, blk, home_block[0] if nh else 0))
    blkcnt = np.zeros((nh, 2), np.int64)
    np.add.at(blkcnt, (hidx[live], typ[live]), 1)
    blkstart = np.cumsum(blkcnt, axis=0) - blkcnt
    nfa_new, nva_new = int(blkcnt[:, 0].sum()), int(blkcnt[:, 1].sum())
    home_range = np.stack([blkstart[:, 0], blkstart[:, 0] + blkcnt[:, 0], Nf + blkstart[:, 1],
                           Nf + blkstart[:, 1] + blkcnt[:, 1]], -1)
    cellcnt = np.zeros((nh, 2, 64), np.int64)
    np.add.at(cellcnt, (hidx[live], typ[live], key[live] & 63), 1)
    cell_prefix = np.cumsum(cellcnt, axis=2) - cellcnt
    seg_lo = np.full(len(slots), -1, np.int64)
    seg_lo[live] = (typ[live] * Nf + blkstart[hidx[live], typ[live]] + cell_prefix[hidx[live], typ[live], key[live] & 63])
    seg_hi = np.full(len(slots), -1, np.int64)
    seg_hi[live] = seg_lo[live] + cellcnt[hidx[live], typ[live], key[live] & 63]
    # deterministic order: the stable sort of the previous order by (type, block, cell) = by (type, key)
    dst = np.full(len(slots), -1, np.int64)
    li = np.flatnonzero(live)
    order = li[np.lexsort((slots[li], key[li], typ[li]))]
    rank_in_type = np.concatenate([np.arange(nfa_new), np.arange(nva_new)])
    dst[order] = typ[order] * Nf + rank_in_type
    # wave groups: windows of 64 of the merged sequence cell 0 faces, cell 0 vertices, cell 1 faces, ...
    total = blkcnt.sum(axis=1)
    home_ngroups = (total + 63) >> 6
    group_offset = ((home_range[:, 0] + (home_range[:, 2] - Nf)) >> 6) + np.arange(nh)
    groups = []
    for h in range(nh):
        is_vert = np.repeat(np.tile([0, 1], 64), cellcnt[h].T.reshape(-1))    # merged order: per cell faces, vertices
        faces_before = np.concatenate([[0], np.cumsum(1 - is_vert)])
        m0 = np.minimum(64 * np.arange(home_ngroups[h]), total[h])
        m1 = np.minimum(m0 + 64, total[h])
        f0, f1 = faces_before[m0], faces_before[m1]
        groups.append(np.stack([home_range[h, 0] + f0, home_range[h, 0] + f1, home_range[h, 2] + (m0 - f0),
                                home_range[h, 2] + (m1 - f1)], -1))
    # work items
    held = nfa_new + nva_new
    ig = min(prm["item_groups"], prm["item_groups_small"]) if ((held + 63) >> 6) < prm["item_small_below"] \
        else prm["item_groups"]
    n_of = (home_ngroups + ig - 1) // ig
    first = np.cumsum(n_of) - n_of
    home_items = np.stack([first, n_of], -1)
    desc = []
    for h in range(nh):
        ng, ni = int(home_ngroups[h]), int(n_of[h])
        for k in range(ni):
            desc.append((h, k * ng // ni, (k + 1) * ng // ni, 0))
    item_desc = np.array(desc, np.int64).reshape(-1, 4)
    # active list and the look-up tables
    nbr_h = neighbours(home_block, nb)
    act_block = np.unique(nbr_h[nbr_h >= 0])
    lut_home = np.full(nblocks, -1, np.int64)
    lut_home[home_block] = np.arange(nh)
    lut_act = np.full(nblocks, -1, np.int64)
    lut_act[act_block] = np.arange(len(act_block))
    home_nbr_act = np.where(nbr_h >= 0, lut_act[np.maximum(nbr_h, 0)], -1)
    nbr_a = neighbours(act_block, nb)
    act_nbr_home = np.where(nbr_a >= 0, lut_home[np.maximum(nbr_a, 0)], -1)
    hn = np.maximum(act_nbr_home, 0)
    act_nbr_items = np.where(act_nbr_home >= 0, home_items[hn, 0] | (np.minimum(home_items[hn, 1], 127) << 24), -1) \
        if nh else np.full_like(act_nbr_home, -1)
    return dict(home_block=home_block, blkcnt=blkcnt, blkstart=blkstart, home_range=home_range, nfa_new=nfa_new,
                nva_new=nva_new, cell_prefix=cell_prefix, cellcnt=cellcnt, slots=slots, seg_lo=seg_lo, seg_hi=seg_hi,
                dst=dst, home_ngroups=home_ngroups, group_offset=group_offset, groups=groups, ig=ig,
                home_items=home_items, item_desc=item_desc, n_items=len(item_desc), act_block=act_block,
                lut_home=lut_home, lut_act=lut_act, home_nbr_act=home_nbr_act, act_nbr_home=act_nbr_home,
                act_nbr_items=act_nbr_items)


def check_item_order(item_order, item_desc):
    """item_order is a permutation of the items whose group counts, capped at 63, never increase"""
    item_order = np.asarray(item_order, np.int64)
    n = len(item_desc)
    assert len(item_order) == n, ("item_order: length", len(item_order), n)
    assert np.array_equal(np.sort(item_order), np.arange(n)), "item_order is not a permutation of the items"
    cnt = np.minimum(item_desc[item_order, 2] - item_desc[item_order, 1], 63)
    bad = np.flatnonzero(np.diff(cnt) > 0)
    assert bad.size == 0, (f"item_order: not heaviest first at position {bad[:1]}: groups "
                           f"{cnt[bad[:1]]} before {cnt[bad[:1] + 1]}")


def derived_item_tables(ref, item_order, prm):
    """item_pos, item_flat (n, 8), item_rng (n, 4) that follow from the engine's own item_order"""
    item_order = np.asarray(item_order, np.int64)
    n = ref["n_items"]
    pos = np.empty(n, np.int64)
    pos[item_order] = np.arange(n)
    d = ref["item_desc"][item_order]
    h = d[:, 0]
    rg = ref["home_range"][h]
    flat = np.stack([item_order, h, ref["home_block"][h], d[:, 2] - d[:, 1], rg[:, 0], rg[:, 1], rg[:, 2],
                     ref["group_offset"][h] + d[:, 1]], -1)
    rng = np.array([(ref["groups"][hh][g0, 0], ref["groups"][hh][g1 - 1, 1], ref["groups"][hh][g0, 2],
                     ref["groups"][hh][g1 - 1, 3]) for hh, g0, g1 in d[:, :3]], np.int64).reshape(-1, 4)
    return pos, flat, rng


def _same(name, got, want, where=""):
    got, want = np.asarray(got, np.int64), np.asarray(want, np.int64)
    assert got.shape == want.shape, f"{name}{where}: shape {got.shape}, reference {want.shape}"
    bad = np.argwhere(got != want)
    assert bad.size == 0, (f"{name}{where}: {len(bad)} entries differ from the reference, first at {tuple(bad[0])}: "
                           f"{got[tuple(bad[0])]} instead of {want[tuple(bad[0])]}")


def check_tables(T, ref, prm, deterministic, where=""):
    """every table of the download T (dict of RT tables, lower-case names; ctl and params as dicts) against the integer
    layer's `ref`; an AssertionError names the table"""
    ctl = T["ctl"]
    assert ctl["error"] == 0, f"error flags {ctl['error']}{where}"
    nh, na, ni = len(ref["home_block"]), len(ref["act_block"]), ref["n_items"]
    assert (ctl["n_home"], ctl["n_active"], ctl["n_items"], ctl["n_items_wanted"]) == (nh, na, ni, ni), \
        f"n_home / n_active / n_items / n_items_wanted{where}: {ctl}, reference {(nh, na, ni)}"
    assert ni <= prm["capS"] and nh <= prm["capH"] and na <= prm["capA"]
    _same("home_block", T["home_block"], ref["home_block"], where)
    _same("home_range", T["home_range"], ref["home_range"], where)
    hb = ref["home_block"]
    _same("blkstart[0] at the home blocks", T["blkstart0"][hb], ref["blkstart"][:, 0], where)
    _same("blkstart[1] at the home blocks", T["blkstart1"][hb], ref["blkstart"][:, 1], where)
    _same("lut_home", T["lut_home"], ref["lut_home"], where)
    _same("act_block", T["act_block"], ref["act_block"], where)
    _same("lut_act", T["lut_act"], ref["lut_act"], where)
    _same("home_nbr_act", T["home_nbr_act"], ref["home_nbr_act"], where)
    _same("act_nbr_home", T["act_nbr_home"], ref["act_nbr_home"], where)
    _same("act_nbr_items", T["act_nbr_items"], ref["act_nbr_items"], where)
    _same("home_ngroups", T["home_ngroups"], ref["home_ngroups"], where)
    for h in range(nh):
        o = int(ref["group_offset"][h])
        _same(f"home_groups of home block {h}", T["home_groups"][o:o + int(ref["home_ngroups"][h])], ref["groups"][h], where)
    _same("home_items", T["home_items"], ref["home_items"], where)
    _same("item_desc", T["item_desc"], ref["item_desc"], where)
    check_item_order(T["item_order"], ref["item_desc"])
    pos, flat, rng = derived_item_tables(ref, T["item_order"], prm)
    _same("item_pos", T["item_pos"], pos, where)
    _same("item_flat", T["item_flat"], flat, where)
    _same("item_rng", T["item_rng"], rng, where)
    # the permutation
    slots, live = ref["slots"], ref["seg_lo"] >= 0
    dst = np.asarray(T["dst_of"], np.int64)[slots]
    _same("dst_of of the dropped particles", dst[~live], np.full(int((~live).sum()), -1), where)
    if deterministic:
        _same("dst_of (canonical order)", dst, ref["dst"], where)
    inside = (dst[live] >= ref["seg_lo"][live]) & (dst[live] < ref["seg_hi"][live])
    assert inside.all(), (f"dst_of{where}: {int((~inside).sum())} particles outside their (type, cell) segment, first "
                          f"previous slot {slots[live][~inside][0]}")
    assert len(np.unique(dst[live])) == int(live.sum()), f"dst_of{where}: two particles share a destination"


def check_finish(T, ref, prm, before, where="", quiet_is_zero=False, old_pid=None, corner_ids=None, dist=False,
                 pos_by_prev_slot=None):
    """the state after k_rb_finish.  before: the control block before the re-sort; old_pid: PID before it;
    corner_ids: (scene faces, 3) original ids of every face's corners (ARR.INDICES); pos_by_prev_slot: (Np, 3) float64
    position every particle was binned at, by previous slot"""
    ctl = T["ctl"]
    Nf = prm["Nf"]
    for name in ("blkcnt0", "blkcnt1", "cellcnt0", "cellcnt1", "home_bits"):
        nz = np.flatnonzero(T[name])
        assert nz.size == 0, f"{name}{where}: {nz.size} entries not cleared by k_rb_finish, first at {nz[0]} = {T[name][nz[0]]}"
    tk = np.asarray(T["tickets"]).reshape(32, 32)
    assert not tk[:, 0].any() and not tk[:, 1].any() and ctl["ticket"] == 0, f"tickets{where}: {tk[:, :2].T}, {ctl['ticket']}"
    assert ctl["need_rebuild"] == 0, f"need_rebuild{where}"
    assert ctl["rebuilds"] == before["rebuilds"] + 1, f"rebuilds{where}: {before['rebuilds']} -> {ctl['rebuilds']}"
    assert (ctl["nfa"], ctl["nva"]) == (ref["nfa_new"], ref["nva_new"]), f"nfa / nva{where}: {ctl}, reference {ref['nfa_new'], ref['nva_new']}"
    assert ctl["add_f"] == 0 and ctl["add_v"] == 0, f"add_f / add_v{where}"
    assert ctl["cur"] == before["cur"] ^ 1, f"cur{where}"
    if quiet_is_zero:
        assert ctl["quiet_time"] == 0.0, f"quiet_time{where}: {ctl['quiet_time']}"
    slots, live = ref["slots"], ref["seg_lo"] >= 0
    dst = np.asarray(T["dst_of"], np.int64)
    src = np.asarray(T["src_of"], np.int64)
    active = listed_slots(Nf, ctl["nfa"], ctl["nva"])
    assert np.array_equal(src[dst[slots[live]]], slots[live]), f"src_of[dst_of]{where} is not the identity on the listed slots"
    assert np.array_equal(dst[src[active]], active), f"dst_of[src_of]{where} is not the identity on the active slots"
    pid, imap = np.asarray(T["pid"], np.int64), np.asarray(T["imap"], np.int64)
    assert np.array_equal(imap[pid[active]], active), f"imap[pid[s]] != s{where}"
    if old_pid is not None:
        old_pid = np.asarray(old_pid, np.int64)
        assert np.array_equal(pid[active], old_pid[src[active]]), f"pid{where} is not the old one gathered through src_of"
        gone = old_pid[slots[~live]]
        assert np.all(imap[gone] == -1), f"imap{where} of the dropped particles"
    if corner_ids is not None:
        refs = np.asarray(T["face_refs"], np.int64)[:ctl["nfa"], 1:]
        want_ids = np.asarray(corner_ids, np.int64)[pid[:ctl["nfa"]]]
        if dist:
            _same("face corner references (imap of the corner ids)", refs, imap[want_ids], where)
        else:
            assert (refs >= Nf).all() and (refs < Nf + ctl["nva"]).all(), f"face corner references{where} outside the vertex slots"
            _same("ids at the face corner references", pid[refs], want_ids, where)
    if pos_by_prev_slot is not None:
        dxinv = float(1 << prm["bits"])
        home_of = np.full(prm["Np"], -1, np.int64)
        for h, rg in enumerate(ref["home_range"]):
            home_of[rg[0]:rg[1]] = h
            home_of[rg[2]:rg[3]] = h
        assert (home_of[active] >= 0).all(), f"home_range{where} does not cover the active slots"
        t = np.asarray(pos_by_prev_slot, np.float64)[src[active]] * dxinv - 0.5
        rel = t - (4 * block_coords(ref["home_block"][home_of[active]]) - FREE_ZONE)
        bad = np.flatnonzero(~((rel >= GUARD) & (rel < TOP)).all(axis=1))
        assert bad.size == 0, (f"binning{where}: {bad.size} particles outside the free zone of their home block, first "
                               f"slot {active[bad[0]]} at {rel[bad[0]]} cells of its tile")


# ---- layouts and sequences of the table tests ------------------------------------------------------------------------
def _layout(name, bits, rest, idx, pos_v, vel_v=None, gravity_axis=2, env=None):
    """a layout dict in the form of transfer_layouts (one cloth): rest vertices (nv, 3) in cell units u = x dxinv,
    triangles idx (nt, 3), the vertex state to upload (cell units; m/s), faces at the float32 centroids"""
    dx = 1.0 / (1 << bits)
    rest, pos_v = np.asarray(rest, np.float64) * dx, np.asarray(pos_v, np.float64) * dx
    idx = np.asarray(idx, np.int32).reshape(-1, 3)
    nf, nv = len(idx), len(rest)
    vel_v = np.zeros((nv, 3)) if vel_v is None else np.asarray(vel_v, np.float64)
    xv, vv = tl.f32(pos_v), tl.f32(vel_v)
    cen = ((xv[idx[:, 0]] + xv[idx[:, 1]]) + xv[idx[:, 2]]) / np.float32(3)
    cvel = ((vv[idx[:, 0]] + vv[idx[:, 1]]) + vv[idx[:, 2]]) / np.float32(3)
    n = nf + nv
    return dict(name=name, bits=bits, gravity_axis=gravity_axis, cloths=[(tl.f32(rest), np.zeros((nv, 3), np.float32), idx)],
                densities=None, nf=nf, nv=nv, idx_all=idx, pos=np.concatenate([cen, xv]), vel=np.concatenate([cvel, vv]),
                C=np.zeros((n, 9), np.float32), vol=np.full(n, 1e-8, np.float32), env=dict(env or {}),
                anticipate=tl.ANTICIPATE, claims={})


def interleaved(n_cells, seed=11):
    """A previous order that alternates slot by slot between n_cells cells (2: two cells of one block; 8: two cells in
    each of four blocks).  The rest state puts vertex k alone into the cell with the k-th key of a run of consecutive
    keys, so Finalize's own sort leaves the vertices in id order whatever the arrival order of its atomics; the faces'
    centroids fall into cells of their own too, so their order is as predictable (finalize_order).  The uploaded state
    puts vertex k into cell k mod n_cells, and with it face f (corners 3 f, 3 f + 1, 3 f + 2) into a cell that depends on
    f mod n_cells only."""
    rng = np.random.default_rng(seed)
    bits = 6
    nt = 72
    key0 = int(tl.cell_key(16, 16, 16))                      # an aligned 8^3 region: 512 consecutive keys
    cells = tl.key_coords(bits)[key0:key0 + 3 * nt]
    rest = cells + 1.0 + rng.uniform(-0.1, 0.1, cells.shape)   # u = t + 1/2: the cell's centre, within 0.1 cells
    idx = np.arange(3 * nt).reshape(nt, 3)
    B = np.array([9, 9, 9])
    if n_cells == 2:
        target = np.array([4 * B + [1, 1, 1], 4 * B + [1, 1, 2]])
    else:
        target = np.array([4 * (B + o) + c for o in ([0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1])
                           for c in ([1, 1, 1], [2, 2, 2])])
    pos = target[np.arange(3 * nt) % n_cells] + 1.0 + rng.uniform(-0.1, 0.1, (3 * nt, 3))
    return _layout(f"interleaved{n_cells}", bits, rest, idx, pos)


def finalize_order(lay):
    """original ids by slot after Finalize's sort of the rest state, where that is the same on every run: every
    particle alone in its (type, cell) segment (asserted)"""
    nf, nv = lay["nf"], lay["nv"]
    rest = lay["cloths"][0][0]
    x0, v0 = binned_state(np.concatenate([np.zeros((nf, 3), np.float32), rest]), np.zeros((nf + nv, 3)), nf,
                          corners=nf + lay["idx_all"])
    first = binning(x0, v0, lay["bits"], 0.0)
    assert not first["ambiguous"].any()
    kf, kv = first["key"][:nf], first["key"][nf:]
    assert len(np.unique(kf)) == nf and len(np.unique(kv)) == nv
    return np.concatenate([np.argsort(kf, kind="stable"), nf + np.argsort(kv, kind="stable")])


def shrink_states(seed=12):
    """(layout, second state): 60 small triangles spread over the blocks [3, 7)^3, then all of them inside two blocks
    far away -- fewer home blocks, none shared.  The second state is (pos, vel) in original order."""
    rng = np.random.default_rng(seed)
    bits = 6
    M = tl._Mesh(bits, seed)
    for _ in range(60):
        M.small(4 * rng.uniform(3.2, 6.8, 3), 0.3)
    first = np.concatenate(M.verts)
    idx = np.arange(len(first)).reshape(-1, 3)
    M2 = tl._Mesh(bits, seed + 1)
    for k in range(60):
        M2.small(4 * np.array([11, 11, 11 + k % 2]) + rng.uniform(1.0, 3.0, 3) + 0.5, 0.3)
    lay = _layout("shrink", bits, first, idx, first, vel_v=rng.uniform(-0.05, 0.05, first.shape))
    second = _layout("shrink2", bits, first, idx, np.concatenate(M2.verts), vel_v=rng.uniform(-0.05, 0.05, first.shape))
    return lay, second


EXTRA = {"interleaved2": lambda: interleaved(2), "interleaved8": lambda: interleaved(8)}
STATIC_NAMES = tl.NAMES + tuple(EXTRA)
_CACHE = {}


def layout(name):
    if name in tl.BUILDERS:
        return tl.layout(name)
    if name not in _CACHE:
        _CACHE[name] = EXTRA[name]()
    return _CACHE[name]


def layout_binning(lay, fem_fast=False):
    """the binning layer on a layout's uploaded state, in original order (faces first)"""
    nf = lay["nf"]
    x, v = binned_state(lay["pos"], lay["vel"], nf, corners=nf + lay["idx_all"], fem_fast=fem_fast)
    anticip = np.float32(np.float32(lay["anticipate"]) * np.float32(tl.DT)) * np.float32(1 << lay["bits"])
    bn = binning(x, v, lay["bits"], float(anticip))
    bn["x"], bn["v"] = x, v
    return bn


def layout_params(lay, item_groups_small=None):
    """the parameters a default engine has on this layout (mpm_engine.hip: mpm_finalize)"""
    n = lay["nf"] + lay["nv"]
    bits = lay["bits"]
    nb = 1 << (bits - 2)
    igs = int(item_groups_small or lay["env"].get("MPM_ITEM_GROUPS_SMALL", tl.ITEM_GROUPS_SMALL))
    return dict(Nf=lay["nf"], Np=n, bits=bits, nb=nb, nblocks=nb ** 3, item_groups=48, item_groups_small=igs,
                item_small_below=6500)


# ---- the radix sort's cost model (mpm_sort.h: sort_plan) ---------------------------------------------------------------
SORT_N = (2, 65, 1025, 4097, 2 ** 18 - 1, 2 ** 18, 2 ** 18 + 1, 2 ** 18 + 4097)
SORT_BITS = (1, 8, 9, 16, 17, 19, 22, 25, 28, 31)
SORT_DISTS = ("equal", "two", "uniform", "ascending", "descending", "top_digit", "one_tile")
# the distributions run at the sizes around 2^18 (the file stays within seconds)
SORT_DISTS_LARGE = ("uniform", "top_digit", "one_tile")
SORT_LARGE = 2 ** 18 - 1


def sort_plan(n, bits):
    """Python copy of sort_plan (mpm_sort.h) -> dict(items, tiles, digit_bits, passes, in_b)"""
    items = 64 if n > (1 << 18) else 16
    tiles = (n + 64 * items - 1) // (64 * items)
    best, db, passes = 1e30, 8, (bits + 7) // 8
    for d in range(8, 12):
        ps = (bits + d - 1) // d
        cost = ps * (11.0 + ((1 << d) * tiles * 4) / 65536.0)
        if cost < best:
            best, db, passes = cost, d, ps
    return dict(items=items, tiles=tiles, digit_bits=db, passes=passes, in_b=passes % 2 == 1)


def sort_keys(dist, n, bits, seed=0):
    """keys of one distribution, masked to `bits`"""
    rng = np.random.default_rng([seed, n, bits, SORT_DISTS.index(dist)])
    mask = (1 << bits) - 1
    pl = sort_plan(n, bits)
    top_shift = (pl["passes"] - 1) * pl["digit_bits"]
    if dist == "equal":
        k = np.full(n, 0x5A5A5A5A & mask, np.uint64)
    elif dist == "two":
        k = np.where(rng.integers(0, 2, n) == 1, mask, 0x12345678 & mask).astype(np.uint64)
    elif dist == "uniform":
        k = rng.integers(0, mask + 1, n, dtype=np.uint64)
    elif dist == "ascending":
        k = (np.arange(n, dtype=np.uint64) * np.uint64(mask + 1)) // np.uint64(n)
    elif dist == "descending":
        k = np.uint64(mask) - (np.arange(n, dtype=np.uint64) * np.uint64(mask + 1)) // np.uint64(n)
    elif dist == "top_digit":     # equal low digits, only the top digit differs
        low = 0x2B3C4D5E & ((1 << top_shift) - 1)
        k = (rng.integers(0, (mask >> top_shift) + 1, n, dtype=np.uint64) << np.uint64(top_shift)) | np.uint64(low)
    elif dist == "one_tile":      # one tile (the middle one) holds a single key, the others are uniform
        k = rng.integers(0, mask + 1, n, dtype=np.uint64)
        tile = 64 * pl["items"]
        t = pl["tiles"] // 2
        k[t * tile:(t + 1) * tile] = np.uint64(0x0F1E2D3C & mask)
    else:
        raise KeyError(dist)
    return (k & np.uint64(mask)).astype(np.uint32)
