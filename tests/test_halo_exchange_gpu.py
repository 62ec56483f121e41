"""The exchange of raw node sums across a cut, kernel by kernel and in every variant, on the layouts of
tests/halo_layouts.py against its float32 restatements.  All engines are deterministic; every comparison of parts a - e,
g and h is bit for bit, over every block, node and particle:

    a  k_halo_pack2 (mpm_halo_pack)                      ids, count, sums, the words behind the count
    b  the pack folded into k_grid<0> (substep_begin_halo), one and two zones, three substeps through the same buffers
    c  k_halo_add2 (mpm_halo_add) on a host-written buffer in shuffled order with ids the receiver does not have
    d  the add folded into k_grid<2> (substep_end_halo, n == zones) against add + update + GridToParticle, a block's
       entry at scan positions 0, 63, 64, 127, 128 and last; one buffer for two zones (the k_halo_add2 route)
    e  the split update (begin / mid / end) against begin / end, and the state between mid and end
    f  two ranks exchanging through device copies against the engine that holds both particle sets: identical sums and
       velocities on both ranks, and the rounding bounds of halo_layouts / transfer_layouts against the union
    g  a buffer one block too small: MPM_ERR_CAPACITY, the entries that fit are valid, nothing behind the buffer is written
    h  the direct transport between two engines of one process against f's device copies"""
import numpy as np
import pytest

from tests import halo_layouts as hl
from tests import harness as hs
from tests import transfer_layouts as tl

pytestmark = pytest.mark.gpu

DT = tl.DT
CAP = 512                      # blocks: more than any buffer of these tests holds (two zones in one: < 400)
TAIL = 256                     # words behind a buffer that must stay as they were
ONE_ZONE = [(hl.ZLO, hl.ZHI, 0)]
TWO_ZONES = [(hl.ZLO - hl.PITCH, hl.ZHI - hl.PITCH, +hl.PITCH), (hl.ZLO, hl.ZHI, -hl.PITCH)]
ERR_CAPACITY_BIT = 2           # mpm_device.h: ERR_CAPACITY
MPM_ERR_CAPACITY = -4          # include/mpm_hip.h
_CACHE = {}


# ---- plumbing ------------------------------------------------------------------------------------------------------------
def _engine(lay):
    from tests.test_transfer_layouts_gpu import _engine as make
    return make(lay, "deterministic")


def _dev(host_words):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(host_words, np.uint32).view(np.int32).copy()).to("cuda")
    torch.cuda.synchronize()
    return t


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint32)


def _fresh(cap=CAP):
    return _dev(np.full(hl.buffer_bytes(cap) // 4 + TAIL, hl.FILL, np.uint32))


def _tables(g):
    act = g.resort_table("ACT_BLOCK").astype(np.int64)
    lut = g.resort_table("LUT_ACT").astype(np.int64)
    want = np.full(hl.NBLOCKS, -1, np.int64)
    want[act] = np.arange(len(act))
    assert np.array_equal(lut, want), "LUT_ACT is not the inverse of ACT_BLOCK"
    return act


def _raw(g):
    from drake_amd import ARR as A
    return hl.raw_dense(g.download(A.GRID_MASSES), g.download(A.GRID_MOMENTUM))


def _grid(g):
    from drake_amd import ARR as A
    return dict(gm=g.download(A.GRID_MASSES), gv=g.download(A.GRID_MOMENTUM).reshape(-1, 3),
                gvs=g.download(A.GRID_V_STAR).reshape(-1, 3))


def _particles(g):
    from drake_amd import ARR as A
    return {k: g.download(a) for k, a in (("pids", A.PIDS), ("x", A.POSITIONS), ("v", A.VELOCITIES), ("C", A.AFFINE),
                                          ("F", A.DEFORMATION_GRADIENTS))}


def _same_words(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.dtype.kind == "f":
        got, want = hl.words(got), hl.words(want)
    bad = np.flatnonzero((got != want).reshape(len(got), -1).any(axis=1))
    assert bad.size == 0, f"{what}: {bad.size} rows differ, first {bad[0]}: {np.asarray(got)[bad[0]]} vs {np.asarray(want)[bad[0]]}"


def _same_state(a, b, what):
    for k in ("pids", "x", "v", "C", "F"):
        _same_words(a[k], b[k], f"{what}: particles {k}")


def _same_grid(a, b, what):
    for k in ("gm", "gv", "gvs"):
        _same_words(a[k], b[k], f"{what}: grid {k}")


def _grid_is(grid, raw_after, what):
    m, gv, gvs = hl.update_ref(raw_after)
    _same_words(grid["gm"], m, f"{what}: GRID_MASSES against the restatement")
    _same_words(grid["gvs"], gvs, f"{what}: GRID_V_STAR against the restatement")
    _same_words(grid["gv"], gv, f"{what}: GRID_MOMENTUM against the restatement")


def _ok(g):
    g.gpu_sync()
    assert g.stats()["error_flags"] == 0, g.stats()


def _gather(g):
    """the phase calls up to the raw sums"""
    g.rebuild_mapping(False)
    g.calc_fem_state_and_force(DT)
    g.particle_to_grid(DT)
    g.grid_gather()


def _begin(g, zones, bufs, cap=CAP):
    g.substep_begin_halo(DT, g.halo_zone_args(zones, [b.data_ptr() for b in bufs]), cap)


def _end(g, recv, cap=CAP):
    g.substep_end_halo(DT, -1, g.halo_buffer_args([b.data_ptr() for b in recv]), cap)


def _check_pack(buf_words, cap, act, raw, zone, what, behind=None):
    """the buffer holds exactly pack_ref's entries, each once, bit for bit; behind the count everything is as it was
    (`behind`: the buffer's words before the pack, default the fill pattern); -> the count word"""
    n, ids, data, tail = hl.read_buffer(buf_words, cap)
    ref = hl.pack_ref(act, raw, *zone)
    assert n == len(ref), (what, n, len(ref))
    got = ids[:n].tolist()
    assert len(set(got)) == n and set(got) == set(ref), (what, sorted(set(got) ^ set(ref))[:8])
    for k, bid in enumerate(got):
        assert np.array_equal(data[k], hl.words(ref[bid])), f"{what}: the sums of entry {k} (block {bid}) differ"
    if behind is None:
        assert (ids[n:] == hl.FILL).all() and (data[n:] == hl.FILL).all(), f"{what}: written behind the count"
    else:
        _, ids0, data0, _ = hl.read_buffer(behind, cap)
        assert np.array_equal(ids[n:], ids0[n:]) and np.array_equal(data[n:], data0[n:]), f"{what}: written behind the count"
    assert (tail == hl.FILL).all(), f"{what}: written behind the buffer"
    return n


def _gathered(name, which, pitch=0):
    """(active blocks, raw sums) of one side after the phase calls, cached: what the other side receives from it"""
    key = ("gathered", name, which, pitch)
    if key not in _CACHE:
        g = _engine(hl.side(name, which, pitch))
        _gather(g)
        _ok(g)
        _CACHE[key] = (_tables(g), _raw(g))
        g.destroy()
    return _CACHE[key]


def _other(which):
    return "right" if which == "left" else "left"


def _strangers(act, zone, k=3):
    """k entries of zone blocks that are not active here, with sums that would show"""
    lo, hi = zone
    have = set(act.tolist())
    out = []
    for bx in range(lo, hi + 1):
        for byz in ((5, 13), (12, 2)):
            bid = int(hl.block_id(bx, *byz))
            if bid not in have and len(out) < k:
                out.append((bid, np.full((64, 4), 1.0 + bx, np.float32)))
    assert len(out) == k
    return out


def _received(name, which, zones, act):
    """per zone of the receiver `which` the entries the other side's sums make (its zone blocks relabelled into this
    zone), plus blocks the receiver does not have"""
    oact, oraw = _gathered(name, _other(which))
    out = []
    for lo, hi, _ in zones:
        ent = list(hl.pack_ref(oact, oraw, hl.ZLO, hl.ZHI, lo - hl.ZLO).items())
        out.append(ent + _strangers(act, (lo, hi)))
    return out


def _shuffled(entries, seed):
    order = np.random.default_rng(seed).permutation(len(entries))
    return [entries[i] for i in order]


SIDES = [(n, w) for n in hl.NAMES for w in ("left", "right")]


# ---- a. the pack kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,which", SIDES)
def test_pack(name, which):
    lay = hl.side(name, which)
    g = _engine(lay)
    _gather(g)
    _ok(g)
    act, raw = _tables(g), _raw(g)
    # the layout's claims hold on the engine: its active blocks are the restated ones
    assert np.array_equal(act, hl.active_ref(lay))
    assert np.array_equal(np.sort(_particles(g)["pids"]), np.arange(lay["nf"] + lay["nv"]))
    packs = list(dict.fromkeys(hl.layout(name)["packs"] + ONE_ZONE + TWO_ZONES))
    for zone in packs:
        buf = _fresh()
        g.halo_pack(*zone, buf.data_ptr(), CAP)
        _ok(g)
        n = _check_pack(_host(buf), CAP, act, raw, zone, f"{name} {which} halo_pack{zone}")
        zb = g.halo_zone_blocks(zone[0], zone[1])
        assert zb == hl.zone_blocks(act, zone[0], zone[1])
        assert n <= zb
        if 0 <= zone[0] + zone[2] and zone[1] + zone[2] < hl.NB:   # (no shifted layer leaves the grid)
            assert n == zb
    g.destroy()


# ---- b. the pack folded into the gather ----------------------------------------------------------------------------------
@pytest.mark.parametrize("nz", (1, 2))
@pytest.mark.parametrize("name,which", SIDES)
def test_folded_pack_over_three_substeps(name, which, nz):
    """substeps 1 and 3 pack the zones, substep 2 their two inner layers only, through the same buffers without a fill in
    between: every count starts from 0 again, and behind a smaller count the previous substep's words lie untouched"""
    zones = ONE_ZONE if nz == 1 else TWO_ZONES
    inner = [(lo + 1, hi - 1, sh) for lo, hi, sh in zones]
    g = _engine(hl.side(name, which))
    bufs = [_fresh() for _ in zones]
    counts = []
    for step, zs in enumerate((zones, inner, zones)):
        before = [_host(b).copy() for b in bufs] if step else [None] * len(bufs)
        _begin(g, zs, bufs)
        _ok(g)
        act, raw = _tables(g), _raw(g)
        counts.append([_check_pack(_host(b), CAP, act, raw, z, f"{name} {which} substep {step + 1} zone {z}", behind=w)
                       for b, z, w in zip(bufs, zs, before)])
        assert [g.halo_zone_blocks(z[0], z[1]) for z in zs] == counts[-1]
        _end(g, [])
    _ok(g)
    if name != "empty" or which == "right":
        assert sum(counts[1]) < sum(counts[0]) and sum(counts[2]) > sum(counts[1]), counts
    g.destroy()


# ---- c. the add kernel ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,which", SIDES)
def test_add(name, which):
    g = _engine(hl.side(name, which))
    _gather(g)
    _ok(g)
    act, raw0 = _tables(g), _raw(g)
    entries = _shuffled(_received(name, which, ONE_ZONE, act)[0], 5)
    have = set(act.tolist())
    assert any(b not in have for b, _ in entries)
    buf = _dev(hl.write_buffer(CAP, entries, extra_words=TAIL))
    g.halo_add(buf.data_ptr(), CAP)
    _ok(g)
    want = hl.add_ref(raw0, act, entries)
    _same_words(_raw(g), want, f"{name} {which}: the dense sums after halo_add")
    if name != "empty":
        assert (hl.words(want) != hl.words(raw0)).any()          # (the add matters)
    assert np.array_equal(_host(buf), hl.write_buffer(CAP, entries, extra_words=TAIL))
    g.destroy()


# ---- d. the add folded into the update -----------------------------------------------------------------------------------
def _unfolded(name, which, zones):
    """begin, then the received sums through halo_add, update_grid_from_sums and grid_to_particle: cached
    -> dict(act, raw0, entries per zone, grid, state)"""
    key = ("unfolded", name, which, len(zones))
    if key not in _CACHE:
        g = _engine(hl.side(name, which))
        send = [_fresh() for _ in zones]
        _begin(g, zones, send)
        _ok(g)
        act, raw0 = _tables(g), _raw(g)
        x0 = _particles(g)
        ent = _received(name, which, zones, act)
        for e in ent:
            g.halo_add(_dev(hl.write_buffer(CAP, e)).data_ptr(), CAP)
            g.gpu_sync()
        g.update_grid_from_sums(-1)
        g.grid_to_particle(DT)
        _ok(g)
        _CACHE[key] = dict(act=act, raw0=raw0, entries=ent, grid=_grid(g), state=_particles(g), before=x0)
        g.destroy()
    return _CACHE[key]


def _folded(name, which, zones, recv_entries, mid=False, probe=None):
    """begin, (mid,) end with the given received lists (one per buffer) -> (grid, state); probe(g) runs before end"""
    g = _engine(hl.side(name, which))
    send = [_fresh() for _ in zones]
    _begin(g, zones, send)
    if mid:
        g.substep_mid_halo(DT, -1)
    out = probe(g) if probe else None
    recv = [_dev(hl.write_buffer(CAP, e)) for e in recv_entries]
    _end(g, recv)
    _ok(g)
    res = (_grid(g), _particles(g), out)
    g.destroy()
    return res


@pytest.mark.parametrize("at", (0, 63, 64, 127, 128, -1))
def test_folded_add_finds_an_entry_at_every_scan_position(at):
    ref = _unfolded("straddle", "left", ONE_ZONE)
    entries = ref["entries"][0]
    assert len(entries) > 130
    # the block with the largest own mass among the received ones: its entry goes to position `at`
    have = set(ref["act"].tolist())
    mass = [float(ref["raw0"][b * 64:(b + 1) * 64, 3].sum()) * float(np.abs(d).sum() > 0) if b in have else -1.0
            for b, d in entries]
    k = int(np.argmax(mass))
    assert mass[k] > 0
    rest = _shuffled(entries[:k] + entries[k + 1:], 9)
    pos = len(rest) if at < 0 else at
    ordered = rest[:pos] + [entries[k]] + rest[pos:]
    grid, state, _ = _folded("straddle", "left", ONE_ZONE, [ordered])
    _same_grid(grid, ref["grid"], f"folded add, entry at {pos}, against add + update")
    _same_state(state, ref["state"], f"folded add, entry at {pos}, against add + update + GridToParticle")
    _grid_is(grid, hl.add_ref(ref["raw0"], ref["act"], entries), f"folded add, entry at {pos}")


@pytest.mark.parametrize("name,which", [(n, "left") for n in hl.NAMES] + [("straddle", "right"), ("one_sided", "right")])
def test_two_zones_folded_add_and_one_buffer_for_both(name, which):
    ref = _unfolded(name, which, TWO_ZONES)
    e0, e1 = ref["entries"]
    want = hl.add_ref(hl.add_ref(ref["raw0"], ref["act"], e0), ref["act"], e1)
    _grid_is(ref["grid"], want, f"{name} {which}: add + update")
    # two buffers, one per zone: the folded add
    grid, state, _ = _folded(name, which, TWO_ZONES, [_shuffled(e0, 1), _shuffled(e1, 2)])
    _same_grid(grid, ref["grid"], f"{name} {which}: two zones folded")
    _same_state(state, ref["state"], f"{name} {which}: two zones folded")
    # one buffer for both zones: k_halo_add2 in front of the update
    grid, state, _ = _folded(name, which, TWO_ZONES, [_shuffled(e0 + e1, 3)])
    _same_grid(grid, ref["grid"], f"{name} {which}: one buffer for two zones")
    _same_state(state, ref["state"], f"{name} {which}: one buffer for two zones")


# ---- e. the split update ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nz", (1, 2))
@pytest.mark.parametrize("name,which", [(n, "left") for n in hl.NAMES] + [("straddle", "right"), ("one_sided", "right")])
def test_split_update_equals_the_unsplit_one(name, which, nz):
    zones = ONE_ZONE if nz == 1 else TWO_ZONES
    ref = _unfolded(name, which, zones)
    want_raw = ref["raw0"]
    for e in ref["entries"]:
        want_raw = hl.add_ref(want_raw, ref["act"], e)
    recv = [_shuffled(e, 4 + k) for k, e in enumerate(ref["entries"])]
    whole_grid, whole_state, _ = _folded(name, which, zones, recv)
    _same_grid(whole_grid, ref["grid"], f"{name} {which} {nz} zones: begin / end")

    def between(g):
        g.gpu_sync()
        return _raw(g)

    grid, state, mid_raw = _folded(name, which, zones, recv, mid=True, probe=between)
    what = f"{name} {which} {nz} zones: begin / mid / end"
    _same_grid(grid, whole_grid, what + " against begin / end")
    _same_state(state, whole_state, what + " against begin / end")
    _grid_is(grid, want_raw, what)
    # between mid and end: the blocks outside every zone are updated from this rank's own sums, the zone blocks still
    # hold the raw sums
    m0, gv0, _ = hl.update_ref(ref["raw0"])
    bx = hl.block_coords(np.arange(hl.NBLOCKS))[0]
    done = np.repeat(hl.selected(bx, [z[:2] for z in zones], 0), 64)
    want_mid = np.concatenate([np.where(done[:, None], gv0, ref["raw0"][:, :3]), m0[:, None]], axis=1)
    _same_words(mid_raw, want_mid, what + ": the grid between mid and end")
    # every particle carries post-exchange values: GridToParticle of the restated grid on the positions before it
    x0 = ref["before"]
    assert np.array_equal(x0["pids"], state["pids"])
    p = tl.g2p64(x0["x"], hl.update_ref(want_raw)[1], hl.BITS)
    worst = {k: tl.margin(np.abs(state[k] - p[k]), p["b" + k]) for k in ("v", "C", "x")}
    for k, w in worst.items():
        hs.record(f"halo exchange: split update, {name} {which} {nz} zones, g2p {k}", w)
    assert all(w <= 1.0 for w in worst.values()), worst
    if name != "empty":   # (the received sums matter to particles near the cut: v against the pre-exchange grid differs)
        q = tl.g2p64(x0["x"], hl.update_ref(ref["raw0"])[1], hl.BITS)
        assert tl.margin(np.abs(state["v"] - q["v"]), q["bv"]) > 10.0


# ---- f. two ranks and the union --------------------------------------------------------------------------------------------
def _fem_by_pid(lay):
    """(taus, forces) by original particle id from the phase call on a twin engine (a substep call sums the vertex
    forces inside ParticleToGrid and stores none)"""
    from drake_amd import ARR as A
    g = _engine(lay)
    g.rebuild_mapping(False)
    g.calc_fem_state_and_force(DT)
    _ok(g)
    pids, taus, f = g.download(A.PIDS), g.download(A.TAUS), g.download(A.FORCES)
    g.destroy()
    n = lay["nf"] + lay["nv"]
    t, ff = np.zeros((n, 9), np.float32), np.zeros((n, 3), np.float32)
    face = pids < lay["nf"]
    t[pids[face]] = taus[face]
    ff[pids[~face]] = f[~face]
    return t, ff


def _p2g_inputs(g, lay, fem):
    from drake_amd import ARR as A
    pids = g.download(A.PIDS)
    return dict(pids=pids, x=g.download(A.POSITIONS), v=g.download(A.VELOCITIES), C=g.download(A.AFFINE),
                m=g.download(A.MASSES), taus=fem[0][pids], f=fem[1][pids])


def _exchange(name, pitch):
    """left and right engines on one stream, three substeps with the sends copied device to device.  Substep 1 adds the
    received sums with halo_add, so that the summed raw sums can be looked at; 2 and 3 add them inside the update."""
    key = ("exchange", name, pitch)
    if key in _CACHE:
        return _CACHE[key]
    import torch
    lays = {w: hl.side(name, w, pitch) for w in ("left", "right")}
    fem = {w: _fem_by_pid(lays[w]) for w in lays}
    eng = {w: _engine(lays[w]) for w in lays}
    zone = {w: hl.zone_of(w, pitch) for w in lays}
    stream = torch.cuda.Stream()
    send = {w: _fresh() for w in lays}
    recv = {w: _fresh() for w in lays}
    out = {w: {} for w in lays}
    with torch.cuda.stream(stream):
        for w, g in eng.items():
            g.set_stream(stream.cuda_stream)
        for step in range(3):
            for w, g in eng.items():
                _begin(g, [zone[w]], [send[w]])
            for w in lays:
                recv[w].copy_(send[_other(w)], non_blocking=True)
            if step == 0:
                for w, g in eng.items():
                    _ok(g)
                    d = out[w]
                    d["act"], d["raw0"], d["inputs"] = _tables(g), _raw(g), _p2g_inputs(g, lays[w], fem[w])
                    d["sent"] = _host(send[w]).copy()
                    g.halo_add(recv[w].data_ptr(), CAP)
                    _ok(g)
                    d["raw1"] = _raw(g)
                    g.update_grid_from_sums(-1)
                    g.grid_to_particle(DT)
                    _ok(g)
                    d["grid"], d["state1"] = _grid(g), _particles(g)
            else:
                for w, g in eng.items():
                    _end(g, [recv[w]])
            for w, g in eng.items():
                _ok(g)
                out[w].setdefault("gvs", []).append(_grid(g)["gvs"])
    for w, g in eng.items():
        out[w]["state3"] = _particles(g)
        g.destroy()
    _CACHE[key] = out
    return out


def _union(name):
    key = ("union", name)
    if key not in _CACHE:
        from drake_amd import ARR as A
        lay = hl.side(name, "union")
        g = _engine(lay)
        g.rebuild_mapping(False)
        g.calc_fem_state_and_force(DT)
        inp = _p2g_inputs(g, lay, (np.zeros((lay["nf"] + lay["nv"], 9), np.float32), np.zeros((lay["nf"] + lay["nv"], 3), np.float32)))
        face = inp["pids"] < lay["nf"]
        inp["taus"] = np.where(face[:, None], g.download(A.TAUS), 0.0).astype(np.float32)
        inp["f"] = np.where(face[:, None], 0.0, g.download(A.FORCES)).astype(np.float32)
        g.particle_to_grid(DT)
        raw = _raw(g)
        g.update_grid(-1)
        grid = _grid(g)
        g.grid_to_particle(DT)
        _ok(g)
        _CACHE[key] = dict(inputs=inp, raw=raw, grid=grid, state=_particles(g))
        g.destroy()
    return _CACHE[key]


@pytest.mark.parametrize("name,pitch", [(n, 0) for n in hl.EXCHANGE_NAMES] + [("straddle", hl.PITCH)])
def test_two_ranks_against_their_union(name, pitch):
    ex = _exchange(name, pitch)
    L, R = ex["left"], ex["right"]
    lay_u = hl.side(name, "union")
    gax = lay_u["gravity_axis"]
    # in the union's frame
    shift = {"left": 0, "right": pitch}
    frame = lambda w, dense: hl.to_union_frame(dense, shift[w]) if shift[w] else dense
    act = {}
    for w, d in (("left", L), ("right", R)):
        bx, by, bz = hl.block_coords(d["act"])
        act[w] = hl.block_id(bx + shift[w], by, bz)
        # what was sent is the rank's zone, relabelled for the other frame
        _check_pack(d["sent"], CAP, d["act"], d["raw0"], hl.zone_of(w, pitch), f"{name} pitch {pitch} {w}: sent")
    shared = np.intersect1d(act["left"], act["right"])
    zoned = hl.in_zone(hl.block_coords(shared)[0], [(hl.ZLO, hl.ZHI)])
    # (blocks of both ranks outside the zone are neighbours of home blocks that no stencil of one of the ranks reaches)
    apart = (shared[~zoned][:, None] * 64 + np.arange(64)).reshape(-1)
    assert not (frame("left", L["raw1"])[apart].any(axis=1) & frame("right", R["raw1"])[apart].any(axis=1)).any()
    shared = shared[zoned]
    assert len(shared) > 20
    cells = (shared[:, None] * 64 + np.arange(64)).reshape(-1)
    # the same pair of numbers on both ranks: identical sums, then identical velocities -- in every one of the substeps
    _same_words(frame("left", L["raw1"])[cells], frame("right", R["raw1"])[cells], f"{name} pitch {pitch}: summed raw sums")
    assert (hl.words(L["raw1"][cells]) != hl.words(L["raw0"][cells])).any()
    for k in ("gm", "gv", "gvs"):
        _same_words(frame("left", L["grid"][k])[cells], frame("right", R["grid"][k])[cells], f"{name} pitch {pitch}: {k}")
    for step in range(3):
        a, b = frame("left", L["gvs"][step])[cells], frame("right", R["gvs"][step])[cells]
        _same_words(a, b, f"{name} pitch {pitch}: GRID_V_STAR after substep {step + 1}")
        assert a.any()
    # the sums against the float64 sums over both ranks' particles
    both = {k: np.concatenate([L["inputs"][k], R["inputs"][k]]) for k in ("x", "v", "C", "m", "taus", "f")}
    both["x"] = both["x"].astype(np.float64)
    both["x"][len(L["inputs"]["x"]):, 0] += pitch / 16.0
    r = tl.p2g64(both["x"], both["v"], both["C"], both["m"], both["taus"], both["f"], hl.BITS, gax)
    quanta = tl.fixed_quanta(both["m"])
    bm, bmv = hl.union_bounds(r, quanta)
    u = _union(name)
    worst = {}
    fails = []
    # the nodes each rank's own particles reach (a rank's active blocks are the neighbours of its home blocks: outside
    # the zone some of them hold nothing of its own and lie under the other rank's particles -- no stencil of this rank
    # reaches them, nothing is exchanged there, and they must hold zeros; everywhere else in its active blocks the rank
    # holds the union's sum)
    nl = len(L["inputs"]["x"])
    reach = {}
    for w, sl in (("left", slice(0, nl)), ("right", slice(nl, None))):
        reach[w] = tl.p2g64(*(both[k][sl] for k in ("x", "v", "C", "m", "taus", "f")), hl.BITS, gax)["N"] > 0
    zone_cells = np.repeat(hl.in_zone(hl.block_coords(np.arange(hl.NBLOCKS))[0], [(hl.ZLO, hl.ZHI)]), 64)
    for w, d in (("left", L), ("right", R)):
        mine = np.zeros(hl.NCELLS, bool)
        mine[(act[w][:, None] * 64 + np.arange(64)).reshape(-1)] = True
        raw1 = frame(w, d["raw1"])
        assert not raw1[~mine].any()
        others = mine & ~zone_cells & reach[_other(w)]
        assert not (others & reach[w]).any() and not raw1[others].any()
        mine &= ~others
        worst[f"{w} sums mass"] = tl.margin(np.abs(raw1[mine, 3] - r["m"][mine]), bm[mine])
        worst[f"{w} sums momentum"] = tl.margin(np.abs(raw1[mine, :3] - r["mv"][mine]), bmv[mine])
        # GridToParticle on the rank's own grid
        inp, st = d["inputs"], d["state1"]
        assert np.array_equal(inp["pids"], st["pids"])
        p = tl.g2p64(inp["x"], d["grid"]["gv"], hl.BITS)
        for k in ("v", "C", "x"):
            worst[f"{w} g2p {k}"] = tl.margin(np.abs(st[k] - p[k]), p["b" + k])
        # ... and against the engine that holds both sets.  Both grids are within their P2G bounds of the same float64
        # sums, so the sums differ by at most da = bmv + bmv_u and dm = bm + bm_u; |a/m - a'/m'| <= (da + |v'| dm) / m,
        # plus the rounding of the two divisions; the walls clamp both alike.  GridToParticle is linear in the grid
        # velocities: the difference reaches a particle with its weights (g2p64's magnitude sums of that grid),
        # next to the two G2P bounds.
        uo = lay_u["orig"]
        lay_w = hl.side(name, w)
        upid = lay_w["orig"][st["pids"]]                    # this rank's particles in the union's numbering
        slot_u = np.empty(len(uo), np.int64)
        slot_u[u["state"]["pids"]] = np.arange(len(uo))
        su = slot_u[upid]
        bm_u, bmv_u = tl.p2g_bounds(r, quanta)
        gv_w, gv_u = frame(w, d["grid"]["gv"]).astype(np.float64), u["grid"]["gv"].astype(np.float64)
        m_w = raw1[:, 3].astype(np.float64)
        with np.errstate(all="ignore"):
            D = ((bmv + bmv_u) + np.abs(gv_u) * (bm + bm_u)[:, None]) / m_w[:, None] + tl.U32 * (np.abs(gv_w) + np.abs(gv_u))
        D[~(m_w > 0)] = 0.0
        x_u = inp["x"].astype(np.float64)
        x_u[:, 0] += shift[w] / 16.0
        s = tl.K * (tl.K_G2P_L + 16) * tl.U32
        spread = tl.g2p64(x_u, D, hl.BITS)
        pu = tl.g2p64(u["inputs"]["x"][su], u["grid"]["gv"], hl.BITS)
        # (in a frame of its own a rank rounds a face's centroid on another grid of floats: its positions may differ from
        # the union engine's by one spacing, and GridToParticle of the SAME grid at the two positions -- both evaluated
        # here in float64 from the inputs -- differs by `moved`, which the bound is widened by; 0 at pitch 0)
        xu0 = u["inputs"]["x"][su].astype(np.float64)
        # (((a + b) + c) / 3 in float32: the two sums round by <= 1/2 ulp(2 x) and 1/2 ulp(3 x), a third of which is
        # <= ulp(x), the division by another 1/2 ulp(x) -- 1.5 spacings in each frame)
        assert (np.abs(xu0 - x_u) <= 3.0 * np.spacing(np.abs(u["inputs"]["x"][su]))).all(), "the union engine starts elsewhere"
        assert pitch or np.array_equal(xu0, x_u)
        at_rank = tl.g2p64(x_u, u["grid"]["gv"], hl.BITS)
        moved = {k: np.abs(at_rank[k] - pu[k]) for k in ("v", "C", "x")}
        got_x = st["x"].astype(np.float64)
        got_x[:, 0] += shift[w] / 16.0
        worst[f"{w} against the union engine v"] = tl.margin(np.abs(st["v"] - u["state"]["v"][su]),
                                                             p["bv"] + pu["bv"] + spread["bv"] / s + moved["v"])
        worst[f"{w} against the union engine C"] = tl.margin(np.abs(st["C"] - u["state"]["C"][su]),
                                                             p["bC"] + pu["bC"] + spread["bC"] / s + moved["C"])
        worst[f"{w} against the union engine x"] = tl.margin(np.abs(got_x - u["state"]["x"][su]),
                                                             p["bx"] + pu["bx"] + tl.DT32 * spread["bv"] / s + moved["x"])
    for k, v in worst.items():
        hs.record(f"halo exchange: two ranks and the union, {name} pitch {pitch}, {k}", v)
        if not v <= 1.0:
            fails.append(f"{k}: {v:.3g} x the bound")
    assert not fails, fails


# ---- g. capacity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ("halo_pack", "substep_begin_halo"))
def test_a_buffer_one_block_too_small(route):
    from drake_amd import MpmError
    lay = hl.side("straddle", "left")
    zone = ONE_ZONE[0]

    def run(cap):
        """-> (error code or 0, error flags, buffer words, act, raw or None)"""
        g = _engine(lay)
        # the buffer sits inside a larger tensor: TAIL words of the fill pattern behind halo_buffer_bytes(cap)
        assert g.halo_buffer_bytes(cap) == hl.buffer_bytes(cap)
        buf = _fresh(cap)
        assert buf.numel() * 4 == g.halo_buffer_bytes(cap) + 4 * TAIL
        if route == "halo_pack":
            _gather(g)
            g.halo_pack(*zone, buf.data_ptr(), cap)
        else:
            _begin(g, [zone], [buf], cap)
        code = 0
        try:
            g.gpu_sync()
        except MpmError as err:
            code = err.code
        flags = g.stats()["error_flags"]
        res = (code, flags, _host(buf).copy(), _tables(g) if code == 0 else None, _raw(g) if code == 0 else None)
        g.destroy()
        return res

    zb = hl.zone_blocks(hl.active_ref(lay), zone[0], zone[1])
    code, flags, words_ok, act, raw = run(zb)
    assert code == 0 and flags == 0
    assert _check_pack(words_ok, zb, act, raw, zone, f"{route}, capacity = zone blocks") == zb
    code, flags, w, _, _ = run(zb - 1)
    assert code == MPM_ERR_CAPACITY and flags & ERR_CAPACITY_BIT, (code, flags)
    n, ids, data, tail = hl.read_buffer(w, zb - 1)
    assert n == zb                                   # every block asked for a slot; cap of them got one
    ref = hl.pack_ref(act, raw, *zone)
    got = ids.tolist()
    assert len(set(got)) == zb - 1 and set(got) <= set(ref)
    for k, bid in enumerate(got):
        assert np.array_equal(data[k], hl.words(ref[bid])), f"{route}: entry {k} (block {bid})"
    assert (tail == hl.FILL).all() and len(tail) == TAIL


# ---- h. the direct transport -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pitch", (0, hl.PITCH))
def test_direct_transport_between_two_engines_equals_device_copies(pitch):
    ex = _exchange("straddle", pitch)
    eng = {w: _engine(hl.side("straddle", w, pitch)) for w in ("left", "right")}
    eng["left"].chain_init(None, 0, 2, 0, hl.CUT, pitch, hl.ZONE_BLOCKS, CAP)
    eng["right"].chain_init(None, 1, 2, hl.CUT - pitch, hl.NB, pitch, hl.ZONE_BLOCKS, CAP)
    for g in eng.values():
        g.chain_direct_prepare()
    base = {w: g.chain_direct_base() for w, g in eng.items()}
    eng["left"].chain_direct_connect_local(None, base["right"])
    eng["right"].chain_direct_connect_local(base["left"], None)
    for _ in range(3):
        for g in eng.values():
            g.chain_substeps(1, DT, -1)
    for w, g in eng.items():
        _ok(g)
    for w, g in eng.items():
        _same_state(_particles(g), ex[w]["state3"], f"direct transport, pitch {pitch}, {w} rank after 3 substeps")
    for g in eng.values():
        g.chain_destroy()
        g.destroy()
