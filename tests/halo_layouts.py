"""Particle layouts for the exchange of raw node sums across a cut (k_halo_pack2, the pack folded into k_grid<0>,
k_halo_add2, the add folded into k_grid<2>, and the split update around the exchange: mpm_step.h, mpm_grid_update.inc),
exact float32 restatements of those operations, and the rounding bound of a sum that is formed in two halves.  CPU only:
nothing here imports the engine.

Geometry
--------
bits = 6: 64 cells and NB = 16 blocks per axis.  One cut at block CUT = 8 with ZONE_BLOCKS = 2: the zone is the block
layers ZLO..ZHI = 6..9 (cells 24..39).  A left and a right rank hold a particle set each, in the same frame (pitch 0) or
the right one moved by -PITCH blocks into a frame of its own (pitch 4: its zone is layers 2..5, the relabel is +-4).  A
rank of such a partition keeps its stencils inside the zone (k_p2g raises ERR_HALO otherwise on a partitioned engine), so
the left set's base cells end at column 37 (nodes <= 39) and the right set's begin at column 24: outside the zone no node
is reached from both sides, and after the exchange a rank holds the union's sum at every node of its active blocks that
lies in the zone or that the other rank does not reach (the rest -- neighbours of its home blocks under the other rank's
particles, outside the zone -- hold zeros, and none of its stencils reaches them).

Layouts (tests/transfer_layouts.py's disconnected triangles; every one gives `left`, `right`, `union` and `claims`, the
union built first and the sides cut out of it, so a particle has the same state wherever it appears)
--------
straddle    both sets have base cells in every x column 24..37 of the zone (the left one also 22, 23, the right one also
            38..41), so both reach every node column of layers 6..9; 4 x 4 home blocks in y, z: >= 130 active zone blocks
            on each rank (an active block is a neighbour of a home block), three steps of the folded add's 64-id scan
one_sided   home blocks of the left set only, of the right set only, and of both: zone blocks active on the sender only
            (the receiver drops the entry: lut_act < 0), on the receiver only (no entry: the sum stays) and on both
relabel     blocks at by, bz = 0 and NB - 1 (the wall band, the highest Morton bits), the right set also at bx = 0, 1 and
            14, 15; PACKS lists zones with shift +-4 and +-8, some of whose shifted bx leave [0, NB): those entries are
            skipped and the count is smaller
magnitudes  volumes over six decades; pairs of identical triangles on the two sides with opposite velocities and affine
            matrices and no stress (rest shape = shape): own + received cancels to rounding on the two axes without
            gravity; node rows reached from one side only inside blocks active on both (own mass 0, received > 0 and the
            reverse: s.w > 0 holds only after the add)
empty       the left set far from the cut: its zone holds no active block (count 0), and everything it receives names
            blocks it does not have; one neighbour only

Restatements (numpy, exact in float32: compared bit by bit)
--------
block_id / block_coords   mpm_math.h: Morton id of a block, x in the highest bit of each triple
pack_ref    {relabelled block id: (64, 4) float32} of the active blocks of a zone whose shifted bx stays in [0, nb)
add_ref     float32 add per cell for the listed blocks that are active; everything else untouched
update_ref  tl.grid32 on the result: what GRID_MASSES / GRID_MOMENTUM / GRID_V_STAR hold after k_grid<2>
selected / selected_pm1   halo_block_selected and halo_item_selected: the two passes of the split update
buffer layout             mpm_zone_buffer.h (mpm_halo_buffer_bytes): word 0 the count, ids from word 4, the sums 16-byte
                          aligned behind

Bound of a sum formed in two halves (u = 2^-24)
--------
Each rank sums its own particles, rounds to float32, and adds the neighbour's float32 sum in float32.  Against the
float64 sum over the union, per node and component:
    |f32(f32(S_L) + f32(S_R)) - S|  <=  tl's P2G bound for the union  +  3 u A_n
one extra rounding of each half (<= u |S_L|, u |S_R| <= u A_n each, and A_n^L + A_n^R = A_n, so together <= u A_n; 2 u A_n
allowed) and one of the add (<= u (|S_L| + |S_R|)(1 + u) <= u A_n (1 + u)).  On the engine each half is within the
union's bound too: L_n, N_n, A_n and the fixed-point quantum of a half are at most the union's, and A, N add up.
"""
import numpy as np

from tests import transfer_layouts as tl

BITS = 6
NB = 1 << (BITS - 2)
NBLOCKS = NB ** 3
NCELLS = NBLOCKS * 64
CUT = 8
ZONE_BLOCKS = 2
ZLO, ZHI = CUT - ZONE_BLOCKS, CUT + ZONE_BLOCKS - 1
PITCH = 4
FILL = 0xA5A5A5A5          # what a test writes into a buffer before the engine packs into it
L_COLS = range(22, 38)     # base cell columns of a left set: stencils end at node 39, the zone's last
R_COLS = range(24, 42)     # ... of a right set: stencils begin at node 24, the zone's first


# ---- Morton ids (mpm_math.h: spread3, compact3, block_id, block_coords) ---------------------------------------------
def spread3(v):
    v = np.asarray(v, np.uint64)
    m32 = np.uint64(0xFFFFFFFF)
    v = ((v * np.uint64(0x00010001)) & m32) & np.uint64(0xFF0000FF)
    v = ((v * np.uint64(0x00000101)) & m32) & np.uint64(0x0F00F00F)
    v = ((v * np.uint64(0x00000011)) & m32) & np.uint64(0xC30C30C3)
    v = ((v * np.uint64(0x00000005)) & m32) & np.uint64(0x49249249)
    return v


def compact3(v):
    v = np.asarray(v, np.uint64) & np.uint64(0x09249249)
    v = (v ^ (v >> np.uint64(2))) & np.uint64(0x030C30C3)
    v = (v ^ (v >> np.uint64(4))) & np.uint64(0x0300F00F)
    v = (v ^ (v >> np.uint64(8))) & np.uint64(0xFF0000FF)
    v = (v ^ (v >> np.uint64(16))) & np.uint64(0x000003FF)
    return v


def block_id(bx, by, bz):
    return (spread3(bx) * np.uint64(4) + spread3(by) * np.uint64(2) + spread3(bz)).astype(np.int64)


def block_coords(ids):
    """-> (bx, by, bz) int64 arrays"""
    ids = np.asarray(ids, np.uint64)
    return tuple(compact3(ids >> np.uint64(s)).astype(np.int64) for s in (2, 1, 0))


# ---- the exchange, restated ------------------------------------------------------------------------------------------
def raw_dense(gm, gmv):
    """(ncells, 4) float32 (mv_x, mv_y, mv_z, m): the engine's float4 per node from the downloaded dense arrays"""
    return np.concatenate([tl.f32(gmv).reshape(-1, 3), tl.f32(gm).reshape(-1, 1)], axis=1)


def pack_ref(act_block, raw, lo, hi, shift, nb=NB):
    """{relabelled id: (64, 4) float32}: every active block with lo <= bx <= hi whose bx + shift stays in [0, nb)"""
    act = np.asarray(act_block, np.int64)
    bx, by, bz = block_coords(act)
    out = {}
    for a, x, y, z in zip(act.tolist(), bx.tolist(), by.tolist(), bz.tolist()):
        if x < lo or x > hi or not 0 <= x + shift < nb:
            continue
        out[int(block_id(x + shift, y, z))] = raw[a * 64:(a + 1) * 64].copy()
    return out


def zone_blocks(act_block, lo, hi):
    """mpm_halo_zone_blocks: the number of active blocks with lo <= bx <= hi"""
    bx = block_coords(act_block)[0]
    return int(((bx >= lo) & (bx <= hi)).sum())


def add_ref(raw, active_ids, entries):
    """raw (ncells, 4) float32 with the entries [(id, (64, 4) float32)] added in float32 at every listed block that is
    active; entries of other blocks are dropped"""
    out = tl.f32(raw).copy()
    act = set(np.asarray(active_ids, np.int64).tolist())
    for bid, data in (entries.items() if isinstance(entries, dict) else entries):
        if int(bid) in act:
            out[int(bid) * 64:(int(bid) + 1) * 64] += tl.f32(data)
    return out


def update_ref(raw, bits=BITS):
    """-> (gm, gv, gvs) after the update from sums without colliders: the mass, v where m > 0 (the sum as it is
    elsewhere) and v* (0 where m == 0), bit for bit what the engine's three dense grid arrays hold"""
    m, mv = raw[:, 3].copy(), raw[:, :3].copy()
    v = tl.grid32(m, mv, bits)
    gv = np.where((m > 0)[:, None], v, mv)
    return m, gv, v


def in_zone(bx, zones):
    bx = np.asarray(bx)
    z = np.zeros(bx.shape, bool)
    for lo, hi in zones:
        z |= (bx >= lo) & (bx <= hi)
    return z


def selected(bx, zones, cls):
    """halo_block_selected: the blocks the grid update of pass `cls` touches (0: outside every zone, before the
    exchange; 1: the zone blocks, after it; < 0: all)"""
    bx = np.asarray(bx)
    return np.ones(bx.shape, bool) if cls < 0 else in_zone(bx, zones) == bool(cls)


def selected_pm1(bx, zones, cls):
    """halo_item_selected: the home blocks whose particles GridToParticle of pass `cls` moves -- pass 1 takes every
    block within one block of a zone, whose stencils reach zone nodes"""
    bx = np.asarray(bx)
    near = in_zone(bx - 1, zones) | in_zone(bx, zones) | in_zone(bx + 1, zones)
    return np.ones(bx.shape, bool) if cls < 0 else near == bool(cls)


# ---- buffer layout (mpm_halo_buffer_bytes; zbuf_ids_offset, zbuf_data_offset, zone_buffer_bytes in mpm_zone_buffer.h) ---
def buffer_bytes(cap):
    return (((4 + cap) * 4 + 15) // 16) * 16 + cap * 64 * 16


def _data_word(cap):
    return (((4 + cap) * 4 + 15) // 16) * 4


def write_buffer(cap, entries, fill=FILL, extra_words=0):
    """uint32 words of a buffer of capacity `cap` holding `entries` [(id, (64, 4) float32)] in the order given, every
    other word `fill`, `extra_words` of `fill` behind it"""
    assert len(entries) <= cap
    w = np.full(buffer_bytes(cap) // 4 + extra_words, fill, np.uint32)
    w[0] = len(entries)
    w[1:4] = 0
    d0 = _data_word(cap)
    for k, (bid, data) in enumerate(entries):
        w[4 + k] = bid
        w[d0 + k * 256:d0 + (k + 1) * 256] = np.ascontiguousarray(tl.f32(data)).view(np.uint32).reshape(-1)
    return w


def read_buffer(words, cap):
    """-> (count word, ids (cap,) uint32, data (cap, 64, 4) as uint32 words, whatever lies behind the buffer)"""
    w = np.asarray(words, np.uint32)
    d0 = _data_word(cap)
    return int(w[0]), w[4:4 + cap].copy(), w[d0:d0 + cap * 256].reshape(cap, 64, 4).copy(), w[buffer_bytes(cap) // 4:].copy()


def words(a):
    return np.ascontiguousarray(tl.f32(a)).view(np.uint32)


# ---- the bound of a sum formed in two halves -------------------------------------------------------------------------
def union_bounds(r_union, quanta=None):
    """(bm, bmv): tl's P2G bound for the union plus 3 u A_n (module docstring)"""
    bm, bmv = tl.p2g_bounds(r_union, quanta)
    return bm + 3.0 * tl.U32 * r_union["A_m"], bmv + 3.0 * tl.U32 * r_union["A_mv"]


def active_ref(lay):
    """ascending ids of the active blocks after the re-sort of the uploaded state: the neighbours of the home blocks
    (tl.binning's float64 restatement of the anticipatory binning)"""
    blk = np.unique(tl.binning(lay)["block"], axis=0)
    o = np.arange(27)
    off = np.stack([o // 9 - 1, (o // 3) % 3 - 1, o % 3 - 1], -1)
    n = (blk[:, None, :] + off[None]).reshape(-1, 3)
    n = n[((n >= 0) & (n < NB)).all(axis=1)]
    return np.unique(block_id(n[:, 0], n[:, 1], n[:, 2]))


def shift_frame(lay, blocks):
    """the layout moved by -`blocks` blocks along x (exact in float32 for the positions used here: see the test)"""
    out = dict(lay)
    s = np.float32(blocks * 4.0 / (1 << BITS))
    out["pos"] = lay["pos"].copy()
    out["pos"][:, 0] -= s
    cl = []
    for rest, vel, idx in lay["cloths"]:
        rest = rest.copy()
        rest[:, 0] -= s
        cl.append((rest, vel, idx))
    out["cloths"] = cl
    out["frame_shift"] = blocks
    return out


def to_union_frame(dense, blocks):
    """a dense per-cell array of a frame moved by -`blocks` blocks, re-indexed by the union frame's cell keys (cells
    the moved frame does not have: 0)"""
    dense = np.asarray(dense)
    xyz = tl.key_coords(BITS)
    out = np.zeros_like(dense)
    ok = xyz[:, 0] - 4 * blocks >= 0
    src = tl.cell_key(xyz[ok, 0] - 4 * blocks, xyz[ok, 1], xyz[ok, 2])
    out[np.flatnonzero(ok)] = dense[src]
    return out


# ---- builders ----------------------------------------------------------------------------------------------------------
class _Two:
    """one mesh for the union; every triangle belongs to the left (0) or the right (1) set"""

    def __init__(self, seed):
        self.M = tl._Mesh(BITS, seed)
        self.rng = self.M.rng
        self.side = []

    def cell(self, side, b, vel=None, size=0.3):
        """a small triangle whose four particles have base cell b (t = b + 1/2 +- size on every axis)"""
        vel = self.rng.uniform(-0.3, 0.3, 3) if vel is None else vel
        self.M.small(np.asarray(b, np.float64) + 1.0, size, vel)
        self.side.append(side)

    def twin(self, side):
        """the last triangle once more, for `side`; -> (index of the original, index of the copy)"""
        v = self.M.verts[-1]
        self.M.tri(v[0], v[1], v[2], vel=self.M.vvel[-1])
        self.side.append(side)
        return len(self.side) - 2, len(self.side) - 1


def _subset(lay, tris):
    """the layout of the triangles `tris` of a one-cloth layout; `orig`: their particles' indices in `lay`"""
    tris = np.asarray(tris, np.int64)
    nf, nt = lay["nf"], len(tris)
    vsel = (3 * tris[:, None] + np.arange(3)).reshape(-1)
    sel = np.r_[tris, nf + vsel]
    rest, vel, _ = lay["cloths"][0]
    idx = np.arange(3 * nt, dtype=np.int32).reshape(nt, 3)
    out = dict(lay)
    out.update(cloths=[(rest[vsel].copy(), vel[vsel].copy(), idx)], nf=nt, nv=3 * nt, idx_all=idx.copy(), orig=sel)
    for k in ("pos", "vel", "C", "vol", "mass", "taus", "forces"):
        out[k] = lay[k][sel].copy()
    return out


def _finish(name, T, gravity_axis, claims, packs=None, post=None, **kw):
    u = tl._finish(name, [T.M], gravity_axis, {}, **kw)
    if post:
        post(u)
    _clear_of_binning_boundaries(u, claims.get("pairs", ()))
    side = np.asarray(T.side)
    u["orig"] = np.arange(u["nf"] + u["nv"])
    return dict(name=name, union=u, left=_subset(u, np.flatnonzero(side == 0)), right=_subset(u, np.flatnonzero(side == 1)),
                claims=claims, packs=packs or [(ZLO, ZHI, 0)])


BIN_MARGIN = 0.02          # cells: how far every particle stays from a boundary of the re-sort's binning


def _clear_of_binning_boundaries(u, pairs):
    """slows triangles down (x 0.9, a twin with its original) until no particle is binned within BIN_MARGIN cells of a
    boundary: the home blocks, and with them the active blocks, are then the same in float32 and in float64"""
    nf = u["nf"]
    partner = {}
    for a, b in pairs:
        partner[a], partner[b] = b, a
    for _ in range(200):
        bad = np.flatnonzero(tl.binning(u)["margin"] < BIN_MARGIN)
        tris = {int(i) if i < nf else int(i - nf) // 3 for i in bad}
        tris |= {partner[t] for t in tris if t in partner}
        if not tris:
            return
        for t in tris:
            _set_vertex_vel(u, t, u["vel"][nf + 3 * t:nf + 3 * t + 3] * np.float32(0.9))
    raise AssertionError("particles on a binning boundary")


def _set_vertex_vel(u, tri, vel3):
    """velocities (3, 3) of triangle `tri`'s corners; the face's as _finish forms it"""
    nf = u["nf"]
    u["vel"][nf + 3 * tri:nf + 3 * tri + 3] = vel3
    v = tl.f32(vel3)
    u["vel"][tri] = ((v[0] + v[1]) + v[2]) / np.float32(3)


def straddle(seed=21):
    T = _Two(seed)
    for by in range(3, 7):
        for bz in range(3, 7):
            for side, cols in ((0, L_COLS), (1, R_COLS)):
                for x in cols:
                    T.cell(side, (x, 4 * by + T.rng.integers(0, 4), 4 * bz + T.rng.integers(0, 4)))
    return _finish("straddle", T, 2, dict(both_reach=(24, 37), zone_active_min=130), seed=seed)


# y home blocks of one_sided: the left set only, the right set only, both (their neighbourhoods do not meet)
ONE_SIDED_BY = dict(left=3, right=7, both=11)


def one_sided(seed=22):
    T = _Two(seed)
    for bz in (4, 8):
        for side, cols in ((0, L_COLS), (1, R_COLS)):
            for by in (ONE_SIDED_BY["left" if side == 0 else "right"], ONE_SIDED_BY["both"]):
                for x in cols:
                    T.cell(side, (x, 4 * by + 1, 4 * bz + 1))
    return _finish("one_sided", T, 0, dict(one_sided=True), seed=seed)


RELABEL_PACKS = [(ZLO, ZHI, +4), (ZLO, ZHI, -4), (ZLO, ZHI, +8), (ZLO, ZHI, -8), (0, 3, -4), (0, 3, +4), (12, 15, +4),
                 (12, 15, -8), (0, NB - 1, +1)]


def relabel(seed=23):
    T = _Two(seed)
    corners = [(1, 1), (1, 60), (60, 1), (60, 60), (30, 30)]
    for y, z in corners:
        for x in L_COLS:
            T.cell(0, (x, y, z))
        for x in list(R_COLS) + [1, 2, 5, 6, 57, 58, 60]:
            T.cell(1, (x, y, z))
    return _finish("relabel", T, 1, dict(corners=True), packs=RELABEL_PACKS, seed=seed)


def magnitudes(seed=24):
    T = _Two(seed)
    pairs, rows = [], []
    for x in range(24, 38):
        for y, z in ((17, 17), (21, 18)):
            T.cell(0, (x, y, z))
            pairs.append(T.twin(1))
        # node rows of one side only inside a block of both: base y = 32 reaches rows 32..34, base y = 33 rows 33..35
        T.cell(0, (x, 32, 34))
        T.cell(1, (x, 33, 34))
        rows.append((x, 32, 35, 34))
    for side, cols in ((0, L_COLS), (1, R_COLS)):
        for x in cols:
            for _ in range(3):
                T.cell(side, (x, T.rng.integers(16, 28), T.rng.integers(16, 28)))

    def post(u):
        nf = u["nf"]
        # no stress: the rest shape is the shape
        rest = u["pos"][nf:].copy()
        u["cloths"] = [(rest, u["cloths"][0][1], u["cloths"][0][2])]
        for k, (a, b) in enumerate(pairs):
            va = u["vel"][nf + 3 * a:nf + 3 * a + 3]
            _set_vertex_vel(u, b, -va * np.float32(1.0 + 2.0 ** -20 * (1 + k % 3)))
            pa, pb = np.r_[a, nf + 3 * a + np.arange(3)], np.r_[b, nf + 3 * b + np.arange(3)]
            u["C"][pb] = -u["C"][pa]
            u["vol"][pb] = u["vol"][pa]
            u["mass"][pb] = u["mass"][pa]

    return _finish("magnitudes", T, 1, dict(vol_decades=6, pairs=pairs, rows=rows), post=post, vel_scale=(1e-3, 10.0),
                   C_scale=(1e-3, 10.0), vol_decades=6.0, seed=seed)


def empty(seed=25):
    T = _Two(seed)
    for x in range(4, 13):
        for _ in range(4):
            T.cell(0, (x, T.rng.integers(16, 28), T.rng.integers(16, 28)))
    for x in R_COLS:
        for _ in range(2):
            T.cell(1, (x, T.rng.integers(16, 28), T.rng.integers(16, 28)))
    return _finish("empty", T, 2, dict(left_zone_empty=True), seed=seed)


BUILDERS = dict(straddle=straddle, one_sided=one_sided, relabel=relabel, magnitudes=magnitudes, empty=empty)
NAMES = tuple(BUILDERS)
EXCHANGE_NAMES = ("straddle", "one_sided", "magnitudes")   # the layouts of the two-rank exchange against the union
_CACHE = {}


def layout(name):
    if name not in _CACHE:
        _CACHE[name] = BUILDERS[name]()
    return _CACHE[name]


def side(name, which, pitch=0):
    """the left / right / union particle set of layout `name`; at pitch > 0 the right one in a frame of its own"""
    lay = layout(name)[which]
    return shift_frame(lay, pitch) if (which == "right" and pitch) else lay


def zone_of(which, pitch=0):
    """(lo, hi, shift) of the one zone a rank of the two-rank partition packs"""
    if which == "left":
        return (ZLO, ZHI, -pitch)
    return (ZLO - pitch, ZHI - pitch, +pitch)
