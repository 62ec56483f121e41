"""The contact solve of a partitioned domain (mpm_contact.h: zone_exchange3, partitioned_direction, newton_*_host;
mpm_contact_dev.h: k_ct_flags_to_field, k_zone_pack<3> / k_zone_add<3>, k_ct_node_dir<1> / <2>, node_owned; mpm_team.h)
restated on the layouts of tests/contact_layouts.py (`cl`) cut into x slabs, and layouts built around a cut.  CPU only:
nothing here imports the engine.  Every restated phase is cl's (stencil, gather, contact_terms, direction, line_search,
impulses, chain_lengths): this module only says who holds what.

The split (cuts: world + 1 ascending x block indices, mpm_dist_init's)
----------------------------------------------------------------------
    particle -> the rank whose slab [4 cuts[r], 4 cuts[r + 1]) holds its base cell's x (k_dist_init_roles)
    contact  -> the rank that owns its particle (the contact position is the particle's)
    node     -> the rank whose slab holds its x cell (node_owned)
    zone of a cut c: the x blocks c - Z .. c + Z - 1 (Z = zone_blocks), sent by both ranks of the cut to each other
A rank lists the nodes its own contacts reach plus, through the one-off exchange of node flags, the nodes of zone blocks
active on both ranks that the neighbour's contacts reach (`node_lists`).  Per Newton iteration it gathers the (H, G) sums
of its own contacts at every listed node (zeros included), the zone exchange adds the neighbour's sums, and it solves
from the total; |Dir|^2, the DoF count and the inertia part of the energies take every node from its owner only.

What a rank must hold at a listed node is fl(own sums + neighbour's sums) (`held32`; two terms: the order does not
matter), so both ranks of a cut hold the same bits there.  Against the float64 restatement of the UNION (all contacts on
one grid, every node's grid values taken from its owner) the bound is cl's with ONE change, derived, not measured: a
node that receives a neighbour's non-zero sums has exactly one more float addition in its chain, L_n + 1 (`received`,
passed through cl.chain_lengths).  Nothing else changes: splitting the contacts over ranks only shortens segments, and
adding a neighbour's zeros is exact.

Layouts
-------
    cl.NAMES   as they are, cut at block 8 (cell 32); regimes_mu0 also at block 7 and fringe at block 11, where more
               nodes see contacts of both sides (MORE)
    cut        built around x = 32, for zone_blocks 1 and 2.  Base cells in every x column 24 .. 39 of a shared
               region (columns 28 .. 35: the four columns either side of the cut, the last owned column of each side
               reaching two cells into the neighbour's slab; columns 24 .. 27 and 36 .. 39: the outermost blocks of the
               zone of zone_blocks = 2), every regime of cl.REGIMES in every column, and
        a  regions where only ONE rank has contacts in the columns next to the cut: nodes that get onto the other rank's
           list through the flag exchange alone (the other rank owns those of x >= 32 / x < 32 and counts their DoFs)
        b  nodes reached by both ranks' contacts in every regime
        c  an isolated triangle 5 columns beyond the cut, far from everything the other rank holds: its blocks are
           active on the sender, in the zone, and not active on the receiver (dropped: ZBUF_FOREIGN)
        d  listed nodes whose own rank's sums are exactly zero (the nodes of a; and, in a second solve through the same
           engines with `second_pairs`, nodes that had own sums in the first solve)
        e  two light contacts, one per rank, at one isolated spot: at their common nodes each rank's |H|_F and |G|
           lie below the 1e-7 DoF threshold and the total above it, clear of the bounds
        f  contacts in the zone's outermost blocks (distance zone_blocks from the cut)
    three, three_empty   cuts [0, 7, 9, 16], zone_blocks 1: the middle slab is two zones wide (the narrowest
               mpm_dist_init admits), the middle rank exchanges with both sides in one launch; three_empty leaves
               rank 2 without a contact (it owns nodes that rank 1's contacts reach)
"""
import numpy as np

from tests import contact_layouts as cl
from tests import migration as mg
from tests import transfer_layouts as tl

BITS = cl.BITS
N = 1 << BITS
NB = N // 4
CUT_BLOCK = 8
CUT = 4 * CUT_BLOCK
TWO = (0, CUT_BLOCK, NB)
THREE = (0, 7, 9, NB)
SHARED = (20.0, 27.0)          # y, z range of the region where both ranks have contacts


def node_x(keys):
    return tl.key_coords(BITS)[np.asarray(keys, np.int64), 0]


def node_block(keys):
    return np.asarray(keys, np.int64) >> 6


# ---- the split ---------------------------------------------------------------------------------------------------------
def slabs(cuts):
    """[(own_lo, own_hi)] in cells; the outermost ranks extend to the walls"""
    world = len(cuts) - 1
    return [(4 * cuts[r] if r > 0 else 0, 4 * cuts[r + 1] if r < world - 1 else N) for r in range(world)]


def particle_owner(lay, cuts):
    xi = mg.xi32(lay["pos"][:, 0], lay["bits"])
    bx = mg.cell_x(xi, lay["bits"])
    owner = np.full(len(bx), -1, np.int64)
    for r, (lo, hi) in enumerate(slabs(cuts)):
        owner[(bx >= lo) & (bx < hi)] = r
    return owner


def held(lay, cuts, zone_blocks):
    """per rank: the particles mpm_dist_init keeps (owned, or inside the band in which the rank keeps ghosts; band widths
    from the mesh, tests/migration.py: band_rules)"""
    rest, vel, idx = lay["cloths"][0]
    rules = mg.band_rules(mg.longest_edge_cells(rest, idx, lay["bits"]), zone_blocks, 0, 0)
    xi = mg.xi32(lay["pos"][:, 0], lay["bits"])
    bx = mg.cell_x(xi, lay["bits"])
    w = np.where(np.arange(len(xi)) < lay["nf"], rules["ghost_w"], rules["vert_w"]).astype(np.float32)
    out = []
    world = len(cuts) - 1
    for r, (lo, hi) in enumerate(slabs(cuts)):
        keep = (bx >= lo) & (bx < hi)
        if r > 0:
            keep |= (bx < lo) & (xi >= (np.float32(lo) - w).astype(np.float32))
        if r < world - 1:
            keep |= (bx >= hi) & (xi < (np.float32(hi) + w).astype(np.float32))
        out.append(keep)
    return out


def split(lay, cuts, zone_blocks=1):
    """per rank: dict(rank, sel (indices of its contacts, ascending), owned (dense bool: the nodes it owns), zones
    {neighbour: (first, last x block of the zone they exchange)}, flags (dense keys of the nodes its contacts reach))"""
    b, wt, keys = cl.stencil(lay)
    owner_p = particle_owner(lay, cuts)
    owner_c = owner_p[lay["cp"]["particle"]]
    X = tl.key_coords(lay["bits"])[:, 0]
    world = len(cuts) - 1
    out = []
    for r, (lo, hi) in enumerate(slabs(cuts)):
        sel = np.nonzero(owner_c == r)[0]
        zones = {}
        if r > 0:
            zones[r - 1] = (cuts[r] - zone_blocks, cuts[r] + zone_blocks - 1)
        if r < world - 1:
            zones[r + 1] = (cuts[r + 1] - zone_blocks, cuts[r + 1] + zone_blocks - 1)
        out.append(dict(rank=r, sel=sel, owned=(X >= lo) & (X < hi), zones=zones, own=(lo, hi),
                        flags=np.unique(keys[sel]) if len(sel) else np.zeros(0, np.int64)))
    return out


def node_lists(parts, active=None):
    """per rank: the sorted dense keys of its node list -- its own contacts' nodes plus the neighbours' flagged nodes in
    zone blocks active on both ranks.  active: per rank the ids of its active blocks (the engine's ACT_BLOCK table); None:
    every zone block the neighbour flags is taken as active here"""
    out = []
    for p in parts:
        got = [p["flags"]]
        for s, (blo, bhi) in p["zones"].items():
            f = parts[s]["flags"]
            bx = node_x(f) >> 2
            ok = (bx >= blo) & (bx <= bhi)
            if active is not None:
                ok &= np.isin(node_block(f), active[p["rank"]]) & np.isin(node_block(f), active[s])
            got.append(f[ok])
        out.append(np.unique(np.concatenate(got)))
    return out


def received(parts, lists):
    """dense keys of the nodes at which some rank adds a neighbour's non-zero sums: listed on two ranks and reached by
    the contacts of both"""
    out = []
    for p in parts:
        for s in p["zones"]:
            if s > p["rank"]:
                both = np.intersect1d(p["flags"], parts[s]["flags"])
                out.append(both[np.isin(both, lists[p["rank"]]) & np.isin(both, lists[s])])
    return np.unique(np.concatenate(out)) if out else np.zeros(0, np.int64)


def sub_terms(T, sel):
    """cl.contact_terms' per-contact arrays of a subset of the contacts"""
    return {k: (v[sel] if isinstance(v, np.ndarray) and len(v) == len(T["H"]) else v) for k, v in T.items()}


def rank_sums(lay, P, wt, keys, mass_c, T, grid, parts):
    """the float64 (H, G) sums of every rank's own contacts, on the union's node axis: (nodes, [(Hn (n, 9), Gn (n, 3))])"""
    gm, gv, gvs = grid
    nodes = np.unique(keys)
    out = []
    for p in parts:
        Hn, Gn = np.zeros((len(nodes), 9)), np.zeros((len(nodes), 3))
        sel = p["sel"]
        if len(sel):
            dr = cl.direction(lay, P, wt[sel], keys[sel], np.asarray(mass_c)[sel], sub_terms(T, sel), gm, gv, gvs)
            at = np.searchsorted(nodes, dr["nodes"])
            Hn[at], Gn[at] = dr["Hn"], dr["Gn"]
        out.append((Hn, Gn))
    return nodes, out


def held32(own, others):
    """what a rank holds at its listed nodes after the zone exchange: fl(own + neighbour's), float32 arrays in and out
    (at most one of `others` is non-zero at a node: zones of different cuts do not overlap)"""
    tot = tl.f32(own).copy()
    for o in others:
        tot = tot + tl.f32(o)
    return tot


# ---- builders ------------------------------------------------------------------------------------------------------------
def _regime_contact(L, t, corner, reg, pset="soft"):
    """one contact of the given regime of cl.REGIMES (cl.regimes' recipe)"""
    k, d, dt, mu = cl.params32(pset)
    nrm = cl._sphere(L.rng, 1)[0]
    n = -nrm
    phi0 = L.rng.uniform(2e-4, 2e-3)
    vhat = min(phi0 / dt, 1.0 / d if d > 0 else np.inf)
    if reg == "separating":
        vn, vt = vhat * L.rng.uniform(1.2, 2.0) + 0.01, L.rng.uniform(0.0, 0.3)
    else:
        vn = -L.rng.uniform(0.02, 0.4)
        vt = {"sliding": L.rng.uniform(100 * cl.EPSV, 0.4), "sticking": L.rng.uniform(0.0, 0.005 * cl.EPSV),
              "transitional": cl.EPSV * L.rng.uniform(0.3, 3.0)}[reg]
    L.contact(t, corner, nrm, -phi0, u_rel=vn * n + cl._tangent(L.rng, n, vt))


def _column(L, c, n_tri, yz, regimes=cl.REGIMES, vol=1.0):
    """n_tri triangles whose four particles have base cell x = c (u in [c + 0.7, c + 1.3]), y and z uniform in yz"""
    for j in range(n_tri):
        ctr = np.array([c + 1.0, L.rng.uniform(*yz), L.rng.uniform(*yz)])
        t = L.tri(ctr, 0.28, L.rng.uniform(-0.3, 0.3, 3), vol=vol)
        for corner in range(4):
            _regime_contact(L, t, corner, regimes[(4 * j + corner + c) % len(regimes)])


E_SPOT = (12.0, 12.0)          # y, z of case e's two contacts
C_SPOTS = {0: (CUT - 6, 8.0), 1: (CUT + 5, 56.0)}      # per rank: x column and y = z of case c's isolated triangle
A_REGIONS = {0: (40.0, 43.0), 1: (48.0, 51.0)}          # per rank: y, z range where only that rank has contacts


def _build_cut(vol_e, seed=21):
    L = cl._Layout("cut", seed, "soft")
    for c in range(CUT - 8, CUT + 8):
        _column(L, c, 12, SHARED)
    # a: only one rank has contacts here, in its two columns next to the cut (approaching: they make DoFs)
    for r, cols in ((0, (CUT - 2, CUT - 1)), (1, (CUT, CUT + 1))):
        for c in cols:
            _column(L, c, 6, A_REGIONS[r], regimes=("sliding", "transitional"))
    # c (and f for zone_blocks = 2): isolated triangles
    for r, (c, s) in C_SPOTS.items():
        _column(L, c, 1, (s, s + 0.5), regimes=("sliding",))
    # e: one light contact per rank on the face particle, the same normal and the same sliding relative velocity (their
    # sums add up), base cells 31 and 32; stencils share the x nodes 32 and 33
    nrm = cl._unit(np.array([0.2, -0.1, 1.0]))
    u = nrm * 0.2 + cl._unit(np.cross(nrm, [1.0, 0.0, 0.0])) * 0.25        # (n = -normal: n . u < 0, approaching)
    for r, ux in ((0, CUT + 0.3), (1, CUT + 0.7)):
        t = L.tri(np.array([ux, E_SPOT[0] + 1.0, E_SPOT[1] + 1.0]), 0.04, np.array([0.1, -0.05, 0.02]), vol=vol_e[r])
        L.contact(t, 3, nrm, -1e-3, u_rel=u)
    return L.finish(dict(cut_cases=("a", "b", "c", "d", "e", "f")))


def _e_nodes(lay, parts, grid=None):
    """case e at the common nodes of its two contacts: (nodes, per rank (hF, gF, eHF, eGF), union direction dict)"""
    P = cl.params32(lay["params"])
    cp = lay["cp"]
    vp = lay["vel"][cp["particle"]].astype(np.float64)
    mass_c = lay["mass"][cp["particle"]].astype(np.float64)
    b, wt, keys, T = cl.prepare(lay, P, None, None, None, vp, mass_c)
    ncell = 1 << (3 * lay["bits"])
    gm = np.ones(ncell) if grid is None else grid[0]
    z = np.zeros((ncell, 3))
    e_c = [int(p["sel"][-1]) for p in parts]      # (the two contacts of e are the last of each rank)
    common = np.intersect1d(keys[e_c[0]], keys[e_c[1]])
    per = []
    for p in parts:
        sel = p["sel"]
        dr = cl.direction(lay, P, wt[sel], keys[sel], mass_c[sel], sub_terms(T, sel), gm, z, z)
        at = np.searchsorted(dr["nodes"], common)
        eHF = 3.0 * dr["eHn"][at] + 20 * cl.U32 * dr["hF"][at]
        eGF = np.sqrt(3.0) * dr["eGn"][at] + 20 * cl.U32 * dr["gF"][at]
        per.append((dr["hF"][at], dr["gF"][at], eHF, eGF))
    lists = node_lists(parts)
    un = cl.direction(lay, P, wt, keys, mass_c, T, gm, z, z, received=received(parts, lists))
    return common, per, un


def cut():
    # the masses of e's two triangles: from a first build with unit volumes, so that at the common node where the smaller
    # of the two ranks' sums is largest, each rank's larger norm is 0.7e-7 (the sums are linear in the contact mass)
    lay = _build_cut((1.0, 1.0))
    parts = split(lay, TWO)
    common, per, un = _e_nodes(lay, parts)
    big = [np.maximum(h, g) for h, g, _, _ in per]
    at = int(np.argmax(np.minimum(big[0], big[1])))
    lay = _build_cut(tuple(0.7 * cl.THRESH / float(b[at]) for b in big))
    lay["second_pairs"] = second_pairs(lay)
    return lay


def second_pairs(lay):
    """d: the contacts of a second solve through the same engines -- the first solve's without rank 1's contacts of the
    shared region in the columns 32 and 33: the nodes x = 32, 33 there stay on rank 1's list (rank 0's contacts reach
    them), with own sums that are now exactly zero"""
    b, wt, keys = cl.stencil(lay)
    y = b[:, 1]
    drop = (b[:, 0] >= CUT) & (b[:, 0] <= CUT + 1) & (y >= SHARED[0] - 2) & (y <= SHARED[1] + 2)
    return np.nonzero(~drop)[0]


def sub_layout(lay, sel):
    """the layout with the contacts `sel` only (same particles)"""
    out = dict(lay)
    out["cp"] = {k: v[sel] for k, v in lay["cp"].items()}
    out["name"] = lay["name"] + "/sub"
    return out


def three(empty=False, seed=22):
    L = cl._Layout("three_empty" if empty else "three", seed, "soft")
    for c in range(CUT - 8, CUT + (4 if empty else 8)):
        _column(L, c, 10, SHARED)
    return L.finish(dict(three=True, empty_rank=2 if empty else None))


BUILDERS = {"cut": cut, "three": three, "three_empty": lambda: three(True)}
NAMES = tuple(BUILDERS)
# (layout, cuts, zone_blocks) of every partitioned case
# (cl's layouts were not built around a cut: block 8 passes regimes_mu0 where few nodes see both sides, and misses the
# contacts of fringe and occupancy altogether -- their contacts next to cell 32 lie on one side.  MORE: further cuts that go
# through regimes_mu0 and fringe; no cut at a block boundary goes through occupancy, whose cells are a block apart)
MORE = [("regimes_mu0", (0, 7, NB), 1), ("fringe", (0, 11, NB), 1)]
CASES = [(n, TWO, 1) for n in cl.NAMES] + MORE + [("cut", TWO, 1), ("cut", TWO, 2), ("three", THREE, 1), ("three_empty", THREE, 1)]
_CACHE = {}


def layout(name):
    if name in cl.BUILDERS:
        return cl.layout(name)
    if name not in _CACHE:
        _CACHE[name] = BUILDERS[name]()
    return _CACHE[name]


def case_id(case):
    name, cuts, z = case
    at = "" if tuple(cuts) in (TWO, THREE) else "-at" + "_".join(str(c) for c in cuts[1:-1])
    return f"{name}-{len(cuts) - 1}r-z{z}{at}"
