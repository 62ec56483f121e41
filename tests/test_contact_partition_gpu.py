"""The contact solve of a partitioned domain on the layouts of tests/cut_layouts.py, per node against float64 across a cut.

A. one rank, the partitioned path forced (MPM_CT_FORCE_DIST=1, mpm_dist_init of a world of one, an identity all-reduce):
   the split direction kernels (k_ct_node_dir<1>, <2>), the two-phase k_ct_decide and the host-driven loops
   (newton_backtracking_host, newton_exact_host) against the plain paths of an engine set up in the same way without
   the switch (k_ct_node_dir<0>, the device-resident loops), to the bit -- with no neighbour nothing is added, so any
   difference is a defect of the mode split or of the host loop.
B. two and three ranks in one process (drake_amd.dist.LocalWorld), host-driven transport.  Every rank: substep_begin, the
   halo exchange, update_grid_from_sums, download of the pre-solve grid, copy_contact_pairs with the contacts of the
   particles it owns, update_contact.  mpm_update_contact blocks inside its callbacks until the neighbours arrive, so every
   rank's call runs in a thread of its own (ctypes releases the GIL); the exchange callback copies through the engines
   behind a threading.Barrier, the all-reduce callback sums the ranks' arrays in rank order in float64.  Every wait has
   a time limit: a rank that does not arrive is a failed callback and an error code on the others, never a hang.
   Per rank, on that rank's own downloaded inputs (test_contact_layouts_gpu._iteration_checks with `part`):
       before the solve   GRID_MASSES, the grid velocity and GRID_V_STAR bit-equal on the ranks of a cut at every node of
                          a zone block active on both; the union's grid takes every node from its owner
       counts             nodes = the restated list (own contacts' nodes + flagged zone nodes), DoFs the union's on every
                          rank (shared nodes once), contacts per rank the split's
       GRID_DIR           within the union's bound widened by one addition where a neighbour's sums arrive, exactly zero
                          where the restatement has no DoF and off the list, bit-equal between the ranks at shared nodes
       sums               |Dir|^2, E0, E(alpha) within the union's bounds, the contact log rows identical on every rank
       step               consistent with the restated energies; v - alpha D on the list, unchanged elsewhere, bit-equal
                          across ranks at shared nodes
       contacts           CONTACT_VEL0 / CONTACT_VEL per contact, the impulses summed over the ranks per body (+ one
                          accumulator quantum per rank)
   GRID_DIR is NOT compared to the bit with fl(own + neighbour's) of restated float sums: a rank's own sums depend on
   k_ct_tile's grouping (segments, subset sums, the butterfly), which no restatement here predicts to the bit, and the
   engine has no download of the exchanged (H, G) field.  What is checked instead: the direction -- a function of that
   field and of grid values that are bit-equal -- is bit-equal on both ranks at every shared node.
C. the team transport (mpm_team.h: k_team_zone_pack<3>, k_team_zone_add<3>, the rank-ordered line-search rows) on worlds of
   two and three ranks with pairs from colliders, two coupled substeps, against B's host-driven sequence on a twin world,
   to the bit."""
import threading
import time

import numpy as np
import pytest

from tests import contact_layouts as cl
from tests import cut_layouts as ct
from tests import harness as hs
from tests import test_contact_layouts_gpu as single
from tests import transfer_layouts as tl

pytestmark = pytest.mark.gpu

ERR_CAPACITY_FLAG = 2
MPM_ERR_CAPACITY = -4
SOLVE_S = {}          # part A's solve time per layout, in this session


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- A. one rank, the partitioned path forced ----------------------------------------------------------------------------
def _forced(g):
    g.dist_init(0, 1, [0, ct.NB], 1, 0, 0)
    g.dist_set_transport(lambda sl, sr, rl, rr, nbytes: None, lambda values: None, 64)


@pytest.mark.parametrize("iters,exact", [(1, False), (2, False), (1, True)], ids=["1", "2", "1-exact"])
@pytest.mark.parametrize("name", cl.NAMES)
def test_forced_partitioned_path_of_one_rank_equals_the_plain_engine(name, iters, exact):
    lay = cl.layout(name)
    # (the plain engine is partitioned in the same way, a world of one: mpm_dist_init re-sorts the particles into slot
    # space of its own, and ParticleToGrid groups its float sums by that order -- without it the two pre-solve grids
    # differ in the last bits, 2e-7 of the node masses, before any contact kernel has run)
    g, pre = single._engine(lay, deterministic=True, before_pairs=_forced)
    ref = single._solve(g, lay, iters, exact)
    g.destroy()
    g, pre2 = single._engine(lay, deterministic=True, env={"MPM_CT_FORCE_DIST": "1"}, before_pairs=_forced)
    t0 = time.perf_counter()
    got = single._solve(g, lay, iters, exact)
    SOLVE_S[name] = max(SOLVE_S.get(name, 0.0), time.perf_counter() - t0)
    print(f"forced partitioned solve {name} iters={iters} exact={exact}: {SOLVE_S[name]:.3f} s")
    g.destroy()
    for k in ("gm", "gv", "gvs"):
        assert np.array_equal(_bits(pre[k]), _bits(pre2[k])), k
    assert got["stats"]["error_flags"] == 0 and ref["stats"]["error_flags"] == 0
    assert got["rg"]["iterations"] == ref["rg"]["iterations"] == iters
    for k in ("D", "gv1", "vel0", "vel", "tau", "f"):
        assert np.array_equal(_bits(got[k]), _bits(ref[k])), (name, k, np.abs(got[k].astype(np.float64) - ref[k]).max())
    assert got["log"].shape == ref["log"].shape and got["log"].shape[0] == iters
    # (rows: residual, evaluations, E(alpha), alpha, E(0), |Dir|^2, DoFs, 0)
    assert np.array_equal(_bits(got["log"]), _bits(ref["log"])), (name, got["log"], ref["log"])
    assert got["cs"]["dofs"] == ref["cs"]["dofs"] and got["cs"]["nodes"] == ref["cs"]["nodes"]
    assert got["cs"]["contacts"] == ref["cs"]["contacts"] == len(lay["cp"]["particle"])


# ---- B. worlds of two and three ranks ------------------------------------------------------------------------------------
def _timeout(name):
    """50 times part A's solve of the layout in this session (the slowest of A's where A does not run the layout), 30 s at
    least"""
    t = SOLVE_S.get(name, max(SOLVE_S.values(), default=0.0))
    return max(30.0, 50.0 * t)


class _World:
    def __init__(self, lay, cuts, Z, zone_capacity=512):
        import torch
        from drake_amd.dist import LocalWorld
        self.lay, self.cuts, self.Z = lay, list(cuts), Z
        self.world = len(cuts) - 1
        made = [single._create(lay, deterministic=True) for _ in range(self.world)]
        self.engines = [m[0] for m in made]
        self.slot_of, self.pids = made[0][1], made[0][2]
        assert all(np.array_equal(m[2], self.pids) for m in made)
        # (a fixed cadence that never comes due: nothing migrates here)
        self.w = LocalWorld(self.engines, self.cuts, Z, 0, 0, capacity_blocks=512, migrate_every=1000, migrate_capacity=8192,
                            device=torch.device("cuda", 0))
        for g in self.engines:
            single._upload_layout(g, lay, self.pids)
        self.parts = ct.split(lay, cuts, Z)
        self.timeout = _timeout(lay["name"])
        self.bar = threading.Barrier(self.world)
        self.mail, self.red = {}, [None] * self.world
        self.sent = [[] for _ in range(self.world)]        # per rank and exchange: {neighbour: the buffer as sent}
        self.reduced = [[] for _ in range(self.world)]     # per rank and all-reduce: the global array handed back
        for r, g in enumerate(self.engines):
            g.dist_set_transport(*self._transport(r), zone_capacity)
        self.zone_capacity = zone_capacity

    def _transport(self, r):
        g, W = self.engines[r], self.world

        def exchange(sl, sr, rl, rr, nbytes):
            sent = {}
            for n, src in ((r - 1, sl), (r + 1, sr)):
                if 0 <= n < W:
                    buf = np.empty(nbytes, np.uint8)
                    g.memcpy_d2h(buf.ctypes.data, src, nbytes)
                    self.mail[(r, n)] = sent[n] = buf
            self.sent[r].append(sent)
            self.bar.wait(self.timeout)
            for n, dst in ((r - 1, rl), (r + 1, rr)):
                if 0 <= n < W:
                    buf = self.mail[(n, r)]
                    assert len(buf) == nbytes
                    g.memcpy_h2d(dst, buf.ctypes.data, nbytes)
            self.bar.wait(self.timeout)      # (nobody packs the next exchange before everybody has read this one)

        def allreduce(values):
            self.red[r] = values.copy()
            self.bar.wait(self.timeout)
            tot = np.zeros_like(values)
            for q in range(W):               # rank order, float64
                tot += self.red[q]
            self.bar.wait(self.timeout)
            values[:] = tot
            self.reduced[r].append(tot)

        return exchange, allreduce

    def begin(self):
        """one substep up to the grid update on every rank, the halo exchange between; -> per rank its pre-solve state"""
        import torch
        k, d, dt, mu = cl.params32(self.lay["params"])
        w = self.w
        with torch.cuda.stream(w.stream):
            for c in w.chains:
                c.e.substep_begin(dt)
            for c in w.chains:
                for lo, hi, shift, n in c._zones():
                    c.e.halo_pack(lo, hi, shift, c.send[n].data_ptr(), c.cap)
            w._move(lambda c, n: c.send[n], lambda c: c.recv)
            for c in w.chains:
                for n in c.recv:
                    c.e.halo_add(c.recv[n].data_ptr(), c.cap)
                c.e.update_grid_from_sums(-1)
        w.stream.synchronize()
        self.pre, self.roles, self.act = [], [], []
        for g in self.engines:
            g.gpu_sync()
            assert g.stats()["error_flags"] == 0, g.stats()
            pre, s = single._pre(g, self.lay, self.slot_of)
            self.pre.append(pre)
            self.s = s
            self.roles.append(g.dist_roles())
            self.act.append(g.resort_table("ACT_BLOCK").astype(np.int64))
        return self.pre

    def check_roles(self, sel_all=None):
        """every contact's particle is owned by exactly the rank the split gives it to"""
        for p, roles in zip(self.parts, self.roles):
            mine = np.nonzero(roles[self.s] == 1)[0]
            assert np.array_equal(mine, p["sel"]), (p["rank"], len(mine), len(p["sel"]))

    def refresh(self):
        """the grid as it stands (after a solve) as the next solve's input"""
        for r, g in enumerate(self.engines):
            g.reallocate_external_bodies(self.lay["n_bodies"])      # (the impulse accumulators start from zero)
            self.pre[r], _ = single._pre(g, self.lay, self.slot_of)

    def pairs(self, lay=None, parts=None):
        lay, parts = lay or self.lay, parts or self.parts
        s = self.slot_of[lay["cp"]["particle"]]
        for g, p in zip(self.engines, parts):
            single._pairs(g, lay, s, p["sel"])

    def solve(self, iters, exact=False):
        """mpm_update_contact on every rank, each in its own thread -> per rank single._outputs, or raises the first error"""
        k, d, dt, mu = cl.params32(self.lay["params"])
        res, err = [None] * self.world, [None] * self.world

        def run(r):
            try:
                res[r] = self.engines[r].update_contact(dt, mu, k, d, exact_line_search=exact, max_newton_iterations=iters)
            except BaseException as ex:  # noqa: BLE001
                err[r] = ex
                self.bar.abort()         # (the others fail at once instead of waiting for their time limit)

        th = [threading.Thread(target=run, args=(r,)) for r in range(self.world)]
        t0 = time.perf_counter()
        for t in th:
            t.start()
        for t in th:
            t.join(self.timeout + 60.0)
        assert not any(t.is_alive() for t in th), "a rank's solve did not return"
        self.solve_s = time.perf_counter() - t0
        self.errors = err
        if any(e is not None for e in err):
            # (the rank that failed first broke the barrier for the others: theirs are failed callbacks)
            own = [e for e in err if e is not None and "callback" not in str(e)]
            print("errors per rank:", [None if e is None else str(e) for e in err])
            raise (own or [e for e in err if e is not None])[0]
        return [single._outputs(g, rg) for g, rg in zip(self.engines, res)]

    # -- the union, every node from its owner
    def owner_pick(self, per_rank):
        out = np.array(per_rank[0], copy=True)
        for p, a in zip(self.parts[1:], per_rank[1:]):
            out[p["owned"]] = a[p["owned"]]
        return out

    def union_pre(self, lay=None, parts=None):
        lay, parts = lay or self.lay, parts or self.parts
        s = self.slot_of[lay["cp"]["particle"]]
        pre = {k: self.owner_pick([q[k] for q in self.pre]) for k in ("gm", "gv", "gvs")}
        from drake_amd import ARR as A
        vel = [g.download(A.VELOCITIES) for g in self.engines]
        mass = [q["mass_all"] for q in self.pre]
        vp = np.zeros((len(s), 3))
        mass_all = np.array(mass[0], copy=True)
        for p, v, m, roles in zip(parts, vel, mass, self.roles):
            vp[p["sel"]] = v[s[p["sel"]]]
            mass_all[roles == 1] = m[roles == 1]
        pre.update(vp=vp, mass_all=mass_all, mass_c=mass_all[s].astype(np.float64))
        return pre

    def zone_nodes(self, r, s):
        """dense keys of the nodes of the zone blocks of ranks r and s that are active on both"""
        blo, bhi = self.parts[r]["zones"][s]
        both = np.intersect1d(self.act[r], self.act[s])
        bx = ct.node_x(both << 6) >> 2
        blk = both[(bx >= blo) & (bx <= bhi)]
        return (blk[:, None] * 64 + np.arange(64)[None]).reshape(-1)

    def destroy(self):
        for g in self.engines:
            g.destroy()


def _grid_before_the_solve(W):
    """bit-equal on the ranks of a cut at every node of a zone block active on both"""
    for p in W.parts:
        for s in p["zones"]:
            if s > p["rank"]:
                z = W.zone_nodes(p["rank"], s)
                assert len(z) > 0
                for k in ("gm", "gv", "gvs"):
                    a, b = W.pre[p["rank"]][k], W.pre[s][k]
                    assert np.array_equal(_bits(a[z]), _bits(b[z])), (W.lay["name"], k, p["rank"], s)


def _world_checks(W, outs, tag, lay=None, parts=None, relax=cl.RELAX):
    """one Newton iteration of the world against the union's restatement, rank by rank -> single._iteration_checks' dict"""
    lay, parts = lay or W.lay, parts or W.parts
    lists = ct.node_lists(parts, W.act)
    rec = ct.received(parts, lists)
    pre = W.union_pre(lay, parts)
    D_u = W.owner_pick([o["D"] for o in outs])
    gv1_u = W.owner_pick([o["gv1"] for o in outs])
    f = sum(o["f"].astype(np.float64) for o in outs)
    tau = sum(o["tau"].astype(np.float64) for o in outs)
    assert sum(o["cs"]["contacts"] for o in outs) == len(lay["cp"]["particle"])
    # every node that sees a contact is listed on its owner (else nobody counts its DoF): the engine's active blocks allow it
    union_nodes = np.unique(cl.stencil(lay)[2])
    for p, l in zip(parts, lists):
        assert np.isin(union_nodes[p["owned"][union_nodes]], l).all(), (tag, p["rank"])
    info = None
    for p, l, o in zip(parts, lists, outs):
        r = p["rank"]
        chk = single._Checks(f"{tag} rank {r}")
        part = dict(sel=p["sel"], list=l, received=rec, D=D_u, gm=W.pre[r]["gm"], gv=W.pre[r]["gv"], gv1=gv1_u, f=f, tau=tau,
                    ranks=W.world)
        info = single._iteration_checks(lay, pre, o, chk, relax=relax, part=part)
        chk.done()
    # across the ranks: the same bits at shared nodes, the same global numbers
    for p in parts:
        for s in p["zones"]:
            if s > p["rank"]:
                sh = np.intersect1d(lists[p["rank"]], lists[s])
                assert len(sh) > 0 or not len(rec)
                for k in ("D", "gv1"):
                    a, b = outs[p["rank"]][k], outs[s][k]
                    assert np.array_equal(_bits(a[sh]), _bits(b[sh])), (tag, k, "differs between ranks", p["rank"], s)
    for o in outs[1:]:
        assert np.array_equal(_bits(o["log"]), _bits(outs[0]["log"])), (tag, o["log"], outs[0]["log"])
        for k in ("dofs", "alpha", "E0", "energy", "norm_dir_sq", "iterations"):
            assert o["cs"][k] == outs[0]["cs"][k], (tag, k)
    return dict(info, lists=lists, received=rec, pre=pre, D=D_u, gv1=gv1_u)


@pytest.fixture(scope="module")
def worlds():
    """the worlds of SECOND after one iteration, shared by the tests that only read them; destroyed with the module"""
    cache = {}
    yield cache
    for W, _ in cache.values():
        W.destroy()
    cache.clear()


# the cases whose world of one iteration is kept for the tests that follow
SECOND = [c for c in ct.CASES if c in (("cut", ct.TWO, 1), ("regimes_soft", ct.TWO, 1), ("bodies", ct.TWO, 1))]


def _first_iteration(case, cache):
    """the world of a case after one iteration of one solve (kept in `cache`: the twin of the second-iteration test;
    nothing that takes it from there changes it)"""
    key = ct.case_id(case)
    if key not in cache:
        name, cuts, Z = case
        W = _World(ct.layout(name), cuts, Z)
        W.begin()
        W.check_roles()
        W.pairs()
        outs = W.solve(1)
        cache[key] = (W, outs)
    return cache[key]


@pytest.mark.parametrize("case", ct.CASES, ids=[ct.case_id(c) for c in ct.CASES])
def test_one_newton_iteration_of_the_world_per_node(case, worlds):
    from tests import helpers
    helpers.tag_default_engine(False)
    name, cuts, Z = case
    W, outs = _first_iteration(case, worlds if case in SECOND else {})
    lay = W.lay
    print(f"world solve {ct.case_id(case)}: {W.solve_s:.3f} s (time limit per wait {W.timeout:.0f} s)")
    _grid_before_the_solve(W)
    info = _world_checks(W, outs, ct.case_id(case))
    lists = info["lists"]
    # the flag exchange ran once, then one exchange of sums; the all-reduce of the pair counts, then the line search's;
    # every rank entered each and was handed the same numbers
    assert all(len(s) == 2 for s in W.sent) and all(len(a) == 2 for a in W.reduced), ([len(s) for s in W.sent],)
    assert W.reduced[0][0].tolist() == [float(len(lay["cp"]["particle"]))]
    for a in W.reduced[1:]:
        assert all(np.array_equal(x, y) for x, y in zip(a, W.reduced[0]))
    if name == "bodies":        # ids beyond k_ct_impulse's LDS accumulators on both ranks
        for p in W.parts:
            assert (lay["cp"]["body"][p["sel"]] >= 32).sum() >= 16
    if name == "cut":
        # a. nodes listed through the flags alone, owned (their DoFs are counted here) and not
        for p, l in zip(W.parts, lists):
            only = np.setdiff1d(l, p["flags"])
            assert len(only) >= 20 and (~p["owned"][only]).sum() >= 10
        # c. a zone block active on the sender and not on the receiver: listed in the buffer, dropped, no error
        for s, r in ((0, 1), (1, 0)):
            blo, bhi = W.parts[s]["zones"][r]
            bx = ct.node_x(W.act[s] << 6) >> 2
            foreign = np.setdiff1d(W.act[s][(bx >= blo) & (bx <= bhi)], W.act[r])
            assert len(foreign) >= 1, (s, r)
            n, ids = _buffer_ids(W.sent[s][0][r], W.zone_capacity)
            assert np.isin(foreign, ids[:n]).all()
        # e. the DoF that exists only after the add is one on both ranks
        common, per, un = ct._e_nodes(lay, W.parts, (info["pre"]["gm"],))
        at = np.searchsorted(un["nodes"], common)
        below = np.ones(len(common), bool)
        for hF, gF, eHF, eGF in per:
            below &= (hF + eHF < cl.THRESH) & (gF + eGF < cl.THRESH)
        e_nodes = common[below & un["dof"][at] & ~un["amb"][at] & (info["pre"]["gm"][common] > 0)]
        assert len(e_nodes) >= 1
        for o in outs:
            assert np.abs(o["D"][e_nodes]).max(axis=1).min() > 0
    if W.lay["claims"].get("empty_rank") is not None:
        r = W.lay["claims"]["empty_rank"]
        assert outs[r]["rg"]["contacts"] == 0 and outs[r]["cs"]["nodes"] == len(lists[r]) > 0
        assert (W.parts[r]["owned"][lists[r]] & (np.abs(outs[r]["D"][lists[r]]).max(axis=1) > 0)).sum() >= 20
    if case not in SECOND:
        W.destroy()


def _buffer_ids(buf, cap):
    """a zone exchange buffer (mpm_zone_buffer.h) -> (count word, the ids listed)"""
    words = buf.view(np.uint32)
    return int(words[0]), words[4:4 + min(int(words[0]), cap)].astype(np.int64)


def _buffer_cells(buf, cap, nv=3):
    """-> (cap, 64, nv, 4) float32: the entries' vectors"""
    off = (((4 + cap) * 4 + 15) // 16) * 16
    return buf[off:off + cap * 64 * nv * 16].view(np.float32).reshape(cap, 64, nv, 4)


@pytest.mark.parametrize("case", SECOND, ids=[ct.case_id(c) for c in SECOND])
def test_second_iteration_of_the_world_from_the_first_ones_grid(case, worlds):
    """twin worlds of one and two iterations: the lazy v - alpha D must have reached the zone nodes on both ranks before
    the second direction is formed"""
    name, cuts, Z = case
    Wa, a = _first_iteration(case, worlds)
    Wb = _World(ct.layout(name), cuts, Z)
    Wb.begin()
    Wb.pairs()
    b = Wb.solve(2)
    lay = Wa.lay
    for r in range(Wa.world):
        assert b[r]["cs"]["iterations"] == 2
        assert np.array_equal(_bits(a[r]["log"][0]), _bits(b[r]["log"][0])), (a[r]["log"][0], b[r]["log"][0])
        for k in ("gm", "gv", "gvs"):
            assert np.array_equal(_bits(Wa.pre[r][k]), _bits(Wb.pre[r][k]))
        assert np.array_equal(_bits(b[r]["log"]), _bits(b[0]["log"]))
    lists = ct.node_lists(Wa.parts, Wa.act)
    rec = ct.received(Wa.parts, lists)
    pre = Wa.union_pre()
    P = cl.params32(lay["params"])
    v1 = Wa.owner_pick([o["gv1"] for o in a])
    bb, wt, keys = cl.stencil(lay)
    cv, ecv = cl.gather(wt, keys, v1, pre["gm"])
    T = cl.contact_terms(lay, P, cv, pre["vp"], ecv)
    dr = cl.direction(lay, P, wt, keys, pre["mass_c"], T, pre["gm"], v1, pre["gvs"], received=rec)
    assert np.abs(dr["o"][dr["mn"] > 0]).max() > 0
    for p, l, o in zip(Wa.parts, lists, b):
        chk = single._Checks(f"{ct.case_id(case)} iteration 2 rank {p['rank']}")
        D = o["D"].astype(np.float64)
        listed = np.isin(dr["nodes"], l)
        ok = dr["dof"] & ~dr["amb"] & listed
        chk("Dir", D[dr["nodes"]][ok] - dr["D"][ok], dr["eD"][ok])
        assert not D[dr["nodes"]][~dr["dof"] & ~dr["amb"] & listed].any()
        chk.done()
    for p in Wa.parts:
        for s in p["zones"]:
            if s > p["rank"]:
                sh = np.intersect1d(lists[p["rank"]], lists[s])
                for k in ("D", "gv1"):
                    assert np.array_equal(_bits(b[p["rank"]][k][sh]), _bits(b[s][k][sh])), (k, p["rank"], s)
    Wb.destroy()


def test_second_solve_with_other_pairs_through_the_same_engines():
    """d: after a first solve, a second one whose pairs leave rank 1 without own sums at nodes where it had some -- mode 1
    writes the zeros (the exchanged field still holds the flags, and the first solve's sums before them)"""
    case = ("cut", ct.TWO, 1)
    W, first = _first_iteration(case, {})       # (a world of its own: this test goes on with its engines)
    lay2 = ct.sub_layout(W.lay, W.lay["second_pairs"])
    parts2 = ct.split(lay2, ct.TWO, 1)
    W.refresh()
    W.pairs(lay2, parts2)
    n_ex = [len(s) for s in W.sent]
    outs = W.solve(1)
    assert [len(s) for s in W.sent] == [n + 2 for n in n_ex]
    info = _world_checks(W, outs, "cut second solve", lay2, parts2)
    own1 = parts2[1]["flags"]
    zero_own = np.setdiff1d(info["lists"][1], own1)
    had = np.intersect1d(zero_own, W.parts[1]["flags"])
    assert len(had) >= 20 and (np.abs(outs[1]["D"][had]).max(axis=1) > 0).sum() >= 10
    W.destroy()


def test_exact_line_search_of_the_world_ends_at_the_restated_root():
    case = ("cut", ct.TWO, 1)
    name, cuts, Z = case
    W = _World(ct.layout(name), cuts, Z)
    W.begin()
    W.pairs()
    outs = W.solve(1, exact=True)
    lay = W.lay
    lists = ct.node_lists(W.parts, W.act)
    pre = W.union_pre()
    P = cl.params32(lay["params"])
    gm, gv, gvs = pre["gm"], pre["gv"], pre["gvs"]
    b, wt, keys, T = cl.prepare(lay, P, gm, gv, gvs, pre["vp"], pre["mass_c"])
    dr = cl.direction(lay, P, wt, keys, pre["mass_c"], T, gm, gv, gvs, received=ct.received(W.parts, lists))
    al = float(outs[0]["cs"]["alpha"])
    assert all(float(o["cs"]["alpha"]) == al for o in outs) and 0.0 < al <= 1.0
    D_u = W.owner_pick([o["D"] for o in outs]).astype(np.float64)
    a, one = cl.line_search(lay, P, wt, keys, pre["mass_c"], T, gm, gv, gvs, D_u, dr["nodes"], [al, 1.0], derivs=True,
                            vp=pre["vp"])
    f_tol, x_tol = 1e-8, 1e-8 * cl.RELAX
    at_root = abs(a["dE"]) <= a["edE"] + f_tol + 2 * x_tol * abs(a["d2E"])
    at_end = al == 1.0 and one["dE"] < one["edE"]
    r = abs(a["dE"]) / (a["edE"] + f_tol + 2 * x_tol * abs(a["d2E"]))
    hs.record("contact partition: cut exact search dE(alpha)", r if not at_end else 0.0)
    assert at_root or at_end, (al, a, one)
    W.destroy()


def test_zone_capacity_one_block_short_is_an_error_code():
    """the buffers of the contact solve's exchange one block too small for the fuller zone: MPM_ERR_CAPACITY or the capacity
    flag, the entries that fit are valid (the flag exchange: 1 at the sender's flagged nodes, 0 elsewhere), nothing hangs.
    (Words behind a buffer are not checked: the buffers are the engine's own, exactly as large as the capacity says.)"""
    from drake_amd import MpmError
    lay = ct.layout("cut")
    probe = _World(lay, ct.TWO, 1)
    probe.begin()
    need = []
    for s, r in ((0, 1), (1, 0)):
        blo, bhi = probe.parts[s]["zones"][r]
        bx = ct.node_x(probe.act[s] << 6) >> 2
        need.append(int(((bx >= blo) & (bx <= bhi)).sum()))
    probe.destroy()
    cap = max(need) - 1
    assert cap >= 1
    W = _World(lay, ct.TWO, 1, zone_capacity=cap)
    W.begin()
    W.pairs()
    raised = None
    try:
        W.solve(1)
    except MpmError as ex:
        raised = ex
    assert all(e is None or isinstance(e, MpmError) for e in W.errors), W.errors
    flags = [g.stats()["error_flags"] for g in W.engines]
    assert (raised is not None and raised.code == MPM_ERR_CAPACITY) or any(f & ERR_CAPACITY_FLAG for f in flags), (raised, flags)
    for s, r in ((0, 1), (1, 0)):
        buf = W.sent[s][0][r]
        n, ids = _buffer_ids(buf, cap)
        over = need[s] > cap
        assert n == need[s] and len(ids) == min(need[s], cap), (n, need[s], cap)
        # the sender whose zone does not fit reports it, the other one does not
        assert bool(flags[s] & ERR_CAPACITY_FLAG) == over, (s, flags, need, cap)
        blo, bhi = W.parts[s]["zones"][r]
        bx = ct.node_x(ids << 6) >> 2
        assert len(set(ids.tolist())) == len(ids) and np.isin(ids, W.act[s]).all() and ((bx >= blo) & (bx <= bhi)).all()
        cells = _buffer_cells(buf, cap)[:len(ids)]
        want = np.isin((ids[:, None] * 64 + np.arange(64)[None]), W.parts[s]["flags"]).astype(np.float32)
        assert np.array_equal(cells[:, :, 0, 0], want)
        assert not cells[:, :, 0, 1:].any() and not cells[:, :, 1:].any()
    W.destroy()


# ---- C. the team transport ----------------------------------------------------------------------------------------------
def _colliders():
    """a floor through the shared region of `cut` and `three` and one tilted half-space (its normal leans 0.3 rad towards
    +x) below it: both reach particles on every side of the cuts"""
    from drake_amd import Collider
    c, s = float(np.cos(0.3)), float(np.sin(0.3))
    R = (c, 0.0, s, 0.0, 1.0, 0.0, -s, 0.0, c)          # row-major R_WB: z_B = (s, 0, c) in the world
    return [Collider(0, body=0, p_WB=(0.5, 0.5, 23.0 / 64)),
            Collider(0, body=1, p_WB=(0.5, 0.5, 21.5 / 64), R_WB=R, v=(0.05, 0.0, 0.1))]


def _pair_layout(W, pairs):
    """the pairs the ranks generated (mpm_download_contact_pairs, rank by rank) as a layout of tests/cut_layouts.py"""
    cat = [np.concatenate([p[k] for p in pairs]) for k in range(7)]
    cp = dict(particle=W.pids[cat[0]].astype(np.uint32), body=cat[1], dist=cat[2], normal=cat[3], pos=cat[4], rigid_v=cat[5],
              p_WB=cat[6])
    return dict(W.lay, cp=cp, name=W.lay["name"] + "/colliders")


def _after(g, res=None):
    from drake_amd import ARR as A
    g._n_contacts = None          # (the count of the world's call is on the device: download_contact_pairs reads it back)
    return dict(D=g.download(A.GRID_DIR), gv1=g.download(A.GRID_MOMENTUM), log=g.contact_log(), cs=g.contact_stats(),
                pairs=g.download_contact_pairs(), res=res)


@pytest.mark.parametrize("case", [("cut", ct.TWO, 1), ("three", ct.THREE, 1)], ids=["cut-2r", "three-3r"])
def test_team_transport_equals_the_host_driven_one_to_the_bit(case):
    """LocalWorld.enable_team + coupled_substeps(1, max_newton_iterations=1), twice (the two gates: the parity of the team's
    slots alternates), against a twin world from the same colliders that runs B's host-driven sequence with
    generate_contact_pairs and GridToParticle behind the solve.  Both add own + neighbour's sums at a node and sum the
    line-search rows in rank order: rank by rank the pairs, GRID_DIR, the first row of the contact log, the DoF count and
    the grid after the step are the same bits.  The host-driven twin's first substep is held to B's float64 bounds through
    the pairs it generated (mpm_download_contact_pairs), so the team world is too."""
    name, cuts, Z = case
    lay = dict(ct.layout(name), n_bodies=2)
    k, d, dt, mu = cl.params32(lay["params"])
    cols = _colliders()
    Wt, Wh = _World(lay, cuts, Z), _World(lay, cuts, Z)
    Wt.w.enable_team(512)
    for sub in range(2):
        res = Wt.w.coupled_substeps(1, dt, cols, mu, k, d, max_newton_iterations=1)
        Wt.w.sync()
        team = [_after(g, r[0]) for g, r in zip(Wt.engines, res)]
        Wh.begin()
        counts = [g.generate_contact_pairs(cols) for g in Wh.engines]
        pairs = [g.download_contact_pairs() for g in Wh.engines]
        outs = Wh.solve(1)
        assert all(n >= 50 for n in counts), counts            # every rank generates pairs
        lay_c = _pair_layout(Wh, pairs)
        parts_c = ct.split(lay_c, cuts, Z)
        assert [len(p["sel"]) for p in parts_c] == counts      # ... of the particles it owns
        assert len(set(lay_c["cp"]["body"].tolist())) == 2
        lists = ct.node_lists(parts_c, Wh.act)
        assert len(ct.received(parts_c, lists)) >= 50
        if sub == 0:
            _world_checks(Wh, outs, f"{name} colliders host-driven", lay_c, parts_c)
        for r, (t, h) in enumerate(zip(team, outs)):
            what = (name, "substep", sub, "rank", r)
            assert t["res"]["contacts"] == counts[r] and t["res"]["iterations"] == 1, (what, t["res"], counts)
            for a, b in zip(t["pairs"], pairs[r]):
                assert np.array_equal(a, b), what
            assert t["cs"]["dofs"] == h["cs"]["dofs"] and t["cs"]["dofs"] > 0, what
            assert np.array_equal(_bits(t["log"][0]), _bits(h["log"][0])), (what, t["log"][0], h["log"][0])
            assert np.array_equal(_bits(t["D"]), _bits(h["D"])), (what, "GRID_DIR")
            assert np.array_equal(_bits(t["gv1"][lists[r]]), _bits(h["gv1"][lists[r]])), (what, "grid after the step")
        for g in Wh.engines:          # (behind the checks: they read the particle velocities the solve started from)
            g.grid_to_particle(dt)
    for W in (Wt, Wh):
        for g in W.engines:
            assert g.stats()["error_flags"] == 0
        W.destroy()
