"""The contact solve of the engine on the layouts of tests/contact_layouts.py against the float64 restatements of the same
module, contact by contact, node by node and body by body:

    set-up      CONTACT_VEL0 within the gather bound; the counts of nodes and contacts exact
    iteration   (max_newton_iterations = 1) GRID_DIR within its bound at every DoF and exactly zero where the
                restatement has none, the DoF count, sum |Dir|^2, E(0) and E(alpha) within bound; the accepted step is one
                the restatement accepts within the bound and every larger candidate one it rejects within the bound; the
                grid velocity after the step, CONTACT_VEL and the impulses of every body within bound
    iteration 2 twin deterministic engines, one and two iterations: the first row of the contact log bit-equal, and the
                second direction within bound of the restatement taken from the first engine's final grid velocity
    deep        MPM_CT_RELAX = 40: the step lies beyond the first pass of four candidates, the same consistency check
    exact       the exact line search ends where the restated dE/dalpha vanishes within its bound (or at alpha = 1 with
                dE(1) < 0)
Each phase is judged on the engine's own inputs of that phase (the grid after UpdateGrid, the direction it computed)."""
import numpy as np
import pytest

from tests import contact_layouts as cl
from tests import harness as hs
from tests import transfer_layouts as tl

pytestmark = pytest.mark.gpu

CANDIDATES = [2.0 ** -j for j in range(28)]


def _create(lay, deterministic=False, env=None):
    """the layout's mesh in a finalised engine -> (engine, API slot of every particle of the layout)"""
    from drake_amd import ARR as A, GpuMpm
    with hs.environ(env):
        mat = GpuMpm.default_material()
        mat.gravity_axis = lay["gravity_axis"]
        g = GpuMpm(lay["bits"], mat)
    g.set_deterministic(deterministic)
    for rest, vel, idx in lay["cloths"]:
        g.add_qr_cloth(rest, vel, idx)
    g.finalize()
    k, d, dt, mu = cl.params32(lay["params"])
    g.calc_fem_state_and_force(dt)
    g.gpu_sync()
    pids = g.download(A.PIDS)
    slot_of = np.empty_like(pids)
    slot_of[pids] = np.arange(len(pids))
    return g, slot_of, pids


def _upload_layout(g, lay, pids):
    g.upload_particle_state(lay["pos"][pids], lay["vel"][pids], lay["C"][pids], lay["vol"][pids], None)
    g.reallocate_external_bodies(lay["n_bodies"])


def _pre(g, lay, slot_of):
    """the inputs of the solve as the engine holds them, and the API slots of the layout's contact particles"""
    from drake_amd import ARR as A
    s = slot_of[lay["cp"]["particle"]]
    pre = dict(gm=g.download(A.GRID_MASSES), gv=g.download(A.GRID_MOMENTUM), gvs=g.download(A.GRID_V_STAR),
               vp=g.download(A.VELOCITIES)[s].astype(np.float64), mass_all=g.download(A.MASSES))
    pre["mass_c"] = pre["mass_all"][s].astype(np.float64)
    return pre, s


def _pairs(g, lay, s, sel=slice(None)):
    cp = lay["cp"]
    g.copy_contact_pairs(s[sel].astype(np.uint32), cp["body"][sel], cp["dist"][sel], cp["normal"][sel], cp["pos"][sel],
                         cp["rigid_v"][sel], cp["p_WB"][sel])


def _engine(lay, deterministic=False, env=None, before_pairs=None):
    """before_pairs(g): runs between mpm_create (under `env`) + Finalize and the upload of the state"""
    g, slot_of, pids = _create(lay, deterministic, env)
    if before_pairs:
        before_pairs(g)
    k, d, dt, mu = cl.params32(lay["params"])
    _upload_layout(g, lay, pids)
    g.rebuild_mapping(False)
    g.calc_fem_state_and_force(dt)
    g.particle_to_grid(dt)
    g.update_grid(-1)
    pre, s = _pre(g, lay, slot_of)
    _pairs(g, lay, s)
    return g, pre


def _outputs(g, rg):
    from drake_amd import ARR as A
    n = rg["contacts"]
    none = np.zeros((0, 3), np.float32)
    out = dict(rg=rg, cs=g.contact_stats(), D=g.download(A.GRID_DIR), gv1=g.download(A.GRID_MOMENTUM),
               vel0=g.download(A.CONTACT_VEL0) if n else none, vel=g.download(A.CONTACT_VEL) if n else none,
               log=g.contact_log(), stats=g.stats())
    out["tau"], out["f"] = g.external_body_force_to_host()
    return out


def _solve(g, lay, iters, exact=False):
    k, d, dt, mu = cl.params32(lay["params"])
    return _outputs(g, g.update_contact(dt, mu, k, d, exact_line_search=exact, max_newton_iterations=iters))


class _Checks:
    def __init__(self, tag):
        self.tag, self.fails = tag, []

    def __call__(self, field, err, bound):
        w = cl.margin(np.abs(np.asarray(err, np.float64)), np.asarray(bound, np.float64))
        hs.record(f"contact layouts: {self.tag} {field}", w)
        if not w <= 1.0:
            self.fails.append(f"{field}: {w:.3g} x the bound")

    def done(self):
        assert not self.fails, f"{self.tag}:\n" + "\n".join(self.fails)


def _alpha_consistent(ls, alpha, chk, what):
    """the accepted step is acceptable within the bound, every larger candidate rejected within the bound"""
    E0 = ls[0]
    for a in ls[1:]:
        slack = a["eE"] + E0["eE"]
        if a["alpha"] > alpha:
            chk.fails += [] if a["E"] - E0["E"] >= -slack else [f"{what}: candidate {a['alpha']} was acceptable"]
        elif a["alpha"] == alpha:
            chk.fails += [] if a["E"] - E0["E"] <= slack else [f"{what}: accepted {alpha} was not acceptable"]


def _iteration_checks(lay, pre, out, chk, relax=cl.RELAX, part=None):
    """part: `out` is what ONE RANK of a partitioned domain holds after the solve (tests/cut_layouts.py), `lay` and `pre`
    are the union's (every node's grid values from its owner).  dict(sel: the rank's contacts, in the order it was given
    them; list: the dense keys of the nodes it lists; received: the nodes that add a neighbour's sums (L_n + 1); D: the
    union's direction, every node from its owner (the line search's sums are global); gm, gv: the rank's own grid before
    the solve; gv1: the union's grid after it; f, tau: the impulses summed over the ranks, ranks: how many)"""
    P = cl.params32(lay["params"])
    gm, gv, gvs = pre["gm"], pre["gv"], pre["gvs"]
    b, wt, keys, T = cl.prepare(lay, P, gm, gv, gvs, pre["vp"], pre["mass_c"])
    cs = out["cs"]
    sel = slice(None) if part is None else part["sel"]
    nc = len(lay["cp"]["particle"][sel])
    assert out["stats"]["error_flags"] == 0, out["stats"]
    assert cs["contacts"] == nc and cs["iterations"] == 1, (cs, nc)
    # set-up
    vel0, e0 = cl.gather(wt, keys, gv, gm)
    chk("vel0", out["vel0"] - vel0[sel], e0[sel])
    dr = cl.direction(lay, P, wt, keys, pre["mass_c"], T, gm, gv, gvs, relax=relax,
                      received=None if part is None else part["received"])
    nodes = dr["nodes"]
    listed = np.ones(len(nodes), bool) if part is None else np.isin(nodes, part["list"])
    assert part is None or np.isin(part["list"], nodes).all()
    assert cs["nodes"] == listed.sum(), (cs["nodes"], int(listed.sum()))
    # direction
    D = out["D"].astype(np.float64)
    ok = dr["dof"] & ~dr["amb"] & listed
    chk("Dir", D[nodes][ok] - dr["D"][ok], dr["eD"][ok])
    off = ~dr["dof"] & ~dr["amb"] & listed
    assert not D[nodes][off].any(), f"{chk.tag}: a direction where the restatement has no DoF"
    rest = np.ones(len(D), bool)
    rest[nodes[listed]] = False
    assert not D[rest].any(), f"{chk.tag}: a direction off the node list"
    lo, hi = int((dr["dof"] & ~dr["amb"]).sum()), int(dr["dof"].sum() + dr["amb"].sum())
    assert lo <= cs["dofs"] <= hi, (cs["dofs"], lo, hi)
    if not dr["amb"].any():
        assert cs["dofs"] == lo, (cs["dofs"], lo)
        d = dr["D"] / relax
        chk("|Dir|^2", [cs["norm_dir_sq"] - dr["nd"]], [2 * (np.abs(d) * dr["eD"] / relax).sum() + cl.U32 * dr["nd"]])
    # line search on the engine's direction
    al = float(cs["alpha"])
    cands = [a for a in CANDIDATES if a >= al]
    Dls = D if part is None else np.asarray(part["D"], np.float64)
    ls = cl.line_search(lay, P, wt, keys, pre["mass_c"], T, gm, gv, gvs, Dls, nodes, [0.0] + cands)
    chk("E0", [cs["E0"] - ls[0]["E"]], [ls[0]["eE"]])
    chk("E(alpha)", [cs["energy"] - ls[-1]["E"]], [ls[-1]["eE"]])
    _alpha_consistent(ls, al, chk, "alpha")
    # the step on the grid: v - alpha D at the nodes that see contacts (m > 0), nothing elsewhere
    gm_own, gv_own = (gm, gv) if part is None else (part["gm"], part["gv"])
    v = gv_own.astype(np.float64).copy()
    live = np.zeros(len(v), bool)
    live[nodes[listed]] = gm_own[nodes[listed]] > 0
    want = v.copy()
    want[live] = v[live] - al * D[live]
    chk("grid v after the step", out["gv1"][live] - want[live], 2 * cl.U32 * (np.abs(want[live]) + al * np.abs(D[live])))
    assert np.array_equal(out["gv1"][~live], gv_own[~live])
    # contact velocities after the solve and the impulses of every body
    q = tl.fixed_quanta(pre["mass_all"])[1]   # (the momentum quantum 1 / DP::fix_p)
    imp = cl.impulses(lay, wt, keys, gm, gv, out["gv1"] if part is None else part["gv1"], pre["mass_c"], quantum=q)
    chk("contact vel", out["vel"] - imp["v"][sel], imp["ev"][sel])
    # (a partitioned domain: every rank's accumulator rounds once more, one quantum per rank)
    more = 0.0 if part is None else part["ranks"] * q
    f, tau = (out["f"], out["tau"]) if part is None else (part["f"], part["tau"])
    chk("F_f", f - imp["f"], imp["ef"] + more)
    chk("F_tau", tau - imp["tau"], imp["et"] + more)
    return dict(wt=wt, keys=keys, T=T, dr=dr, P=P, ls=ls)


@pytest.mark.parametrize("name", cl.NAMES)
def test_one_newton_iteration_per_node(name):
    from tests import helpers
    helpers.tag_default_engine(True)
    lay = cl.layout(name)
    g, pre = _engine(lay)
    out = _solve(g, lay, 1)
    g.destroy()
    chk = _Checks(name)
    _iteration_checks(lay, pre, out, chk)
    chk.done()


@pytest.mark.parametrize("name", ["regimes_soft", "regimes_config3", "bodies", "fringe", "occupancy"])
def test_second_iteration_from_the_first_ones_grid(name):
    """the lazy path (k_ct_tile reading v - alpha D, k_ct_node_dir adding it) and the inertia term m (v - v*)"""
    lay = cl.layout(name)
    ga, pre = _engine(lay, deterministic=True)
    a = _solve(ga, lay, 1)
    ga.destroy()
    gb, preb = _engine(lay, deterministic=True)
    b = _solve(gb, lay, 2)
    gb.destroy()
    assert b["cs"]["iterations"] == 2, b["cs"]
    assert np.array_equal(a["log"][0].view(np.uint32), b["log"][0].view(np.uint32)), (a["log"][0], b["log"][0])
    for k in ("gm", "gv", "gvs"):
        assert np.array_equal(pre[k], preb[k])
    P = cl.params32(lay["params"])
    gm, gvs, v1 = pre["gm"], pre["gvs"], a["gv1"]
    bb, wt, keys = cl.stencil(lay)
    cv, ecv = cl.gather(wt, keys, v1, gm)
    T = cl.contact_terms(lay, P, cv, pre["vp"], ecv)
    dr = cl.direction(lay, P, wt, keys, pre["mass_c"], T, gm, v1, gvs)
    chk = _Checks(f"{name} iteration 2")
    D = b["D"].astype(np.float64)
    ok = dr["dof"] & ~dr["amb"]
    chk("Dir", D[dr["nodes"]][ok] - dr["D"][ok], dr["eD"][ok])
    assert not D[dr["nodes"]][~dr["dof"] & ~dr["amb"]].any()
    assert np.abs(dr["o"][dr["mn"] > 0]).max() > 0          # (the inertia term is not zero here)
    chk.done()


def test_deep_backtracking_per_node():
    """MPM_CT_RELAX = 40: the Newton step overshoots, the accepted step lies beyond the first four candidates"""
    lay = cl.layout("regimes_soft")
    g, pre = _engine(lay, env={"MPM_CT_RELAX": "40"})
    out = _solve(g, lay, 1)
    g.destroy()
    assert out["cs"]["alpha"] < 1.0 / 8.0, out["cs"]
    chk = _Checks("regimes_soft relax 40")
    _iteration_checks(lay, pre, out, chk, relax=40.0)
    chk.done()


@pytest.mark.parametrize("name", ["regimes_soft", "bodies"])
def test_exact_line_search_ends_at_the_restated_root(name):
    lay = cl.layout(name)
    g, pre = _engine(lay)
    out = _solve(g, lay, 1, exact=True)
    g.destroy()
    P = cl.params32(lay["params"])
    gm, gv, gvs = pre["gm"], pre["gv"], pre["gvs"]
    b, wt, keys, T = cl.prepare(lay, P, gm, gv, gvs, pre["vp"], pre["mass_c"])
    dr = cl.direction(lay, P, wt, keys, pre["mass_c"], T, gm, gv, gvs)
    al = float(out["cs"]["alpha"])
    ls = cl.line_search(lay, P, wt, keys, pre["mass_c"], T, gm, gv, gvs, out["D"].astype(np.float64), dr["nodes"],
                        [al, 1.0], derivs=True, vp=pre["vp"])
    a, one = ls
    f_tol, x_tol = 1e-8, 1e-8 * cl.RELAX
    at_root = abs(a["dE"]) <= a["edE"] + f_tol + 2 * x_tol * abs(a["d2E"])
    at_end = al == 1.0 and one["dE"] < one["edE"]
    r = abs(a["dE"]) / (a["edE"] + f_tol + 2 * x_tol * abs(a["d2E"]))
    hs.record(f"contact layouts: {name} exact search dE(alpha)", r if not at_end else 0.0)
    assert at_root or at_end, (al, a, one)
