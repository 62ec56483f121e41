"""Per-body contact materials on the CPU: the restatement of tests/contact_materials.py with a uniform table is
contact_layouts' scalar restatement exactly; the table of the tests reaches what it is built for on the double oracle's
pre-solve grid; the nodes the direction check leaves out as ambiguous stay few; the binding exists."""
import numpy as np
import pytest

from tests import contact_layouts as cl
from tests import contact_materials as cm
from tests import test_contact_layouts as base

ALPHAS = [0.0] + [2.0 ** -j for j in range(6)]


@pytest.fixture(scope="module")
def scene():
    """the `bodies` layout in the double oracle: its pre-solve grid (independent of the contact parameters) and direction"""
    lay = cl.layout(cm.LAYOUT)
    o, pre, r = base.run_oracle(lay, np.float64)
    cp = lay["cp"]
    vp = np.asarray(o.vel, np.float64)[cp["particle"]]
    mass_c = lay["mass"][cp["particle"]].astype(np.float64)
    return dict(lay=lay, pre=pre, vp=vp, mass_c=mass_c, gD=np.asarray(o.g_D, np.float64))


def _same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), (what, k)


def test_uniform_table_is_the_scalar_restatement_exactly(scene):
    lay, (gm, gv, gvs), vp, mass_c = scene["lay"], scene["pre"], scene["vp"], scene["mass_c"]
    for pset in ("soft", "config3", "d0"):
        call = cl.params32(pset)
        # (deliberately other scalars behind a full table: nothing may be inherited)
        P = cm.params(lay, cm.uniform_table(call), call=cl.params32("damped")[:2] + (call[2], 0.125))
        for a, s in zip((P[0], P[1], P[3]), (call[0], call[1], call[3])):
            assert (a == s).all()
        b, wt, keys, T = cm.prepare(lay, P, gm, gv, gvs, vp, mass_c)
        b0, wt0, keys0, T0 = cl.prepare(lay, call, gm, gv, gvs, vp, mass_c)
        _same(T, T0, f"{pset}: contact terms (H, G, their bounds)")
        dr = cm.direction(lay, P, wt, keys, mass_c, T, gm, gv, gvs)
        dr0 = cl.direction(lay, call, wt0, keys0, mass_c, T0, gm, gv, gvs)
        _same(dr, dr0, f"{pset}: direction")
        ls = cm.line_search(lay, P, wt, keys, mass_c, T, gm, gv, gvs, scene["gD"], dr["nodes"], ALPHAS, derivs=True, vp=vp)
        ls0 = cl.line_search(lay, call, wt0, keys0, mass_c, T0, gm, gv, gvs, scene["gD"], dr0["nodes"], ALPHAS, derivs=True,
                             vp=vp)
        for x, y in zip(ls, ls0):
            assert x == y, (pset, x, y)


def test_resolution_is_a_select_field_by_field():
    call = cl.params32("soft")
    k, d, dt, mu = call
    body = np.arange(45)
    r = cm.resolve(cm.table(40), body, call)
    assert r.dtype == np.float32
    scal = np.array([mu, k, d], np.float32)
    for b in body:
        want = scal.copy()
        if b < 40:
            e = cm.TABLE[b % 7]
            want = np.where(e < 0, scal, e)
        assert np.array_equal(r[b].view(np.uint32), want.view(np.uint32)), b
    # a short table: the bodies beyond it inherit all three
    assert np.array_equal(cm.resolve(cm.table(40)[:10], body, call)[10:], np.tile(scal, (35, 1)))
    assert cm.resolve(np.zeros((0, 3)), body, call).shape == (45, 3)


def test_the_table_reaches_what_it_is_built_for(scene):
    lay, (gm, gv, gvs), vp, mass_c = scene["lay"], scene["pre"], scene["vp"], scene["mass_c"]
    P = cm.params(lay, cm.table(lay["n_bodies"]))
    b, wt, keys, T = cm.prepare(lay, P, gm, gv, gvs, vp, mass_c)
    entry = cm.entry_of_body(lay["n_bodies"])[lay["cp"]["body"]]
    live = np.bincount(entry[~T["sep"]], minlength=len(cm.TABLE))
    assert (live >= 20).all(), live
    # one cell (hence one segment of a tile) with contacts of at least three entries
    cell = keys[:, 0]
    per_cell = {}
    for c, e in zip(cell.tolist(), entry.tolist()):
        per_cell.setdefault(c, set()).add(e)
    assert max(len(s) for s in per_cell.values()) >= 3
    assert T["sep_margin"].min() > 10.0, T["sep_margin"].min()
    # both kinds of accumulators of k_ct_impulse see several entries
    assert len(set(cm.entry_of_body(40)[:32])) == 7 and len(set(cm.entry_of_body(40)[32:])) == 7
    # the condition that keeps the GPU test honest: few nodes are left out of the direction check
    dr = cm.direction(lay, P, wt, keys, mass_c, T, gm, gv, gvs)
    assert dr["amb"].sum() <= 0.05 * len(dr["nodes"]), (int(dr["amb"].sum()), len(dr["nodes"]))
    assert (dr["dof"] & ~dr["amb"]).sum() > 100
    # nodes whose contacts all resolve to one triple, for at least three of the triples (the locality test of the GPU)
    assert sum(len(n) > 0 for _, n in cm.uniform_nodes(P, keys)) >= 3


def test_the_restatement_tells_the_table_from_the_scalars(scene):
    """the table moves the restated direction by far more than its bound: a solve that ignored it would be seen"""
    lay, (gm, gv, gvs), vp, mass_c = scene["lay"], scene["pre"], scene["vp"], scene["mass_c"]
    P = cm.params(lay, cm.table(lay["n_bodies"]))
    b, wt, keys, T = cm.prepare(lay, P, gm, gv, gvs, vp, mass_c)
    dr = cm.direction(lay, P, wt, keys, mass_c, T, gm, gv, gvs)
    call = cl.params32(lay["params"])
    b0, wt0, keys0, T0 = cl.prepare(lay, call, gm, gv, gvs, vp, mass_c)
    dr0 = cl.direction(lay, call, wt0, keys0, mass_c, T0, gm, gv, gvs)
    ok = dr["dof"] & dr0["dof"] & ~dr["amb"]
    assert cl.margin(np.abs(dr["D"][ok] - dr0["D"][ok]), dr["eD"][ok]) > 100


def test_the_binding_exists():
    from drake_amd import capi
    assert "mpm_set_body_contact_materials" in capi.SYMBOLS and "mpm_get_body_contact_materials" in capi.SYMBOLS
    assert callable(getattr(capi.GpuMpm, "set_body_contact_materials"))
    assert callable(getattr(capi.GpuMpm, "body_contact_materials"))
    assert [f for f, _ in capi.ContactMaterial._fields_] == ["friction_mu", "stiffness", "damping"]
