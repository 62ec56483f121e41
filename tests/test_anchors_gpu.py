"""Anchors -- springs and cords from cloth vertices to rigid bodies (mpm_set_anchors) -- on the engine.

 1. mpm_anchor_forces per vertex against the float64 restatement of tests/anchors.py on every scene x state, within the
    bound counted in mpm_anchors.h, 2^-24 ((18 + n_i) sum S + sum (k |y| + c |v_Q|)); the points of mpm_anchor_state
    within one float ulp per component.  The clocks are nonzero: two substeps run first.
 2. MPM_ARR_FORCES of an engine with anchors is a twin's without plus mpm_anchor_forces, within one rounding of the sum.
 3. The reaction: after one substep every body's accumulators moved by -dt sum f and sum (y - p_WB) x (-dt f), formed in
    float64 from mpm_anchor_forces and the points downloaded just before, within n_b quanta (times the longest arm for
    the torque; plus 4 x 2^-53 of the gross torque for the cross product's own double roundings) and one float rounding
    of the reported sum.  The table has one anchor per vertex, so that a vertex's force is one anchor's force.  The body
    beyond the accumulators' count gets nothing and its vertices feel the force.  mpm_substep, mpm_run_substeps(1) and
    the phase calls leave the same bits.
 4. Energy and lengths against float64, with the bound of links.energy64.
 5. Anchors that do nothing (k = c = 0; slack cords; the degenerate spring) leave forces, state and accumulators
    bit-identical to an engine that never called mpm_set_anchors; clearing the table restores that engine's launches.
 6. Particle order: the forces and one substep's accumulators are the same bits after a forced re-sort.
 7. Clocks: with anchors and no pins the clock advances with every substep; with pins on the same body, once.
 8. A cord stops a fall.   9. Weight at rest, against a pinned twin.
10. Scheduling through re-sorts, and the coupled path.   11. Refusals."""
import functools

import numpy as np
import pytest

from tests import anchors as an
from tests import harness as hs
from tests import links as lk
from tests import transfer_layouts as tl

pytestmark = pytest.mark.gpu

U = an.U
DT = 1e-5          # a substep far inside every scene's stability guard
CASES = [(s, st) for s in an.SCENES for st in an.STATES]


_engine = functools.partial(hs.engine, bodies=an.N_BODIES)
_state = functools.partial(hs.state, bodies=True)


def _motions(motions):
    from drake_amd import BodyMotion
    return [BodyMotion(b, m[0], m[1].ravel(), m[2], m[3]) for b, m in motions.items()]


def _null(anchors):
    out = anchors.copy()
    out["stiffness"] = out["damping"] = 0.0
    return out


def _scene_engine(name, anchors=None, clock=True, material=None):
    """the scene's engine, zero gravity, its bodies' motions set and -- with `clock` -- their clocks at an.CLOCK: two
    substeps of an.CLOCK_DT with a table that does nothing, which launches the clock kernel and leaves the cloth alone"""
    cloths, table, motions, X = an.scene(name)
    anchors = table if anchors is None else anchors
    g = _engine(cloths, material=dict(gravity=0.0, **(material or {})))
    g.set_body_motions(_motions(motions))
    if clock:
        g.set_anchors(_null(anchors))
        assert g.anchors_max_stable_dt() == np.inf
        g.run_substeps(2, an.CLOCK_DT, -1)
    g.set_anchors(anchors)
    return g, anchors, motions, X


# ---- 1 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,st", CASES)
def test_forces_against_float64(name, st):
    g, anchors, motions, X = _scene_engine(name)
    assert np.array_equal(g.get_anchors(), anchors)
    x0, v0 = an.state(st, name, X)
    hs.upload(g, x0, v0)
    f = g.anchor_forces()
    ref, bound, y32, _ = an.vertex_forces64(anchors, x0, v0, motions, an.CLOCK)
    w = lk.margin(f - ref, bound)
    print(f"anchor forces: {name} {st}: {w:.3g} of the bound, largest force {np.abs(f).max():.3g}")
    hs.record(f"anchor forces: {name} {st}", w)
    assert w <= 1.0, w
    anchored = np.zeros(len(X), bool)
    anchored[anchors["vertex"]] = True
    assert not f[~anchored].any()
    assert f.any() or (name == "hung" and st == "rest")          # (hung at rest: l == L exactly, the cords do not act)
    y64, _, _, _ = an.points(anchors, motions, an.CLOCK)
    point = g.anchor_state()["point"]
    ulp = np.spacing(np.abs(y64).astype(np.float32)).astype(np.float64)
    wp = float((np.abs(point.astype(np.float64) - y64) / ulp).max())
    print(f"anchor points: {name} {st}: {wp:.3g} ulp")
    hs.record(f"anchor points: {name} {st}", wp)
    assert wp <= 1.0, wp
    if name == "mixed":
        assert not f[an.DEGENERATE_VERTEX].any()                 # l2 < 1e-30 with L > 0: an exact zero
    assert g.stats()["error_flags"] == 0
    g.destroy()


# ---- 2 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(an.SCENES))
def test_total_forces_include_anchors(name):
    A = hs.ARR()
    g, anchors, motions, X = _scene_engine(name, clock=False)     # (both engines fresh: the same F, the clocks at zero)
    twin = _engine(an.scene(name)[0], material=dict(gravity=0.0))
    x0, v0 = an.state("random", name, X)
    out = []
    for e in (g, twin):
        hs.upload(e, x0, v0)
        e.rebuild_mapping(False)
        e.calc_fem_state_and_force(DT)
        out.append(hs.vertices(e, A.FORCES))
    fa = g.anchor_forces()
    assert fa.any() and out[1].any()
    tot = out[1].astype(np.float64) + fa.astype(np.float64)
    err = np.abs(out[0].astype(np.float64) - tot)
    w = float((err / np.maximum(U * np.abs(out[0]).astype(np.float64), 1e-300))[err > 0].max()) if (err > 0).any() else 0.0
    print(f"total forces: {name}: {w:.3g} of one rounding of the sum")
    hs.record(f"anchors: total forces {name}", w)
    assert w <= 1.0, w
    assert not twin.anchor_forces().any() and twin.anchors_max_stable_dt() == np.inf and len(twin.get_anchors()) == 0
    for e in (g, twin):
        assert e.stats()["error_flags"] == 0
        e.destroy()


# ---- 3 -------------------------------------------------------------------------------------------------------------
def test_reaction():
    table = an.one_per_vertex(an.scene("mixed")[1])
    assert {an.BODY_FAR, an.BODY_NONE} <= set(table["body"].tolist())
    runs = (lambda g: g.substep(DT, -1), lambda g: g.run_substeps(1, DT, -1), lambda g: hs.phases(g, DT))
    states = []
    for k, run in enumerate(runs):
        g, anchors, motions, X = _scene_engine("mixed", anchors=table)
        assert DT <= g.anchors_max_stable_dt()
        x0, v0 = an.state("random", "mixed", X)
        hs.upload(g, x0, v0)
        f = g.anchor_forces().astype(np.float64)
        st = g.anchor_state()
        y, q = st["point"].astype(np.float64), st["impulse_quantum"]
        tau0, f0 = g.external_body_force_to_host()
        assert not tau0.any() and not f0.any()                    # (the clock substeps' anchors did nothing)
        run(g)
        g.gpu_sync()
        assert g.stats()["error_flags"] == 0
        tau1, f1 = g.external_body_force_to_host()
        states.append(_state(g))
        if k:
            continue
        assert q > 0
        dt = float(np.float32(DT))
        worst = 0.0
        for b in range(an.N_BODIES):
            sel = anchors["body"] == b
            n = int(sel.sum())
            l = -dt * f[anchors["vertex"][sel]]
            arm = y[sel] - motions[b][0].astype(np.float64) if n else np.zeros((0, 3))
            want_f, want_tau = l.sum(axis=0), np.cross(arm, l).sum(axis=0)
            if not n:
                assert not f1[b].any() and not tau1[b].any()
                continue
            reach = float(np.linalg.norm(arm, axis=1).max())
            gross = float((np.linalg.norm(arm, axis=1) * np.linalg.norm(l, axis=1)).sum())
            tol_f = n * q + U * np.abs(f1[b]).max()
            tol_tau = n * q * reach + 4 * 2.0 ** -53 * gross + U * np.abs(tau1[b]).max()
            ef, et = float(np.abs(f1[b] - want_f).max()), float(np.abs(tau1[b] - want_tau).max())
            print(f"reaction on body {b}: {n} anchors, force {ef / tol_f:.3g}, torque {et / tol_tau:.3g} of the bound; "
                  f"|impulse| {np.abs(want_f).max():.3g}, quantum {q:.3g}")
            worst = max(worst, ef / tol_f, et / tol_tau)
            assert ef <= tol_f and et <= tol_tau, (b, ef, tol_f, et, tol_tau)
            assert np.abs(want_f).max() > 1e3 * tol_f             # (the check sees the impulse)
        hs.record("anchors: reaction", worst)
        # the body beyond the count: no accumulator, and its vertices feel the force
        none = anchors["vertex"][anchors["body"] == an.BODY_NONE]
        assert len(none) and np.abs(f[none]).max() > 0
        g.destroy()
    hs.same_bits(states[0], states[1], "substep against run_substeps(1)")
    hs.same_bits(states[0], states[2], "substep against the phase calls")
    assert states[0]["f"].any() and states[0]["tau"].any()


# ---- 4 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,st", [("mixed", "rest"), ("mixed", "random"), ("hung", "random")])
def test_energy_and_lengths_against_float64(name, st):
    g, anchors, motions, X = _scene_engine(name)
    x0, v0 = an.state(st, name, X)
    hs.upload(g, x0, v0)
    s = g.anchor_state()
    _, _, y32, _ = an.points(anchors, motions, an.CLOCK)
    assert np.array_equal(s["point"], y32)                        # (the energy below is stated on the engine's own points)
    ref, bound, l64 = an.energy64(anchors, x0, s["point"])
    w = abs(s["energy"] - ref) / bound
    print(f"anchor energy: {name} {st}: {s['energy']:.9e}, {w:.3g} of the bound")
    hs.record(f"anchor energy: {name} {st}", w)
    assert ref > 0 and w <= 1.0, (s["energy"], ref, bound)
    wl = float((np.abs(s["length"].astype(np.float64) - l64) / np.maximum(U * l64 * (1 + 2.0 ** -20), 1e-300))[l64 > 0].max())
    hs.record(f"anchor lengths: {name} {st}", wl)
    assert wl <= 1.0 and not s["length"][l64 == 0].any(), wl
    g.rebuild_mapping(True)                                       # the same bits in another particle order
    s2 = g.anchor_state()
    assert s2["energy"] == s["energy"] and np.array_equal(s2["length"], s["length"]) and np.array_equal(s2["point"], s["point"])
    assert g.stats()["error_flags"] == 0
    g.destroy()


# ---- 5 -------------------------------------------------------------------------------------------------------------
def _flying(name, seed=3):
    cloths, anchors, motions, X = an.scene(name)
    v0 = np.array([4.0, 0.3, 0.0], np.float32) + 0.05 * np.random.default_rng(seed).normal(size=X.shape).astype(np.float32)
    return X.copy(), v0


@pytest.mark.parametrize("case", ["null", "slack"])
def test_anchors_that_do_nothing_add_an_exact_zero(case):
    """40 substeps through re-sorts, the sheets flying: a table of anchors with k = c = 0, or of cords far longer than
    any distance the run reaches, against an engine that never called mpm_set_anchors -- x, v, C, F and the accumulators
    bit for bit, and the forces of CalcFemStateAndForce before the first substep"""
    A = hs.ARR()
    cloths, table, motions, X = an.scene("mixed")
    x0, v0 = _flying("mixed")
    t = _null(table) if case == "null" else table.copy()
    if case == "slack":
        t["flags"], t["rest_length"] = an.TENSION, 10.0
        t["stiffness"], t["damping"] = 1e-6, 1e-9
    es = [_engine(cloths), _engine(cloths)]
    es[0].set_body_motions(_motions(motions))
    es[0].set_anchors(t)
    assert es[0].anchors_max_stable_dt() > tl.DT
    before = es[0].stats()["rebuilds"]
    forces = []
    for g in es:
        hs.upload(g, x0, v0)
        g.rebuild_mapping(False)
        g.calc_fem_state_and_force(tl.DT)
        forces.append(g.download(A.FORCES))
        hs.upload(g, x0, v0)
        for _ in range(4):
            g.run_substeps(10, tl.DT, -1)
        g.gpu_sync()
        assert g.stats()["error_flags"] == 0, g.stats()
    assert np.array_equal(hs.bits(forces[0]), hs.bits(forces[1]))
    assert es[0].stats()["rebuilds"] - before >= 1
    assert not es[0].anchor_forces().any() and es[0].anchor_state()["length"].max() < 10.0
    hs.same_bits(_state(es[0]), _state(es[1]), case)
    for g in es:
        g.destroy()


def test_the_degenerate_spring_and_off_means_off():
    A = hs.ARR()
    cloths, table, motions, X = an.scene("mixed")
    x0, v0 = an.state("random", "mixed", X)
    es = [_engine(cloths), _engine(cloths)]
    es[1].set_body_motions(_motions(motions))
    # (the clocks at zero: the degenerate anchor's point is where its body is now)
    deg = table[-1:].copy()
    _, _, y32, _ = an.points(deg, motions, 0.0)
    x0[an.DEGENERATE_VERTEX] = y32[0]
    es[1].set_anchors(deg)
    assert es[1].anchors_max_stable_dt() < np.inf
    forces = []
    for g in es:
        hs.upload(g, x0, v0)
        g.rebuild_mapping(False)
        g.calc_fem_state_and_force(DT)
        forces.append(g.download(A.FORCES))
    assert es[1].anchor_state()["length"][0] == 0 and not es[1].anchor_forces().any()
    assert np.array_equal(hs.bits(forces[0]), hs.bits(forces[1]))
    a, b = es[0].external_body_force_to_host(), es[1].external_body_force_to_host()
    assert np.array_equal(hs.bits(a[0]), hs.bits(b[0])) and np.array_equal(hs.bits(a[1]), hs.bits(b[1]))
    # cleared: the launches of an engine that never had anchors -- no re-sort check more, an empty vertex-force phase
    es[1].set_anchors(table)
    es[1].set_anchors(table[:0])
    assert len(es[1].get_anchors()) == 0 and es[1].anchors_max_stable_dt() == np.inf and not es[1].anchor_forces().any()
    x1, v1 = _flying("mixed")
    checks = [g.stats()["resort_checks"] for g in es]
    for g in es:
        hs.upload(g, x1, v1)
        for _ in range(4):
            g.run_substeps(10, tl.DT, -1)
        g.gpu_sync()
        assert g.stats()["error_flags"] == 0
    hs.same_bits(_state(es[0]), _state(es[1]), "set and cleared")
    assert es[0].stats()["resort_checks"] - checks[0] == es[1].stats()["resort_checks"] - checks[1]
    ph = [g.profile_substeps(2, tl.DT, -1)[0]["vforce"] for g in es]
    print(f"vertex-force phase, never set / cleared: {ph}")
    es[1].set_body_motions(_motions(motions))
    es[1].set_anchors(_null(table))
    on = es[1].profile_substeps(2, tl.DT, -1)[0]["vforce"]
    assert ph[1] < 0.5 * on, (ph, on)                             # (cleared: the phase is empty again)
    for g in es:
        g.destroy()


# ---- 6 -------------------------------------------------------------------------------------------------------------
def test_particle_order():
    g, anchors, motions, X = _scene_engine("mixed", clock=False)
    x0, v0 = an.state("random", "mixed", X)
    out = []
    for k in range(2):
        if k:
            # a forced re-sort: the state five cells further along x, two substeps; then everything as at the start
            before = g.stats()["rebuilds"]
            hs.upload(g, x0 + np.array([5.0 / 64, 0, 0], np.float32), v0)
            g.run_substeps(2, DT, -1)
            g.gpu_sync()
            assert g.stats()["rebuilds"] > before
            g.rebuild_mapping(True)
            g.reallocate_external_bodies(an.N_BODIES)
            g.set_body_motions(_motions(motions))
        hs.upload(g, x0, v0)
        pids = g.download(hs.ARR().PIDS)
        f = g.anchor_forces()
        g.substep(DT, -1)
        g.gpu_sync()
        out.append((pids, f) + g.external_body_force_to_host())
    assert not np.array_equal(out[0][0], out[1][0])
    for a, b in zip(out[0][1:], out[1][1:]):
        assert a.any() and np.array_equal(hs.bits(a), hs.bits(b))
    assert g.stats()["error_flags"] == 0
    g.destroy()


# ---- 7 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pinned", [False, True])
def test_clocks(pinned):
    """a body translating at constant v: after n substeps every point is p_WB + n dt v + R p_BQ within an ulp -- with
    anchors alone (the clock kernel runs with zero pins), and with a pin on the same body (one advance, not two)"""
    from drake_amd import Pin
    cloths, table, motions, X = an.scene("hung")
    m = an.motion32(motions[0][0], an._rot((1, 1, 0), 0.3), (0.02, -0.01, 0.015), (0, 0, 0))
    soft = table.copy()
    soft["stiffness"], soft["flags"] = 1e-3, 0
    g = _engine(cloths, material=dict(gravity=0.0))
    g.set_anchors(soft)                                            # (motions may be set after anchors)
    g.set_body_motions(_motions({0: m}))
    if pinned:
        pt, Rt, _, _, _ = an.pose64(m, 0.0)
        g.set_pins([Pin(70, 0, (X[70].astype(np.float64) - pt) @ Rt)])
    n = 7
    g.run_substeps(3, tl.DT, -1)
    for _ in range(2):
        g.substep(tl.DT, -1)
    for _ in range(2):
        hs.phases(g, tl.DT)
    g.gpu_sync()
    assert g.stats()["error_flags"] == 0
    y64, _, _, _ = an.points(soft, {0: m}, n * float(np.float32(tl.DT)))
    point = g.anchor_state()["point"].astype(np.float64)
    w = float((np.abs(point - y64) / np.spacing(np.abs(y64).astype(np.float32))).max())
    hs.record(f"anchors: clock after {n} substeps, pinned {pinned}", w)
    assert w <= 1.0, w
    moved = np.abs(y64 - an.points(soft, {0: m}, (n - 1) * float(np.float32(tl.DT)))[0]).max()
    assert moved > 50 * np.spacing(np.float32(0.5))               # (one substep more or less would show)
    g.destroy()


# ---- 8, 9 ------------------------------------------------------------------------------------------------------------
def _hung(k=None, c=0.0, L=2 * an.H0, material=None):
    """the hung scene under gravity; k None: a twin without anchors.  -> (engine, anchors, M)"""
    cloths, anchors, motions = an.scene_hung(k=k or 1.0, c=c, L=L)
    g = _engine(cloths, material=material, bodies=1)
    g.set_body_motions(_motions(motions))
    if k is not None:
        g.set_anchors(anchors)
    return g, anchors, motions


def test_a_cord_stops_a_fall():
    """The hung sheet under gravity, cords taut at the start (l == L), and a twin without anchors; dt is tl.DT or half
    the anchors' stability limit, whichever is smaller.  Allowance
    s = 4 M |g| / k: twice the factor 2 of a suddenly loaded spring with the whole weight on one cord.  k is chosen so
    that s = H0, and the step count so that free fall, 1/2 |g| t^2 >= L + 2 s, carries the twin's corners to twice L + s
    from their attachment points."""
    A = hs.ARR()
    L, grav = 2 * an.H0, 9.8
    twin, anchors, motions = _hung(L=L)
    M = float(twin.download(A.MASSES).astype(np.float64).sum())
    s = an.H0
    k = 4 * M * grav / s
    g, anchors, motions = _hung(k=k, L=L)
    dt = min(tl.DT, 0.5 * g.anchors_max_stable_dt())
    steps = int(np.ceil(np.sqrt(2 * (L + 2 * s) / grav) / dt)) + 1
    y = an.points(anchors, motions, 0.0)[0]
    longest = 0.0
    for _ in range(0, steps, 10):
        g.run_substeps(10, dt, -1)
        twin.run_substeps(10, dt, -1)
        longest = max(longest, float(g.anchor_state()["length"].max()))
    for e in (g, twin):
        e.gpu_sync()
        assert e.stats()["error_flags"] == 0
    far = np.linalg.norm(hs.vertices(twin, A.POSITIONS)[anchors["vertex"]].astype(np.float64) - y, axis=1).min()
    print(f"cords: M = {M:.4g} kg, k = {k:.4g} N/m, {steps} substeps; longest cord {longest:.5f} of L + s = {L + s:.5f}; "
          f"the twin's corners at {far:.5f}")
    hs.record("anchors: longest cord over L + 4 M g / k", longest / (L + s))
    assert far >= 2 * (L + s), (far, L + s)
    assert L < longest <= L + s, (longest, L + s)
    g.destroy()
    twin.destroy()


def test_weight_at_rest():
    """The hung sheet with cord damping and mpm_set_damping, run until speed_max stops falling; then the body's mean
    vertical force over a window against M |g|.  A twin whose corners are pinned to the same still body sets the margin:
    the anchors' deviation may be 4 x the twin's, or 1e-3 M |g|, whichever is larger."""
    from drake_amd import Pin
    A = hs.ARR()
    grav, L, window, chunk = 9.8, 2 * an.H0, 400, 400
    devs = {}
    probe, anchors, motions = _hung(L=L)
    M = float(probe.download(A.MASSES).astype(np.float64).sum())
    m_corner = float(hs.vertices(probe, A.MASSES)[anchors["vertex"]].astype(np.float64).min())
    k = 4 * M * grav / an.H0
    probe.set_anchors(an.scene_hung(k=k, c=0.2 * np.sqrt(k * m_corner), L=L)[1])
    dt = min(tl.DT, 0.5 * probe.anchors_max_stable_dt())         # (one dt for both twins)
    probe.destroy()
    for kind in ("pins", "anchors"):
        g, anchors, motions = _hung(k=k if kind == "anchors" else None, c=0.2 * np.sqrt(k * m_corner), L=L)
        if kind == "pins":
            X = an.scene("hung")[3]
            g.set_pins([Pin(int(v), 0, X[v].astype(np.float64) - motions[0][0].astype(np.float64)) for v in anchors["vertex"]])
        beta = 1e-3                                               # the largest halving of 1 ms that the damping guard lets pass
        g.set_damping([(beta, 0.0)])
        while g.damping_max_stable_dt() < 2 * dt:
            beta *= 0.5
            g.set_damping([(beta, 0.0)])
        speeds = []
        for _ in range(40):
            g.run_substeps(chunk, dt, -1)
            speeds.append(float(g.measure()[1]["speed_max"]))
            if len(speeds) > 3 and speeds[-1] >= 0.9 * speeds[-2]:
                break
        g.reallocate_external_bodies(1)
        g.run_substeps(window, dt, -1)
        _, f = g.finalize_external_contact_forces(window * dt)
        g.gpu_sync()
        assert g.stats()["error_flags"] == 0
        devs[kind] = abs(-float(f[0, 2]) - M * grav) / (M * grav)
        print(f"weight at rest, {kind}: {len(speeds)} chunks of {chunk}, speed_max {speeds[-1]:.3g}, body force {f[0]} N, "
              f"M |g| = {M * grav:.6g} N, deviation {devs[kind]:.3g} of it")
        g.destroy()
    hs.record("anchors: weight at rest over the margin", devs["anchors"] / max(4 * devs["pins"], 1e-3))
    assert devs["anchors"] <= max(4 * devs["pins"], 1e-3), devs


# ---- 10 ------------------------------------------------------------------------------------------------------------
def test_scheduling_through_resorts_and_the_coupled_path():
    from drake_amd import Collider
    cloths, _, _, X = an.scene("hung")
    vb = (4.0, 0.3, 0.0)
    probe = _engine(cloths, bodies=0)
    m_corner = float(hs.vertices(probe, hs.ARR().MASSES)[[0, 11, 132, 143]].astype(np.float64).min())
    probe.destroy()
    # (cords soft enough for tl.DT: W dt^2 = 0.02 and 2 G dt = 0.1 of the guard's 4)
    _, anchors, motions = an.scene_hung(k=0.02 * m_corner / tl.DT ** 2, c=0.05 * m_corner / tl.DT, L=4 * an.H0)
    motions = {0: an.motion32(motions[0][0], np.eye(3), vb, (0, 0, 0))}
    x0 = X.copy()
    v0 = (0.9 * np.array(vb, np.float32) + 0.05 * np.random.default_rng(3).normal(size=x0.shape)).astype(np.float32)
    n, es = 60, []
    for k in range(2):
        g = _engine(cloths, bodies=2)
        g.set_body_motions(_motions(motions))
        g.set_anchors(anchors)
        assert tl.DT <= 0.5 * g.anchors_max_stable_dt()
        hs.upload(g, x0, v0)
        es.append(g)
    before = es[0].stats()["rebuilds"]
    es[0].run_substeps(n, tl.DT, -1)
    for _ in range(n):
        es[1].substep(tl.DT, -1)
    for g in es:
        g.gpu_sync()
        assert g.stats()["error_flags"] == 0, g.stats()
    assert es[0].stats()["rebuilds"] - before >= 2, es[0].stats()
    s = [_state(g) for g in es]
    hs.same_bits(s[0], s[1], "run_substeps(n) against n substeps")
    assert s[0]["f"][0].any() and es[0].anchor_forces().any()     # (the cords pulled: the body felt it)
    es[1].destroy()
    # the coupled path: a sphere (body 1) under the sheet, the anchored body 0 still
    g = es[0]
    g.reallocate_external_bodies(2)
    g.set_body_motions(_motions({0: an.motion32(an.scene("hung")[2][0][0], np.eye(3), (0, 0, 0), (0, 0, 0))}))
    hs.upload(g, X)
    ball = [Collider(1, body=1, p_WB=(0.375 + 5.5 * an.H0, 0.375 + 5.5 * an.H0, 0.5 - 0.03 - 0.002), dims=(0.03, 0, 0))]
    res = g.run_coupled_substeps(60, tl.DT, ball, 0.5, 1e5, 1e-4)
    g.gpu_sync()
    assert g.stats()["error_flags"] == 0
    tau, f = g.external_body_force_to_host()
    print(f"coupled: contacts {max(r['contacts'] for r in res)}, anchored body {f[0]}, sphere {f[1]}")
    assert max(r["contacts"] for r in res) > 0 and f[0].any() and f[1].any()
    assert np.isfinite(g.download(hs.ARR().VELOCITIES)).all()
    g.destroy()


# ---- 11 ------------------------------------------------------------------------------------------------------------
def test_refusals():
    from drake_amd import Collider, GpuMpm, MpmError

    def refused(call, says=None):
        with pytest.raises(MpmError) as e:
            call()
        assert e.value.code == -1, e.value
        if says:
            assert says in str(e.value), e.value

    cloths, table, motions, X = an.scene("mixed")
    nv = len(X)
    g0 = GpuMpm(6)
    for Xc, T in cloths:
        g0.add_qr_cloth(Xc, np.zeros_like(Xc), T)
    refused(lambda: g0.set_anchors(table), says="finalize")
    g0.destroy()

    g = _engine(cloths)
    # the bodies' motions are missing: the table is taken, every entry point that would launch the kernel refuses
    g.set_anchors(table)
    floor = [Collider(0, body=0, p_WB=(0.5, 0.5, 0.3))]
    before = g.stats()["substeps"]
    some = {b: m for b, m in motions.items() if b != 2}
    g.set_body_motions(_motions(some))
    for call in (lambda: g.run_substeps(1, DT, -1), lambda: g.substep(DT, -1), lambda: g.calc_fem_state_and_force(DT),
                 lambda: g.grid_to_particle(DT), lambda: g.profile_substeps(1, DT, -1), lambda: g.substep_begin(DT),
                 lambda: g.run_coupled_substeps(1, DT, floor, 0.5, 1e5, 1e-4), lambda: g.anchor_forces(),
                 lambda: g.anchor_state()):
        refused(call, says="anchor on body 2, which has no motion")
    assert g.stats()["substeps"] == before
    g.set_body_motions(_motions(motions))
    x0, v0 = an.state("random", "mixed", X)
    hs.upload(g, x0, v0)
    g.substep(DT, -1)
    hs.upload(g, x0, v0)
    good, lim = g.get_anchors(), g.anchors_max_stable_dt()
    assert np.array_equal(good, table)
    f_before, acc_before = g.anchor_forces(), g.external_body_force_to_host()
    assert f_before.any() and acc_before[1].any()

    def bad(**kw):
        t = good.copy()
        for key, val in kw.items():
            t[key][3] = val
        return t

    for t in (bad(vertex=nv), bad(vertex=nv + 7), bad(p_BQ=(0.0, np.nan, 0.0)), bad(p_BQ=(np.inf, 0.0, 0.0)), bad(stiffness=-1.0),
              bad(stiffness=np.nan), bad(rest_length=-1e-3), bad(rest_length=np.inf), bad(damping=-0.1), bad(damping=np.nan),
              bad(flags=2), bad(flags=0x80000001)):
        refused(lambda t=t: g.set_anchors(t), says="anchor 3")
        assert np.array_equal(g.get_anchors(), good) and g.anchors_max_stable_dt() == lim
    # a table that does not fit 2^31 records is refused by its count, before an anchor is read
    assert g.lib.mpm_set_anchors(g.h, 1 << 31, good.ctypes.data) == -1 and "too large" in g.lib.mpm_last_error().decode()
    assert np.array_equal(g.get_anchors(), good) and g.anchors_max_stable_dt() == lim
    assert np.array_equal(hs.bits(g.anchor_forces()), hs.bits(f_before))
    acc = g.external_body_force_to_host()
    assert np.array_equal(hs.bits(acc[0]), hs.bits(acc_before[0])) and np.array_equal(hs.bits(acc[1]), hs.bits(acc_before[1]))
    # partitioned, halo, team and chain calls on an engine with anchors
    nb = 64 // 4
    refused(lambda: g.dist_init(0, 1, [0, nb], 2, 2, 2), says="anchors")
    refused(lambda: g.substep_mid_halo(DT), says="anchors")
    refused(lambda: g.team_prepare(), says="anchors")
    refused(lambda: g.chain_substeps(1, DT), says="anchors")
    # the dt guard: the limit is the restatement's; at it the substep runs, just above it every entry point refuses
    mass = hs.vertices(g, hs.ARR().MASSES).astype(np.float64)
    assert abs(lim / an.max_stable_dt(good, mass) - 1.0) < 1e-5
    before = g.stats()["substeps"]
    big = float(np.nextafter(np.float32(lim), np.float32(np.inf)))
    for call in (lambda: g.run_substeps(2, big, -1), lambda: g.substep(big, -1), lambda: g.particle_to_grid(big),
                 lambda: g.profile_substeps(2, big, -1), lambda: g.run_coupled_substeps(2, big, floor, 0.5, 1e5, 1e-4),
                 lambda: g.substep_begin(big)):
        refused(call, says="mpm_anchors_max_stable_dt")
    assert g.stats()["substeps"] == before
    g.substep(lim, -1)
    assert g.stats()["substeps"] == before + 1
    ph, _ = g.profile_substeps(2, DT, -1)
    assert ph["vforce"] > 0.0, ph
    g.gpu_sync()
    # an empty table lifts the refusals; a partitioned engine refuses the call
    g.set_anchors(good[:0])
    g.run_substeps(1, big, -1)
    g.dist_init(0, 1, [0, nb], 2, 2, 2)
    refused(lambda: g.set_anchors(good), says="partitioned")
    assert len(g.get_anchors()) == 0
    g.destroy()
