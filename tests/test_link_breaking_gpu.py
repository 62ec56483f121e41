"""Breakable links (mpm_set_link_limits, mpm_set_broken_links) on the engine; the model, scenes and derived limits are in
tests/link_breaking.py.

1. The flags after one CalcFemStateAndForce are the float64 verdicts on every decided link (every link is decided: the
   CPU test asserts it), mpm_link_break_measure's l2 and verdict are the host function's bits on every link, the count
   matches; in the rows scenes the duplicate pair's two links go different ways and a vertex loses all its links.
2. mpm_link_forces and MPM_ARR_FORCES with a mixed broken / intact table are, to the bit, those of an engine whose table
   lacks the broken links' stiffness and damping; link by link (scissors leave one link at a time) the force on a is the
   host function's and the force on b its negative, every bit but the sign of a zero, which the row's sum onto the
   padding's +0 does not keep; the links' total force is zero within the rounding of the rows' additions.
3. mpm_link_energy: a broken link's term is 0, its length is still reported.
4. Monotone flags, scissors and restore; mpm_set_links clears limits and flags.
5. Particle order and deterministic mode.
6. Every substep path that an engine with links accepts, with links that break during the run.
7. Off means off, to the bit and to the launch count of the re-sort checks.
8. Dynamics: a seam thrown apart rips and the strips part, its twin without limits holds; a strip hung by two cords
   swings on one after the other is cut.
9. Refusals, each with nothing changed."""
import numpy as np
import pytest

from tests import harness as hs
from tests import link_breaking as lb
from tests import links as lk
from tests import substep_paths as sp
from tests import transfer_layouts as tl

pytestmark = pytest.mark.gpu

U = lb.U
_CACHE = {}


def _fem(g):
    g.rebuild_mapping(False)
    g.calc_fem_state_and_force(min(1e-5, 0.5 * g.links_max_stable_dt()))


def _host(links, x, b):
    from drake_amd import capi
    B2 = capi.link_break_squared(b)
    l2, breaks = capi.link_breaks(x[links["a"]], x[links["b"]], B2)
    return l2, breaks & (B2 > 0)


def _without(links, broken):
    """the table with the broken links' stiffness and damping removed"""
    out = links.copy()
    out["stiffness"][broken] = 0.0
    out["damping"][broken] = 0.0
    return out


def refused(call, says=None):
    from drake_amd import MpmError
    with pytest.raises(MpmError) as e:
        call()
    assert e.value.code == -1, e.value
    if says:
        assert says in str(e.value), e.value


# ---- 1 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(lb.SCENES))
def test_flags_are_float64_verdicts_and_measure_is_the_host_bits(name):
    cloths, links, X = lb.scene(name)
    g = hs.engine(cloths)
    g.set_links(links)
    n = len(links)
    assert not g.link_break_measure()[1].any() and g.link_break_state()[1] == 0
    seen = np.zeros(2, int)
    for st in lb.STATES:
        x, v = lb.state(st, X)
        b = lb.limits(name, links, x)
        g.set_link_limits(None)
        g.set_broken_links(np.zeros(n, bool))
        hs.upload(g, x, v)
        g.set_link_limits(b)
        assert np.array_equal(g.get_link_limits(), b)
        flags, count = g.link_break_state()
        assert not flags.any() and count == 0
        l2h, bh = _host(links, x, b)
        l2, would = g.link_break_measure()
        assert np.array_equal(hs.bits(l2), hs.bits(l2h)) and np.array_equal(would, bh), (st, int((would != bh).sum()))
        _fem(g)
        flags, count = g.link_break_state()
        ref, decided, _ = lb.verdicts64(links, x, b)
        assert decided.all()
        assert np.array_equal(flags[decided], ref[decided]), (st, int((flags != ref).sum()))
        assert np.array_equal(flags, bh) and count == int(flags.sum())
        seen += (int(flags.sum()), int((~flags).sum()))
        # measured again, the state is untouched and broken links are evaluated like the others
        l2b, wouldb = g.link_break_measure()
        assert np.array_equal(hs.bits(l2b), hs.bits(l2h)) and np.array_equal(wouldb, bh)
        assert np.array_equal(g.link_break_state()[0], flags)
        f = g.link_forces()
        if name in lb.ROWS:
            assert flags[n - 1] and not flags[n - 2]
            assert not f[lb.doomed(links)].any() and f.any()
        assert np.array_equal(g.get_links(), links)
        assert g.stats()["error_flags"] == 0, g.stats()
    assert seen.min() > 0
    g.destroy()


# ---- 2, 3 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["stack", "rows65"])
def test_forces_and_energy_of_a_mixed_table(name):
    A = hs.ARR()
    cloths, links, X = lb.scene(name)
    x, v = lb.state("random", X)
    b = lb.limits(name, links, x)
    broken = lb.verdicts64(links, x, b)[0]
    assert broken.any() and not broken.all()
    a, t = hs.engine(cloths), hs.engine(cloths)
    a.set_links(links)
    a.set_link_limits(b)
    t.set_links(_without(links, broken))
    lim = a.links_max_stable_dt()
    out = []
    for g in (a, t):
        hs.upload(g, x, v)
        _fem(g)
        out.append((g.link_forces(), hs.vertices(g, A.FORCES), g.link_energy()))
    assert np.array_equal(a.link_break_state()[0], broken)
    (fa, Fa, (ea, la)), (ft, Ft, (et, lt)) = out
    assert fa.any() and np.array_equal(hs.bits(fa), hs.bits(ft)) and np.array_equal(hs.bits(Fa), hs.bits(Ft))
    # the energy: the twin's terms of the broken links are 0 because their k is; the lengths are all there
    assert ea == et and ea > 0 and np.array_equal(hs.bits(la), hs.bits(lt)) and la[broken].all()
    ref, bound, _ = lk.energy64(_without(links, broken), x)
    assert abs(ea - ref) <= bound, (ea, ref, bound)
    # the guard is the whole table's
    assert a.links_max_stable_dt() == lim
    full = hs.engine(cloths)
    full.set_links(links)
    assert full.links_max_stable_dt() == lim and lim <= t.links_max_stable_dt()
    full.destroy()
    # the total: every link's two halves cancel to the bit, what is left is the rounding of the rows' additions
    _, _, acc = lk.vertex_forces64(_without(links, broken), x, v, len(X))
    total = np.abs(fa.astype(np.float64).sum(axis=0)).max()
    print(f"sum of the link forces: {total:.3e}, bound {acc.sum():.3e}, gross {np.abs(fa).sum():.3e}")
    assert total <= acc.sum()
    for g in (a, t):
        assert g.stats()["error_flags"] == 0
        g.destroy()


def test_one_link_at_a_time_is_antisymmetric_to_the_bit():
    """scissors leave one link intact at a time: mpm_link_forces then holds that link's force on a and on b alone -- the
    host function's value, and each other's negative"""
    from drake_amd import capi
    cloths, links, X = lb.scene("stack")
    x, v = lb.state("random", X)
    g = hs.engine(cloths)
    g.set_links(links)
    hs.upload(g, x, v)
    n = len(links)
    acted = 0
    for i in range(n):
        cut = np.ones(n, bool)
        cut[i] = False
        g.set_broken_links(cut)
        f = g.link_forces()
        va, vb = int(links["a"][i]), int(links["b"][i])
        host = capi.link_force(links[i], x[va], x[vb], v[va], v[vb])
        # (values, not words: the row adds the force to the padding's +0, which turns a -0 into +0)
        assert np.array_equal(f[va], host), i
        assert np.array_equal(f[vb], -f[va]), i
        others = np.ones(len(X), bool)
        others[[va, vb]] = False
        assert not f[others].any(), i
        acted += bool(f[va].any())
    assert acted > n // 2
    flags, count = g.link_break_state()
    assert count == n - 1 and not flags[n - 1]
    assert g.stats()["error_flags"] == 0
    g.destroy()


# ---- 4 -------------------------------------------------------------------------------------------------------------------
def test_monotone_flags_scissors_and_restore():
    cloths, links, X = lb.scene("stack")
    x, v = lb.state("random", X)
    b = lb.limits("stack", links, x)
    broken = lb.verdicts64(links, x, b)[0]
    n = len(links)
    g, fresh = hs.engine(cloths), hs.engine(cloths)
    g.set_links(links)
    fresh.set_links(links)
    g.set_link_limits(b)
    hs.upload(g, x, v)
    _fem(g)
    assert np.array_equal(g.link_break_state()[0], broken)
    # the load goes away: every length halves about the centre, nothing would break, the flags stay
    c = x.astype(np.float64).mean(axis=0)
    calm = (c + 0.5 * (x.astype(np.float64) - c)).astype(np.float32)
    hs.upload(g, calm, v)
    assert not g.link_break_measure()[1].any()
    _fem(g)
    flags, count = g.link_break_state()
    assert np.array_equal(flags, broken) and count == int(broken.sum())
    # the limits go away: the flags stay, and so does what the substep applies
    g.set_link_limits(None)
    assert not g.get_link_limits().any() and np.array_equal(g.link_break_state()[0], broken)
    hs.upload(g, x, v)
    _fem(g)
    assert np.array_equal(g.link_break_state()[0], broken) and not g.link_break_measure()[1].any()
    twin = hs.engine(cloths)
    twin.set_links(_without(links, broken))
    hs.upload(twin, x, v)
    assert np.array_equal(hs.bits(g.link_forces()), hs.bits(twin.link_forces()))
    # scissors: the array replaces every flag
    chosen = np.arange(n) % 3 == 1
    g.set_broken_links(chosen)
    flags, count = g.link_break_state()
    assert np.array_equal(flags, chosen) and count == int(chosen.sum())
    twin.set_links(_without(links, chosen))
    hs.upload(twin, x, v)
    assert np.array_equal(hs.bits(g.link_forces()), hs.bits(twin.link_forces()))
    e, length = g.link_energy()
    assert e == twin.link_energy()[0] and length[chosen].all()
    # restore: after an all-zero array the engine is a fresh one's bits
    g.set_broken_links(np.zeros(n, bool))
    assert g.link_break_state()[1] == 0 and not g.link_break_state()[0].any()
    hs.upload(fresh, x, v)
    assert np.array_equal(hs.bits(g.link_forces()), hs.bits(fresh.link_forces()))
    # (the total forces are not compared: this engine's deformation gradients have a history of their own)
    _fem(g)
    assert not g.link_break_state()[0].any() and np.array_equal(hs.bits(g.link_forces()), hs.bits(fresh.link_forces()))
    # mpm_set_links: the limits and flags go with the table they belonged to
    g.set_link_limits(b)
    g.set_broken_links(chosen)
    g.set_links(links)
    assert not g.get_link_limits().any() and g.link_break_state()[1] == 0 and not g.link_break_state()[0].any()
    hs.upload(g, x, v)
    _fem(g)
    assert not g.link_break_state()[0].any()
    assert np.array_equal(hs.bits(g.link_forces()), hs.bits(fresh.link_forces()))
    for e_ in (g, fresh, twin):
        assert e_.stats()["error_flags"] == 0
        e_.destroy()


# ---- 5 -------------------------------------------------------------------------------------------------------------------
def test_particle_order_and_deterministic_mode():
    """flags, l2 and link forces by link / original vertex id are the same bits on an engine whose slots have moved
    (substeps through a re-sort, then the full sort) as on a fresh one, and in default mode"""
    A = hs.ARR()
    cloths, links, X = lb.scene("rows65")
    g, fresh, dflt = hs.engine(cloths), hs.engine(cloths), hs.engine(cloths, deterministic=False)
    pid0 = g.download(A.PIDS)
    x0, v0 = lb.state("random", X)
    hs.upload(g, x0 + np.array([5.0 / 64, 0.0, 0.0], np.float32), v0 + np.array([3.0, 0.5, 0.0], np.float32))
    g.run_substeps(12, 1e-4, -1)
    g.gpu_sync()
    g.rebuild_mapping(True)
    assert not np.array_equal(g.download(A.PIDS), pid0), "no slot moved"
    x, v = lb.state("rotation", X)
    b = lb.limits("rows65", links, x)
    res = []
    for e in (g, fresh, dflt):
        e.set_links(links)
        e.set_link_limits(b)
        hs.upload(e, x, v)
        _fem(e)
        flags, count = e.link_break_state()
        res.append((flags, np.array([count]), hs.bits(e.link_break_measure()[0]), hs.bits(e.link_forces()), hs.bits(e.link_energy()[1])))
    assert res[0][0].any() and not res[0][0].all()
    for k in (1, 2):
        for a, c in zip(res[0], res[k]):
            assert np.array_equal(a, c), k
    for e in (g, fresh, dflt):
        assert e.stats()["error_flags"] == 0
        e.destroy()


# ---- 6 -------------------------------------------------------------------------------------------------------------------
PATH_DELTAS = (1e-5, 5e-5, 2e-4, 1e-3, 1.0)     # m above the length at the start: from "at once" to "never"
SPARSE_CHECKS = {"MPM_RESORT_EVERY": "12", "MPM_QUIET_FACTOR": "0"}   # substeps skip themselves (tests/feature_paths.py)
ACCEPTED = ("run_substeps", "profile_substeps", "phase_calls", "phase_calls_undeferred", "substep_begin_end", "coupled")


def _soft(g, links, dt, share=0.25):
    """the links with every k and c scaled so that dt is `share` of mpm_links_max_stable_dt"""
    out = links.copy()
    for _ in range(3):
        g.set_links(out)
        s = share * g.links_max_stable_dt() / dt
        if abs(s - 1.0) < 1e-3:
            break
        out["stiffness"] *= np.float32(s * s)
        out["damping"] *= np.float32(s)
    g.set_links(out)
    assert abs(share * g.links_max_stable_dt() / dt - 1.0) < 1e-2
    return out


def _armed(env=None, **kw):
    """tests/substep_paths.engine with 342 links between its two sheets -- seams, springs and cords in turn, the springs
    and cords at their rest length, the seams 1e-4 as stiff (they pull from the start, and the lower sheet must still
    reach the coupled path's floor) -- and limits PATH_DELTAS above the lengths at the start: no link would break on
    the state at the start, some break on the way, some never"""
    with hs.environ(env):
        g = sp.engine(fan=True, **kw)
    A = hs.ARR()
    x = hs.vertices(g, A.POSITIONS).astype(np.float64)
    va = np.arange(0, 1024, 3)
    l0 = np.linalg.norm(x[1024 + va] - x[va], axis=1)
    rows = [(int(a), 1024 + int(a), 1e-4 if i % 3 == 0 else 1.0, 0.0 if i % 3 == 0 else float(l0[i]), 0.01,
             lk.TENSION if i % 3 == 2 else 0) for i, a in enumerate(va)]
    _soft(g, lk.make_links(rows), sp.DT)
    length = g.link_energy()[1]
    b = (length.astype(np.float64) + np.array(PATH_DELTAS)[np.arange(len(va)) % len(PATH_DELTAS)]).astype(np.float32)
    g.set_link_limits(b)
    assert not g.link_break_measure()[1].any() and g.link_break_state()[1] == 0
    return g


def _words(g):
    A = hs.ARR()
    g.gpu_sync()
    st = {k: hs.bits(g.download(arr)).copy() for k, arr in (("pos", A.POSITIONS), ("vel", A.VELOCITIES), ("C", A.AFFINE),
                                                          ("F", A.DEFORMATION_GRADIENTS), ("pids", A.PIDS))}
    flags, count = g.link_break_state()
    st["broken"], st["count"] = flags.astype(np.uint32), np.array([count], np.uint32)
    st["link_forces"] = hs.bits(g.link_forces()).copy()
    return st


def _path(name, env=None):
    key = (name, tuple(sorted((env or {}).items())))
    if key not in _CACHE:
        _, runner, kw = sp.PATHS[name]
        g = _armed(env, **kw)
        runner(g)
        skipped = g.owed_substeps()
        st = _words(g)
        _CACHE[key] = (st, g.stats(), skipped)
        g.destroy()
    return _CACHE[key]


def _some_broke_some_did_not(st):
    n, k = len(st["broken"]), int(st["count"][0])
    assert k == int(st["broken"].sum()) and 0 < k < n, (k, n)
    never = np.arange(n) % len(PATH_DELTAS) == len(PATH_DELTAS) - 1
    assert not st["broken"][never].any()


def _same(sa, sb, what):
    assert set(sa) == set(sb)
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), (what, k, int((sa[k] != sb[k]).sum()))


@pytest.mark.parametrize("name", ["profile_substeps", "phase_calls", "phase_calls_undeferred", "run_substeps_sparse_checks"])
def test_fused_paths_end_in_the_same_flags_and_bits(name):
    (sa, ta, _) = _path("run_substeps")
    (sb, tb, skipped) = _path("run_substeps", SPARSE_CHECKS) if name == "run_substeps_sparse_checks" else _path(name)
    for st in (ta, tb):
        assert st["error_flags"] == 0 and st["substeps"] == sp.N and st["rebuilds"] > 1, st
    if name == "run_substeps_sparse_checks":
        assert skipped > 0, "no substep skipped itself with k_link_break in it"
    _some_broke_some_did_not(sa)
    _same(sa, sb, name)


def test_sums_path_with_and_without_skipped_substeps():
    """substep_begin / substep_end, the member of the sums family that is not a halo call: the same flags and bits with
    a re-sort check in front of every substep as with the sparse checks"""
    (sa, ta, _), (sb, tb, _) = _path("substep_begin_end"), _path("substep_begin_end", SPARSE_CHECKS)
    for st in (ta, tb):
        assert st["error_flags"] == 0 and st["substeps"] == sp.N and st["rebuilds"] > 1, st
    _some_broke_some_did_not(sa)
    _same(sa, sb, "substep_begin_end")


def test_coupled_equals_the_seven_calls():
    """run_coupled_substeps in uneven calls against the seven calls per substep over the floor the lower sheet reaches:
    contact-free chunks behind the watch kernel, whose gated substeps skip themselves, then substeps with contact"""
    from drake_amd import Collider
    from tests import feature_paths as fp
    (sb, tb, _) = _path("coupled")
    g = _armed()
    g.reallocate_external_bodies(1)
    rows = fp.seven_calls(g, [Collider(0, body=0, p_WB=(0.5, 0.5, 0.4985))], sp.N)
    sa, ta = _words(g), g.stats()
    g.destroy()
    contacts = [r["contacts"] for r in rows]
    assert max(contacts) > 0 and min(contacts) == 0, contacts
    for st in (ta, tb):
        assert st["error_flags"] == 0 and st["substeps"] == sp.N, st
    assert ta["rebuilds"] >= 2 and ta["rebuilds"] == tb["rebuilds"]
    _some_broke_some_did_not(sa)
    _same(sa, sb, "coupled")


def test_halo_paths_stay_refused():
    from drake_amd import GpuMpm
    assert set(ACCEPTED) | {"substep_begin_end_halo", "substep_begin_mid_end_halo"} == set(sp.PATHS)
    g = _armed()
    zones = GpuMpm.halo_zone_args([], [])
    refused(lambda: g.substep_begin_halo(sp.DT, zones, 0), says="links")
    refused(lambda: g.substep_mid_halo(sp.DT, -1), says="links")
    assert g.stats()["substeps"] == 0 and g.link_break_state()[1] == 0
    g.destroy()


# ---- 7 -------------------------------------------------------------------------------------------------------------------
def test_off_means_off():
    """40 deterministic substeps through re-sorts on engines with links: never called == limits set and cleared again
    with no flag set, to the bit, and with the same number of re-sort check launches"""
    A = hs.ARR()
    cloths, links, X = lb.scene("stack")
    x0 = X.copy()
    v0 = np.array([4.0, 0.3, 0.0], np.float32) + 0.05 * np.random.default_rng(3).normal(size=x0.shape).astype(np.float32)
    es = [hs.engine(cloths) for _ in range(2)]
    for g in es:
        soft = _soft(g, links, tl.DT)
    es[1].set_link_limits(lb.limits("stack", soft, x0))
    assert es[1].get_link_limits().any()
    es[1].set_link_limits(None)
    assert not es[1].get_link_limits().any() and es[1].link_break_state()[1] == 0
    before = es[0].stats()["rebuilds"]
    for g in es:
        hs.upload(g, x0, v0)
        for _ in range(4):
            g.run_substeps(10, tl.DT, -1)
        g.gpu_sync()
        assert g.stats()["error_flags"] == 0
    assert es[0].stats()["rebuilds"] - before >= 1, es[0].stats()
    for which in (A.POSITIONS, A.VELOCITIES, A.AFFINE, A.DEFORMATION_GRADIENTS, A.PIDS):
        assert np.array_equal(hs.bits(es[0].download(which)), hs.bits(es[1].download(which))), which
    for key in ("substeps", "rebuilds", "resort_checks"):
        assert es[0].stats()[key] == es[1].stats()[key], key
    assert es[0].link_forces().any()
    for g in es:
        g.destroy()


# ---- 8 -------------------------------------------------------------------------------------------------------------------
def test_a_seam_thrown_apart_rips_and_its_twin_holds():
    """Zero gravity, two coplanar strips of 4 x 24 vertices a gap g0 of 8 spacings (4 cells: no grid node in common)
    apart along x, their facing edges sewn by 24 stitches with L = 0, thrown apart with -V and +V along x.  dt is a
    tenth of mpm_links_max_stable_dt, which fixes k.  With omega^2 = n k / mu (mu the reduced mass of the strips) V is
    chosen so that 2 V / omega = 1.5 g0.
    * The twin without limits holds.  Its energy is at most the seam's 1/2 n k g0^2 plus the kinetic M V^2, all of it
      relative (the momenta cancel); the strips' own strain and the grid only take from it.  So the root mean square of the
      stitch lengths, and with it the mean gap, stays below gmax = sqrt(g0^2 + (2 V / omega)^2) = 1.803 g0; 1.1 gmax is
      asserted (symplectic Euler's energy error is of the order omega dt, a few percent here), at samples through
      half a period, and no flag is set.
    * With break_length = 1.25 g0, well inside the twin's reach, every stitch breaks, and from then on the strips fly free:
      the mean gap grows from sample to sample and ends beyond the twin's bound."""
    A = hs.ARR()
    n, m, h, dt = 4, 24, lk.H0, 1e-3
    g0 = 8 * h
    sa = lk.sheet(n, m, (0.375, 0.375, 0.5))
    sb = lk.sheet(n, m, (0.375 + (n - 1) * h + g0, 0.375, 0.5))
    X = np.concatenate([sa[0], sb[0]])
    base = lk.make_links([((n - 1) * m + j, n * m + j, 1.0, 0.0, 0.0, 0) for j in range(m)])
    mat = dict(gravity=0.0)
    a, b = hs.engine([sa, sb], material=mat), hs.engine([sa, sb], material=mat)
    links = _soft(a, base, dt, share=0.1)
    b.set_links(links)
    k = float(links["stiffness"][0])
    mass, pids = a.download(A.MASSES).astype(np.float64), a.download(A.PIDS)
    tri_cloth = (a._tri[:, 0] >= n * m).astype(int)
    cloth = np.concatenate([tri_cloth, (np.arange(2 * n * m) >= n * m).astype(int)])[pids]
    M = np.array([mass[cloth == 0].sum(), mass[cloth == 1].sum()])
    mu = M[0] * M[1] / M.sum()
    omega = np.sqrt(m * k / mu)
    V = 0.75 * g0 * omega
    steps = int(np.ceil(np.pi / omega / dt))
    gmax = float(np.sqrt(g0 ** 2 + (2 * V / omega) ** 2))
    print(f"seam: k = {k:.4g} N/m per stitch, omega = {omega:.4g} 1/s, V = {V:.3g} m/s, half a period = {steps} substeps, "
          f"cells per substep {V * dt * 64:.3g}")
    assert V * dt * 64 < 0.25 and steps >= 16
    v0 = np.zeros_like(X)
    v0[:n * m, 0], v0[n * m:, 0] = -V, V
    a.set_link_limits(np.full(m, 1.25 * g0, np.float32))
    gap = lambda g: float(np.diff(hs.vertices(g, A.POSITIONS)[[links["a"], links["b"]]][:, :, 0], axis=0).mean())   # noqa: E731
    gaps = [[], []]
    for q, g in enumerate((a, b)):
        hs.upload(g, X, v0)
        done = 0
        for s in range(1, 9):
            upto = steps * s // 8
            g.run_substeps(upto - done, dt, -1)
            done = upto
            gaps[q].append(gap(g))
        g.gpu_sync()
        assert g.stats()["error_flags"] == 0
    print("seam: mean gap over g0, ripped:", np.round(np.array(gaps[0]) / g0, 3), "twin:", np.round(np.array(gaps[1]) / g0, 3))
    flags, count = a.link_break_state()
    assert flags.all() and count == m
    assert b.link_break_state()[1] == 0 and not b.link_break_state()[0].any()
    assert max(gaps[1]) <= 1.1 * gmax, (max(gaps[1]) / g0, gmax / g0)
    assert max(gaps[1]) > 1.25 * g0, "the twin never reached the break length: the comparison shows nothing"
    assert np.all(np.diff(gaps[0]) > 0) and gaps[0][-1] > 1.1 * gmax, (gaps[0][-1] / g0, gmax / g0)
    assert not a.link_forces().any() and b.link_forces().any()
    for g in (a, b):
        g.destroy()


def test_a_strip_hung_by_two_cords_swings_on_one_when_the_other_is_cut():
    """A strip of 3 x 24 vertices hangs 8 spacings (4 cells) below a pinned bar of 2 x 24 by two cords from its ends,
    tension-only, at their rest length L.  dt is a quarter of mpm_links_max_stable_dt, which fixes k.  After 20 substeps one
    cord is cut with mpm_set_broken_links; 2000 substeps later (t = 0.1 s)
    * the cut end has fallen: nothing holds it up but the strip's own tension, so its drop is at least half of the free
      fall g t^2 / 2 -- asserted -- while
    * the held end is still on its cord.  Energy: the cord's 1/2 k s^2 is at most what gravity can have given the strip,
      M g (H + s), H = the strip's length (its centre of mass cannot drop further): s <= smax = M g / k +
      sqrt((M g / k)^2 + 2 M g H / k).  The held end's distance from the bar stays below L + smax, and smax is less than
      half of the drop asserted for the cut end (checked on these numbers alone)."""
    from drake_amd import BodyMotion, Pin
    A = hs.ARR()
    n, m, h, dt = 3, 24, lk.H0, 5e-5
    L = 8 * h
    strip = lk.sheet(n, m, (0.4375, 0.3125, 0.5))
    bar = lk.sheet(2, m, (0.4375, 0.3125, 0.5 + L))
    g = hs.engine([strip, bar], bodies=1)
    nv = n * m
    g.set_body_motions([BodyMotion(0)])
    g.set_pins([Pin(nv + q, 0, bar[0][q]) for q in range(2 * m)])
    ends, tops = (0, m - 1), (nv, nv + m - 1)
    links = _soft(g, lk.make_links([(ends[q], tops[q], 1.0, L, 0.0, lk.TENSION) for q in range(2)]), dt)
    k = float(links["stiffness"][0])
    mass, pids = g.download(A.MASSES).astype(np.float64), g.download(A.PIDS)
    in_strip = np.concatenate([g._tri[:, 0] < nv, np.arange(nv + 2 * m) < nv])[pids]
    Mg = float(mass[in_strip].sum()) * 9.81
    assert abs(g.default_material().gravity) == pytest.approx(9.81, rel=1e-2)
    print(f"cords: k = {k:.4g} N/m, static stretch M g / k = {Mg / k:.3g} m")
    g.run_substeps(20, dt, -1)
    g.set_broken_links([False, True])
    assert g.link_break_state()[1] == 1
    z_cut0 = float(hs.vertices(g, A.POSITIONS)[ends[1], 2])
    steps = 2000
    smax = Mg / k + float(np.sqrt((Mg / k) ** 2 + 2 * Mg * (m - 1) * h / k))
    assert smax < 0.5 * 0.25 * 9.81 * (steps * dt) ** 2, smax
    g.run_substeps(steps, dt, -1)
    g.gpu_sync()
    assert g.stats()["error_flags"] == 0
    x = hs.vertices(g, A.POSITIONS).astype(np.float64)
    t = steps * dt
    drop = z_cut0 - x[ends[1], 2]
    held = float(np.linalg.norm(x[ends[0]] - x[tops[0]]))
    print(f"cords: the cut end fell {drop:.4g} m (g t^2 / 2 = {0.5 * 9.81 * t * t:.4g}), the held end is {held:.5f} m from the bar (L = {L:.5f})")
    assert drop >= 0.5 * 0.5 * 9.81 * t * t, drop
    assert L < held <= L + smax, (held, L, smax)
    assert x[ends[0], 2] - x[ends[1], 2] >= 0.5 * drop, "the strip does not hang from the held end"
    flags, count = g.link_break_state()
    assert list(flags) == [False, True] and count == 1
    e, length = g.link_energy()
    assert length[1] > L and abs(length[0] - held) <= 4 * U * held
    f = g.link_forces()
    assert not f[ends[1]].any() and not f[tops[1]].any()
    g.destroy()


# ---- 9 -------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from drake_amd import GpuMpm
    cloths, links, X = lb.scene("stack")
    n = len(links)
    x, v = lb.state("random", X)
    b = lb.limits("stack", links, x)
    # before Finalize
    g0 = GpuMpm(6)
    for Xc, T in cloths:
        g0.add_qr_cloth(Xc, np.zeros_like(Xc), T)
    refused(lambda: g0.set_link_limits(None), says="finalize")
    refused(lambda: g0.set_broken_links(np.zeros(0, bool)), says="finalize")
    g0.destroy()

    g = hs.engine(cloths)
    g.set_links(links)
    hs.upload(g, x, v)
    g.set_link_limits(b)
    _fem(g)
    flags = g.link_break_state()[0]
    assert flags.any() and not flags.all()
    f_before = g.link_forces()

    def unchanged():
        assert np.array_equal(g.get_link_limits(), b)
        got, count = g.link_break_state()
        assert np.array_equal(got, flags) and count == int(flags.sum())
        assert np.array_equal(hs.bits(g.link_forces()), hs.bits(f_before))

    spring = int(np.nonzero((links["rest_length"] > 0) & (b > 0))[0][0])

    def bad(i, val):
        t = b.copy()
        t[i] = val
        return t

    for i, val in ((3, -1e-3), (3, np.nan), (3, np.inf), (3, -np.inf), (3, 1e30), (3, 1e-30),
                   (spring, links["rest_length"][spring]), (spring, 0.5 * links["rest_length"][spring])):
        refused(lambda i=i, val=val: g.set_link_limits(bad(i, val)), says=f"link {i}")
        unchanged()
    # a wrong count, a null array
    refused(lambda: g.set_link_limits(b[:-1]), says="link count")
    refused(lambda: g.set_link_limits(np.concatenate([b, b[:1]])), says="link count")
    refused(lambda: g.set_broken_links(flags[:-1]), says="link count")
    refused(lambda: g.set_broken_links(np.zeros(0, bool)), says="link count")
    unchanged()
    assert g.lib.mpm_set_link_limits(g.h, n, None) == -1 and "null" in g.lib.mpm_last_error().decode()
    assert g.lib.mpm_set_broken_links(g.h, n, None) == -1 and "null" in g.lib.mpm_last_error().decode()
    unchanged()
    assert g.stats()["error_flags"] == 0
    # a partitioned engine refuses the calls (it cannot have links: the table is cleared first)
    g.set_links(links[:0])
    assert len(g.get_link_limits()) == 0 and g.link_break_state()[1] == 0
    g.set_link_limits(None)
    g.set_broken_links(np.zeros(0, bool))
    g.dist_init(0, 1, [0, 64 // 4], 2, 2, 2)
    refused(lambda: g.set_link_limits(None), says="partitioned")
    refused(lambda: g.set_broken_links(np.zeros(0, bool)), says="partitioned")
    refused(lambda: g.link_break_measure(), says="partitioned")
    g.destroy()
