"""Links between cloth vertices (mpm_set_links) on the engine.

1. mpm_link_forces per vertex against the float64 restatement of tests/links.py on every scene x state, within
   R_i 2^-24 sum S (R_i = 18 + n_i, counted in mpm_links.h).  The same after substeps that forced a re-sort and after
   mpm_rebuild_mapping(sort = 1); on the same state, uploaded again, the bits are those of the first evaluation.
2. MPM_ARR_FORCES of an engine with links minus a twin's without is mpm_link_forces, within one rounding of the sum; the
   links' total force is zero within the rounding of the rows' additions alone.
3. mpm_link_energy and its lengths against float64.
4. Links that do nothing contribute an exact zero: slack cords against the same links with k = c = 0, bit for bit.
5. Scheduling: run_substeps(n), n x substep and the five phase calls are bit-equal through several re-sorts; the coupled
   path runs on a floor.
6. Off means off, to the bit and to the launch count of the re-sort checks.
7. Dynamics: two strips joined by a seam close their gap; what the links add to the total momentum stays within the
   rounding of the rows' additions; the twin keeps its gap.
8. Refusals."""
import numpy as np
import pytest

from tests import harness as hs
from tests import links as lk
from tests import transfer_layouts as tl

pytestmark = pytest.mark.gpu

U = lk.U
CASES = [(s, st) for s in lk.SCENES for st in lk.STATES]


def _check_forces(g, links, what):
    A = hs.ARR()
    x, v = hs.vertices(g, A.POSITIONS), hs.vertices(g, A.VELOCITIES)
    f = g.link_forces()
    ref, bound, _ = lk.vertex_forces64(links, x, v, len(x))
    w = lk.margin(f - ref, bound)
    print(f"link forces: {what}: {w:.3g} of the bound")
    hs.record(f"link forces: {what}", w)
    assert w <= 1.0, (what, w)
    linked = np.zeros(len(x), bool)
    linked[links["a"]] = linked[links["b"]] = True
    assert not f[~linked].any()
    return x, v, f


# ---- 1 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,st", CASES)
def test_forces_against_float64(name, st):
    cloths, links, X = lk.scene(name)
    g = hs.engine(cloths)
    g.set_links(links)
    assert np.array_equal(g.get_links(), links)
    x0, v0 = lk.state(st, name, X)
    hs.upload(g, x0, v0)
    x, v, f0 = _check_forces(g, links, f"{name} {st}")
    assert np.array_equal(x, x0) and np.array_equal(v, v0)
    assert f0.any()
    # substeps that force a re-sort: the state five cells further along x, two short substeps
    before = g.stats()["rebuilds"]
    shift = np.array([5.0 / 64, 0.0, 0.0], np.float32)
    hs.upload(g, x0 + shift, v0)
    g.run_substeps(2, min(1e-5, 0.5 * g.links_max_stable_dt()), -1)
    g.gpu_sync()
    assert g.stats()["error_flags"] == 0 and g.stats()["rebuilds"] > before, g.stats()
    _check_forces(g, links, f"{name} {st} after a re-sort")
    # the first state again, in the new particle order: the same bits
    hs.upload(g, x0, v0)
    f1 = g.link_forces()
    assert np.array_equal(hs.bits(f1), hs.bits(f0)), float(np.abs(f1 - f0).max())
    g.rebuild_mapping(True)
    _check_forces(g, links, f"{name} {st} after sort = 1")
    f2 = g.link_forces()
    assert np.array_equal(hs.bits(f2), hs.bits(f0)), float(np.abs(f2 - f0).max())
    assert g.stats()["error_flags"] == 0
    g.destroy()


# ---- 2 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(lk.SCENES))
def test_total_forces_include_links(name):
    A = hs.ARR()
    cloths, links, X = lk.scene(name)
    a, b = hs.engine(cloths), hs.engine(cloths)
    a.set_links(links)
    x0, v0 = lk.state("random", name, X)
    out = []
    for g in (a, b):
        hs.upload(g, x0, v0)
        g.rebuild_mapping(False)
        g.calc_fem_state_and_force(min(1e-5, 0.5 * a.links_max_stable_dt()))
        out.append(hs.vertices(g, A.FORCES))
    fl = a.link_forces()
    assert fl.any() and out[1].any()
    tot = out[1].astype(np.float64) + fl.astype(np.float64)
    err = np.abs(out[0].astype(np.float64) - tot)
    w = float((err / np.maximum(U * np.abs(out[0]).astype(np.float64), 1e-300))[err > 0].max()) if (err > 0).any() else 0.0
    print(f"total forces: {name}: {w:.3g} of one rounding of the sum")
    hs.record(f"links: total forces {name}", w)
    assert w <= 1.0, w
    # the links' total: every link's two halves cancel to the bit, what is left is the rounding of the rows' additions
    _, _, acc = lk.vertex_forces64(links, x0, v0, len(X))
    total = np.abs(fl.astype(np.float64).sum(axis=0)).max()
    print(f"sum of the link forces: {total:.3e}, bound {acc.sum():.3e}, gross {np.abs(fl).sum():.3e}")
    hs.record(f"links: sum of the link forces {name}", total / acc.sum())
    assert total <= acc.sum()
    assert not b.link_forces().any() and b.links_max_stable_dt() == np.inf and len(b.get_links()) == 0
    for g in (a, b):
        assert g.stats()["error_flags"] == 0
        g.destroy()


# ---- 3 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,st", [("mixed", "rest"), ("mixed", "random"), ("seam", "random")])
def test_energy_against_float64(name, st):
    cloths, links, X = lk.scene(name)
    g = hs.engine(cloths)
    g.set_links(links)
    x0, v0 = lk.state(st, name, X)
    hs.upload(g, x0, v0)
    e, length = g.link_energy()
    ref, bound, l64 = lk.energy64(links, x0)
    w = abs(e - ref) / bound
    print(f"link energy: {name} {st}: {e:.9e}, {w:.3g} of the bound")
    hs.record(f"link energy: {name} {st}", w)
    assert ref > 0 and w <= 1.0, (e, ref, bound)
    # the lengths: one float rounding of the square root formed in double
    wl = float((np.abs(length.astype(np.float64) - l64) / np.maximum(U * l64 * (1 + 2.0 ** -20), 1e-300))[l64 > 0].max())
    hs.record(f"link lengths: {name} {st}", wl)
    assert wl <= 1.0 and not length[l64 == 0].any(), wl
    # the same bits in another particle order
    g.rebuild_mapping(True)
    e2, length2 = g.link_energy()
    assert e2 == e and np.array_equal(length2, length)
    assert g.stats()["error_flags"] == 0
    g.destroy()


# ---- 4, 5, 6 ---------------------------------------------------------------------------------------------------------
def _flying(name, seed=3):
    """the scene at rest, flying along x and y fast enough for several re-sorts in a few dozen substeps of tl.DT"""
    cloths, links, X = lk.scene(name)
    x0 = X.copy()
    v0 = np.array([4.0, 0.3, 0.0], np.float32) + 0.05 * np.random.default_rng(seed).normal(size=x0.shape).astype(np.float32)
    return cloths, links, x0, v0


def _soft(g, links, dt, share=0.25):
    """the links with every k and c scaled so that dt is `share` of mpm_links_max_stable_dt"""
    out = links.copy()
    for _ in range(3):
        g.set_links(out)
        s = share * g.links_max_stable_dt() / dt
        if abs(s - 1.0) < 1e-3:
            break
        # (W scales with k and G with c: scaling k by s^2 and c by s scales the limit by 1 / s)
        out["stiffness"] *= np.float32(s * s)
        out["damping"] *= np.float32(s)
    g.set_links(out)
    assert abs(share * g.links_max_stable_dt() / dt - 1.0) < 1e-2
    return out


def test_links_that_do_nothing_add_an_exact_zero():
    """every link a slack tension-only cord, L twice the largest distance the run reaches, against the same links with
    k = c = 0: both engines run the same kernels, and after the same substeps through re-sorts x, v, C, F are bit-equal"""
    cloths, links, x0, v0 = _flying("mixed")
    n = 40
    ref = hs.engine(cloths)
    hs.upload(ref, x0, v0)
    reach = 0.0
    for _ in range(4):                      # (the plain engine's trajectory is the two others': the links do nothing)
        ref.run_substeps(n // 4, tl.DT, -1)
        x = hs.vertices(ref, hs.ARR().POSITIONS).astype(np.float64)
        reach = max(reach, float(np.linalg.norm(x[links["b"]] - x[links["a"]], axis=1).max()))
    ref.destroy()
    cords, nulls = links.copy(), links.copy()
    cords["flags"], cords["rest_length"] = lk.TENSION, np.float32(2 * reach)
    cords["stiffness"], cords["damping"] = 1e-6, 1e-9        # (soft: the stability guard lets tl.DT pass)
    nulls["stiffness"] = nulls["damping"] = 0.0
    es = [hs.engine(cloths) for _ in range(2)]
    es[0].set_links(cords)
    es[1].set_links(nulls)
    before = es[0].stats()["rebuilds"]
    for g in es:
        assert g.links_max_stable_dt() > tl.DT
        hs.upload(g, x0, v0)
        for _ in range(4):
            g.run_substeps(n // 4, tl.DT, -1)
        g.gpu_sync()
        assert g.stats()["error_flags"] == 0, g.stats()
    assert es[0].stats()["rebuilds"] - before >= 1, es[0].stats()
    assert not es[0].link_forces().any()
    assert np.linalg.norm(np.diff(hs.vertices(es[0], hs.ARR().POSITIONS)[[links["a"], links["b"]]], axis=0)[0], axis=1).max() < 2 * reach
    hs.same_bits(hs.state(es[0]), hs.state(es[1]), "slack cords against k = c = 0")
    for g in es:
        g.destroy()


def test_scheduling_through_resorts():
    """the linked sheets fly through several re-sorts, deterministic: run_substeps(n), n x substep and n x the five phase
    calls give the same bits in x, v, C and F -- a force added twice under the gate would not"""
    cloths, links, x0, v0 = _flying("mixed")
    n = 60
    es = [hs.engine(cloths) for _ in range(3)]
    for g in es:
        _soft(g, links, tl.DT)
        hs.upload(g, x0, v0)
    before = es[0].stats()["rebuilds"]
    es[0].run_substeps(n, tl.DT, -1)
    for _ in range(n):
        es[1].substep(tl.DT, -1)
    for _ in range(n):
        g = es[2]
        g.rebuild_mapping(False)
        g.calc_fem_state_and_force(tl.DT)
        g.particle_to_grid(tl.DT)
        g.update_grid(-1)
        g.grid_to_particle(tl.DT)
    for g in es:
        g.gpu_sync()
        assert g.stats()["error_flags"] == 0, g.stats()
    assert es[0].stats()["rebuilds"] - before >= 3, es[0].stats()
    s = [hs.state(g) for g in es]
    hs.same_bits(s[0], s[1], "run_substeps(n) against n substeps")
    hs.same_bits(s[0], s[2], "run_substeps(n) against the phase calls")
    assert es[0].link_forces().any()
    for g in es:
        g.destroy()


def test_coupled_path_runs():
    from drake_amd import Collider
    cloths, links, X = lk.scene("mixed")
    g = hs.engine(cloths, bodies=1)
    _soft(g, links, tl.DT)
    x0 = X.copy()
    hs.upload(g, x0)
    floor = [Collider(0, body=0, p_WB=(0.5, 0.5, float(x0[:, 2].min()) - 0.002))]
    res = g.run_coupled_substeps(40, tl.DT, floor, 0.5, 1e5, 1e-4)
    g.gpu_sync()
    assert g.stats()["error_flags"] == 0
    assert max(r["contacts"] for r in res) > 0, "the sheets never reached the floor"
    assert np.isfinite(g.download(hs.ARR().VELOCITIES)).all()
    g.destroy()


def test_off_means_off():
    """40 deterministic substeps through re-sorts: never set == set and cleared, to the bit, and with the same number of
    re-sort check launches (the quiet-time hint is in use again)"""
    cloths, links, x0, v0 = _flying("seam")
    es = [hs.engine(cloths) for _ in range(2)]
    es[1].set_links(links)
    assert es[1].links_max_stable_dt() < np.inf and len(es[1].get_links()) == len(links)
    es[1].set_links(links[:0])
    assert len(es[1].get_links()) == 0 and es[1].links_max_stable_dt() == np.inf and not es[1].link_forces().any()
    before = es[0].stats()["rebuilds"]
    for g in es:
        hs.upload(g, x0, v0)
        for _ in range(4):
            g.run_substeps(10, tl.DT, -1)
        g.gpu_sync()
        assert g.stats()["error_flags"] == 0
    assert es[0].stats()["rebuilds"] - before >= 2, es[0].stats()
    hs.same_bits(hs.state(es[0]), hs.state(es[1]), "set and cleared")
    assert es[0].stats()["resort_checks"] == es[1].stats()["resort_checks"]
    for g in es:
        g.destroy()


# ---- 7 -------------------------------------------------------------------------------------------------------------
def test_seamed_strips_close_their_gap():
    """Zero gravity, two coplanar strips of 4 x 24 vertices at rest, a gap g0 of 8 spacings (4 cells: the strips share no
    grid node at the start) apart along x, their facing edges seamed by 24 links with L = 0.  dt = 1e-3 is a quarter of
    mpm_links_max_stable_dt, which fixes k.
    * Softness.  A strip's axial stiffness is K = M c^2 / w^2 (M its mass, w = 3 spacings its width, c^2 =
      E / (rho (1 - nu^2)) the membrane's plane-stress wave speed squared); the seam's is n k.  The test states K / (n k)
      and asserts that it is above 10: the seam is the soft spring of the system.
    * Rigid-pair estimate: T = 2 pi sqrt(mu / (n k)), mu the reduced mass of the two strips.  After a quarter of T the
      mean seam gap is below g0 / 2 (the rigid estimate predicts 0; the factor 2 covers the strips' own compliance).
    * The twin without links keeps its gap: its only force is what the rounding of the positions leaves (the bound of
      tests/test_bending_gpu.py: a strain of at most s = 8 u max|x| / h per face, an acceleration 16 (lambda + 2 mu) /
      rho s / h).
    * Momentum.  CalcFemStateAndForce replaces a face particle's velocity by its corners' mean, which changes sum m v
      (DESIGN.md section 3.3f), so what the forces add is measured from after the FEM call to after GridToParticle of the
      same substep.  Per substep it stays within 128 u sum m |v| (the two transfers' roundings, as in
      tests/test_bending_gpu.py) + dt u (sum_i n_i sum S, the rounding of the link rows' additions: every link's two
      halves cancel to the bit, + 16 sum_i |f_i| for the membrane's, f the total vertex forces)."""
    A = hs.ARR()
    n, m, h, dt = 4, 24, lk.H0, 1e-3
    g0 = 8 * h
    sa = lk.sheet(n, m, (0.375, 0.375, 0.5))
    sb = lk.sheet(n, m, (0.375 + (n - 1) * h + g0, 0.375, 0.5))
    X = np.concatenate([sa[0], sb[0]])
    base = lk.make_links([((n - 1) * m + j, n * m + j, 1.0, 0.0, 0.0, 0) for j in range(m)])
    mat = dict(gravity=0.0)
    a, b = hs.engine([sa, sb], material=mat), hs.engine([sa, sb], material=mat)
    links = _soft(a, base, dt)
    k = float(links["stiffness"][0])
    assert abs(a.links_max_stable_dt() / (4 * dt) - 1.0) < 1e-2
    mass, pids = a.download(A.MASSES).astype(np.float64), a.download(A.PIDS)
    tri_cloth = (a._tri[:, 0] >= n * m).astype(int)
    cloth = np.concatenate([tri_cloth, (np.arange(2 * n * m) >= n * m).astype(int)])[pids]
    M = np.array([mass[cloth == 0].sum(), mass[cloth == 1].sum()])
    mu = M[0] * M[1] / M.sum()
    T = 2 * np.pi * np.sqrt(mu / (m * k))
    steps = int(np.ceil(0.25 * T / dt))
    mt = a.default_material()
    c2 = mt.youngs_modulus / (mt.density * (1 - mt.poisson_ratio ** 2))
    softness = (M[0] * c2 / ((n - 1) * h) ** 2) / (m * k)
    print(f"seam: k = {k:.4g} N/m per link, T = {T:.4g} s = {T / dt:.1f} substeps, strip / seam stiffness = {softness:.1f}")
    assert softness > 10, softness

    def momentum(g):
        mm, v = g.download(A.MASSES).astype(np.float64), g.download(A.VELOCITIES).astype(np.float64)
        return (mm[:, None] * v).sum(axis=0), float((mm[:, None] * np.abs(v)).sum(axis=0).max())

    added, bound = np.zeros(3), 0.0
    for _ in range(steps):
        a.rebuild_mapping(False)
        a.calc_fem_state_and_force(dt)
        p0, _ = momentum(a)
        f = hs.vertices(a, A.FORCES).astype(np.float64)
        _, _, acc = lk.vertex_forces64(links, hs.vertices(a, A.POSITIONS), hs.vertices(a, A.VELOCITIES), len(X))
        a.particle_to_grid(dt)
        a.update_grid(-1)
        a.grid_to_particle(dt)
        p1, gross = momentum(a)
        added += p1 - p0
        bound += 128 * U * gross + dt * U * float(acc.sum() + 16 * np.abs(f).max(axis=1).sum())
    b.run_substeps(steps, dt, -1)
    for g in (a, b):
        g.gpu_sync()
        assert g.stats()["error_flags"] == 0
    gap = lambda g: float(np.diff(hs.vertices(g, A.POSITIONS)[[links["a"], links["b"]]][:, :, 0], axis=0).mean())   # noqa: E731
    ga, gb = gap(a), gap(b)
    print(f"seam: mean gap {g0:.5f} -> {ga:.5f} after {steps} substeps (g0 / 2 = {g0 / 2:.5f}); the twin's {gb:.5f}")
    hs.record("links: mean seam gap after T / 4 over g0 / 2", ga / (g0 / 2))
    assert ga < g0 / 2, (ga, g0)
    mom = float(np.abs(added).max())
    print(f"seam: momentum added by the substeps {mom:.3e}, bound {bound:.3e}")
    hs.record("links: momentum of the seamed strips", mom / bound)
    assert mom <= bound, (mom, bound)
    lam = mt.youngs_modulus * mt.poisson_ratio / ((1 + mt.poisson_ratio) * (1 - 2 * mt.poisson_ratio))
    mu_l = mt.youngs_modulus / (2 * (1 + mt.poisson_ratio))
    s = 8 * U * float(np.abs(X).max()) / h
    still = 0.5 * (16 * (lam + 2 * mu_l) / mt.density * s / h) * (steps * dt) ** 2
    moved = abs(gb - g0)
    hs.record("links: the twin without links", moved / (2 * still))
    assert moved <= 2 * still, (moved, still)
    for g in (a, b):
        g.destroy()


# ---- 8 -------------------------------------------------------------------------------------------------------------
def test_refusals():
    from drake_amd import Collider, GpuMpm, MpmError

    def refused(call, says=None):
        with pytest.raises(MpmError) as e:
            call()
        assert e.value.code == -1, e.value
        if says:
            assert says in str(e.value), e.value

    cloths, links, X = lk.scene("seam")
    nv = len(X)
    # before Finalize
    g0 = GpuMpm(6)
    for Xc, T in cloths:
        g0.add_qr_cloth(Xc, np.zeros_like(Xc), T)
    refused(lambda: g0.set_links(links), says="finalize")
    g0.destroy()

    g = hs.engine(cloths, bodies=1)
    good = _soft(g, links, tl.DT, share=0.9)
    lim = g.links_max_stable_dt()
    x0, v0 = lk.state("random", "seam", X)
    hs.upload(g, x0, v0)
    f_before = g.link_forces()

    def bad(**kw):
        t = good.copy()
        for key, val in kw.items():
            t[key][3] = val
        return t

    for t in (bad(a=nv), bad(b=nv + 7), bad(a=int(good["b"][3])), bad(stiffness=-1.0), bad(stiffness=np.nan),
              bad(rest_length=-1e-3), bad(rest_length=np.inf), bad(damping=-0.1), bad(damping=np.nan), bad(flags=2),
              bad(flags=0x80000001)):
        refused(lambda t=t: g.set_links(t), says="link 3")
        assert np.array_equal(g.get_links(), good) and g.links_max_stable_dt() == lim
    # a table that does not fit 2^31 records is refused by its count, before a link is read
    assert g.lib.mpm_set_links(g.h, 1 << 30, good.ctypes.data) == -1 and "too large" in g.lib.mpm_last_error().decode()
    assert np.array_equal(g.get_links(), good) and g.links_max_stable_dt() == lim
    assert np.array_equal(hs.bits(g.link_forces()), hs.bits(f_before))
    # partitioned, halo, team and chain calls on an engine with links
    nb = 64 // 4
    refused(lambda: g.dist_init(0, 1, [0, nb], 2, 2, 2), says="links")
    refused(lambda: g.substep_mid_halo(tl.DT), says="links")
    refused(lambda: g.team_prepare(), says="links")
    refused(lambda: g.chain_substeps(1, tl.DT), says="links")
    # a dt above the limit: every entry point that takes one, nothing enqueued
    before = g.stats()["substeps"]
    big = 1.01 * lim
    floor = [Collider(0, body=0, p_WB=(0.5, 0.5, 0.3))]
    for call in (lambda: g.run_substeps(2, big, -1), lambda: g.substep(big, -1), lambda: g.particle_to_grid(big),
                 lambda: g.profile_substeps(2, big, -1), lambda: g.run_coupled_substeps(2, big, floor, 0.5, 1e5, 1e-4),
                 lambda: g.substep_begin(big)):
        refused(call, says="mpm_links_max_stable_dt")
    assert g.stats()["substeps"] == before
    # the limit is the restatement's
    mass = hs.vertices(g, hs.ARR().MASSES).astype(np.float64)
    assert abs(lim / lk.max_stable_dt(good, mass) - 1.0) < 1e-5
    g.run_substeps(2, tl.DT, -1)
    ph, _ = g.profile_substeps(2, tl.DT, -1)
    assert ph["vforce"] > 0.0, ph          # (k_vforce and k_link are timed under MPM_PHASE_VFORCE)
    g.gpu_sync()
    assert g.stats()["error_flags"] == 0
    # an empty table lifts the refusals; a partitioned engine refuses the call
    g.set_links(good[:0])
    g.run_substeps(1, big, -1)
    g.dist_init(0, 1, [0, nb], 2, 2, 2)
    refused(lambda: g.set_links(good), says="partitioned")
    assert len(g.get_links()) == 0
    g.destroy()
