"""Shell bending about a curved rest shape (mpm_set_shell_bending) on the engine.

1. mpm_shell_forces per vertex, psi per hinge and the energy per cloth against the float64 model of
   tests/shell_bending.py on every mesh x state, within R_i 2^-24 B_i (R_i = 46 + n_i, counted in mpm_shell.h), psi
   within 13 (kappa_A + kappa_B) (1 + |psi|) 2^-24, the energy within the same psi bound carried through the square.
   The hinge table is the model's; kc is float(k cbar) within a rounding; psibar is the device's psi of the rest shape.
   Exact zeros on the rest shape; one inactive hinge and exact zeros where x2 lies on the edge.  The same bits after
   forced re-sorts and after mpm_rebuild_mapping(sort = 1).
2. Translation invariance to the bit.
3. MPM_ARR_FORCES of an engine with it minus a twin's without is mpm_shell_forces, within one rounding of the sum.
4. Scheduling: run_substeps(n), the five phase calls and run_coupled_substeps with a collider nobody touches are
   bit-equal through re-sorts.
5. Off means off, to the bit and to the launch count of the re-sort checks.
6. Refusals, the old table staying in force; a dt above the guard is refused before anything is enqueued.
7. One short run with every other feature.
8. Dynamics: a rolled rest shape curls a flat sheet; a tube keeps its shape under this model and not under the flat one."""
import numpy as np
import pytest

from tests import bending as bd
from tests import harness as hs
from tests import shell_bending as sb
from tests import shell_scenes as ss
from tests import transfer_layouts as tl

pytestmark = pytest.mark.gpu

U = sb.U
DT = 2e-4


def _check(g, H, what, cloth_of_hinge=None, n_cloths=1):
    """forces, psi, energies and the inactive count of the engine on its own positions against the float64 model with the
    engine's own kc and psibar (checked by the caller); returns (x, f, psi, energies)"""
    x32 = hs.vertices(g, hs.ARR().POSITIONS)
    ids, kc, psibar = g.shell_hinges()
    assert np.array_equal(ids, H)
    f = g.shell_forces()
    E, psi, inactive = g.shell_state()
    assert np.isfinite(f).all() and np.isfinite(psi).all() and np.isfinite(E).all()
    if len(H) == 0:
        assert not f.any() and not E.any() and inactive == 0
        return x32, f, psi, E
    on = sb.active(x32, H)
    assert inactive == int((~on).sum()), (what, inactive, on)
    x = x32.astype(np.float64)
    B, N, pb = sb.bound(x, H, kc, psibar, on)
    w = sb.margin(f - sb.force64(x, H, kc, psibar, on), B, sb.R_SHELL + N)
    wp = sb.margin(psi - sb.hinge_forces64(x, H, kc, psibar, on)[1], pb, sb.R_PSI)
    E64, Eb = sb.energy64(x, H, kc, psibar, on), sb.energy_bound(x, H, kc, psibar, on)
    ch = np.zeros(len(H), int) if cloth_of_hinge is None else cloth_of_hinge
    we = 0.0
    for c in range(n_cloths):
        err, tol = abs(float(E[c]) - E64[ch == c].sum()), Eb[ch == c].sum() + 1e-15 * E64[ch == c].sum()
        we = max(we, err / tol if err > 0 else 0.0)
    print(f"shell bending: {what}: force {w:.3g}, psi {wp:.3g}, energy {we:.3g} of the bound; inactive {inactive}")
    hs.record(f"shell forces: {what}", w)
    hs.record(f"shell psi: {what}", wp)
    hs.record(f"shell energy: {what}", we)
    assert w <= 1.0 and wp <= 1.0 and we <= 1.0, (what, w, wp, we)
    assert not f[N == 0].any() and not psi[~on].any()
    return x32, f, psi, E


def _check_table(g, name, k):
    """kc is float(k cbar) within a rounding of the float64 cbar; psibar is psi of the rest shape within psi's bound"""
    X, T, rest = sb.mesh(name)
    H = sb.hinges(T)
    ids, kc, psibar = g.shell_hinges()
    assert np.array_equal(ids, H) and len(kc) == len(H)
    if len(H):
        xr = sb.rest_shape(name).astype(np.float64)
        want = float(np.float32(k)) * sb.cbar64(xr, H)
        assert np.abs(kc - want).max() <= 1.0001 * U * np.abs(want).max() and (np.abs(kc - want) <= 1.0001 * U * np.abs(want)).all()
        _, _, pb = sb.bound(xr, H, kc, psibar)
        assert (np.abs(psibar - sb.psi64(xr, H)) <= sb.R_PSI * U * pb).all()
    return H


# ---- 1 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,st", sb.CASES)
def test_forces_psi_and_energy_against_float64(name, st):
    from drake_amd import SHELL_DTYPE
    X, T, rest = sb.mesh(name)
    g = hs.engine([(X, T)])
    g.set_shell_bending([sb.K], rest)
    want = np.zeros(1, SHELL_DTYPE)
    want["stiffness"] = sb.K
    assert np.array_equal(g.get_shell_bending(), want)
    H = _check_table(g, name, sb.K)
    assert (g.shell_max_stable_dt() < np.inf) == (len(H) > 0)
    x0 = sb.state(name, st)
    hs.upload(g, x0)
    x, f0, psi0, E0 = _check(g, H, f"{name} {st}")
    assert np.array_equal(x, x0)
    if st == "rest":
        assert not f0.any() and not E0.any() and np.array_equal(hs.bits(psi0), hs.bits(g.shell_hinges()[2]))     # every float is +-0
    elif st == "collinear":
        assert g.shell_state()[2] == 1 and not f0.any() and not psi0.any()
    elif len(H) and st != "rigid":
        assert f0.any()
    # substeps that force a re-sort: the state five cells further along x, two short substeps (not from `collinear`, whose
    # face of zero area the membrane model cannot step)
    if st != "collinear":
        before = g.stats()["rebuilds"]
        hs.upload(g, x0 + np.array([5.0 / 64, 0.0, 0.0], np.float32))
        g.run_substeps(2, 1e-5, -1)
        g.gpu_sync()
        assert g.stats()["error_flags"] == 0 and g.stats()["rebuilds"] > before, g.stats()
        _check(g, H, f"{name} {st} after a re-sort")
    # the first state again, in the new particle order: the same bits
    for sort in (False, True):
        if sort:
            g.rebuild_mapping(True)
        hs.upload(g, x0)
        f1 = g.shell_forces()
        E1, psi1, _ = g.shell_state()
        assert np.array_equal(hs.bits(f1), hs.bits(f0)), (sort, float(np.abs(f1 - f0).max()))
        assert np.array_equal(hs.bits(psi1), hs.bits(psi0)) and np.array_equal(hs.bits(E1), hs.bits(E0))
    assert g.stats()["error_flags"] == 0
    g.destroy()


def test_flat_rest_option_and_both_models_on_one_cloth():
    """MPM_SHELL_REST_FLAT: psibar = 0 and cbar from the mesh as added whatever rest_pos says; mpm_set_bending beside it
    adds its own force"""
    from drake_amd import SHELL_DTYPE, SHELL_REST_FLAT
    A = hs.ARR()
    X, T, rest = sb.mesh("book")
    H = sb.hinges(T)
    g = hs.engine([(X, T)])
    t = np.zeros(1, SHELL_DTYPE)
    t["stiffness"], t["rest"] = sb.K, SHELL_REST_FLAT
    g.set_shell_bending(t, rest)
    ids, kc, psibar = g.shell_hinges()
    want = float(np.float32(sb.K)) * sb.cbar64(X.astype(np.float64), H)
    assert not psibar.any() and (np.abs(kc - want) <= 1.0001 * U * want).all() and np.array_equal(g.get_shell_bending(), t)
    hs.upload(g, rest)
    _, f, psi, E = _check(g, H, "book, flat rest shape, folded")
    assert f.any() and abs(np.abs(psi).max() - 2 * np.sin(0.5)) < 1e-4 and E[0] > 0
    # with the quadratic model beside it: MPM_ARR_FORCES carries both (against a twin with the quadratic model alone)
    b = hs.engine([(X, T)])
    out = []
    for e in (g, b):
        e.set_bending([sb.K])
        hs.upload(e, rest)
        e.rebuild_mapping(False)
        e.calc_fem_state_and_force(1e-5)
        out.append(hs.vertices(e, A.FORCES).astype(np.float64))
    err = np.abs(out[0] - (out[1] + f.astype(np.float64)))
    assert g.bending_forces().any() and np.array_equal(hs.bits(g.shell_forces()), hs.bits(f)) and (err <= U * np.abs(out[0])).all()
    for e in (g, b):
        assert e.stats()["error_flags"] == 0
        e.destroy()


# ---- 2 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["jittered", "tube", "icosphere2"])
def test_translation_invariance_to_the_bit(name):
    X, T, rest = sb.mesh(name)
    g = hs.engine([(X, T)])
    g.set_shell_bending([sb.K], rest)
    x0 = (np.round(sb.state(name, "perturbed").astype(np.float64) * 2.0 ** 16) / 2.0 ** 16).astype(np.float32)
    x1 = x0 + np.array([2.0 ** -4, -2.0 ** -4, 2.0 ** -4], np.float32)
    assert np.array_equal(x1.astype(np.float64) - x0.astype(np.float64), np.broadcast_to([2.0 ** -4, -2.0 ** -4, 2.0 ** -4], x0.shape))
    out = []
    for x in (x0, x1):
        hs.upload(g, x)
        assert np.array_equal(hs.vertices(g, hs.ARR().POSITIONS), x)
        out.append((g.shell_forces(), g.shell_state()))
    assert out[0][0].any() and np.array_equal(hs.bits(out[0][0]), hs.bits(out[1][0]))
    assert np.array_equal(hs.bits(out[0][1][1]), hs.bits(out[1][1][1])) and np.array_equal(hs.bits(out[0][1][0]), hs.bits(out[1][1][0]))
    assert g.stats()["error_flags"] == 0
    g.destroy()


# ---- the two-cloth scene of the scheduling tests ---------------------------------------------------------------------------
# ---- 3 -------------------------------------------------------------------------------------------------------------------
def test_total_forces_include_the_shell_force():
    A = hs.ARR()
    cloths, rest, H, ch = ss.scene()
    a, b = hs.engine(cloths), hs.engine(cloths)
    a.set_shell_bending([sb.K, 2 * sb.K], rest)
    x0 = bd.perturbed(rest, seed=7).astype(np.float32)
    out = []
    for g in (a, b):
        hs.upload(g, x0)
        g.rebuild_mapping(False)
        g.calc_fem_state_and_force(1e-5)
        out.append(hs.vertices(g, A.FORCES))
    _check(a, H, "tube and book, perturbed", ch, 2)
    fs = a.shell_forces()
    assert fs.any() and out[1].any()
    tot = out[1].astype(np.float64) + fs.astype(np.float64)
    err = np.abs(out[0].astype(np.float64) - tot)
    w = float((err / np.maximum(U * np.abs(out[0]).astype(np.float64), 1e-300))[err > 0].max()) if (err > 0).any() else 0.0
    print(f"total forces: {w:.3g} of one rounding of the sum")
    hs.record("shell: total forces", w)
    assert w <= 1.0, w
    assert not b.shell_forces().any() and b.shell_max_stable_dt() == np.inf
    for g in (a, b):
        assert g.stats()["error_flags"] == 0
        g.destroy()


# ---- 4, 5 ----------------------------------------------------------------------------------------------------------------
def test_scheduling_through_resorts():
    """the tube and the book fly through several re-sorts, deterministic: run_substeps(n), n x the five phase calls and
    run_coupled_substeps(n) with a collider nobody touches give the same bits in x, v, C and F -- a force added twice
    under the gate, or hinge records left from another substep, would not -- and the same psi and energies"""
    from drake_amd import Collider
    cloths, rest, H, ch, x0, v0 = ss.flying()
    n = 40
    es = [hs.engine(cloths, bodies=1) for _ in range(3)]
    k = ss.scale_k(es[0], lambda k: es[0].set_shell_bending([k, k], rest), tl.DT)
    for g in es:
        g.set_shell_bending([k, k], rest)
        hs.upload(g, x0 + 0.05 * sb.H0 * np.random.default_rng(1).normal(size=x0.shape).astype(np.float32), v0)
    before = es[0].stats()["rebuilds"]
    es[0].run_substeps(n, tl.DT, -1)
    for _ in range(n):
        g = es[1]
        g.rebuild_mapping(False)
        g.calc_fem_state_and_force(tl.DT)
        g.particle_to_grid(tl.DT)
        g.update_grid(-1)
        g.grid_to_particle(tl.DT)
    far = [Collider(1, body=0, p_WB=(0.9, 0.1, 0.1), dims=(0.02, 0, 0))]
    res = es[2].run_coupled_substeps(n, tl.DT, far, 0.5, 1e5, 1e-4)
    assert max(r["contacts"] for r in res) == 0
    for g in es:
        g.gpu_sync()
        assert g.stats()["error_flags"] == 0, g.stats()
    assert es[0].stats()["rebuilds"] - before >= 2, es[0].stats()
    s = [hs.state(g) for g in es]
    hs.same_bits(s[0], s[1], "run_substeps(n) against the phase calls")
    hs.same_bits(s[0], s[2], "run_substeps(n) against the coupled path")
    ps = [g.shell_state() for g in es]
    for q in ps[1:]:
        assert np.array_equal(hs.bits(q[0]), hs.bits(ps[0][0])) and np.array_equal(hs.bits(q[1]), hs.bits(ps[0][1])) and q[2] == ps[0][2]
    assert es[0].shell_forces().any() and np.isfinite(s[0]["v"]).all()
    _check(es[0], H, "tube and book after 40 substeps in flight", ch, 2)
    ph, _ = es[0].profile_substeps(2, tl.DT, -1)
    assert ph["vforce"] > 0.0, ph          # (k_vforce and the hinge kernels are timed under MPM_PHASE_VFORCE)
    for g in es:
        g.destroy()


def test_off_means_off():
    """40 deterministic substeps through re-sorts: never set == set and cleared, to the bit, and with the same number of
    re-sort check launches (the quiet-time hint is in use again); an all-zero table is off as well"""
    cloths, rest, H, ch, x0, v0 = ss.flying()
    es = [hs.engine(cloths) for _ in range(3)]
    es[1].set_shell_bending([sb.K, sb.K], rest)
    hs.upload(es[1], bd.perturbed(rest, seed=7).astype(np.float32))
    assert es[1].shell_forces().any() and es[1].shell_max_stable_dt() < np.inf
    es[1].set_shell_bending([])
    es[2].set_shell_bending([sb.K, sb.K], rest)
    es[2].set_shell_bending([0.0, 0.0], rest)
    for g in es[1:]:
        assert not g.get_shell_bending()["stiffness"].any() and len(g.get_shell_bending()) == 2 and not g.shell_forces().any()
        assert g.shell_max_stable_dt() == np.inf and len(g.shell_hinges()[1]) == 0
    before = es[0].stats()["rebuilds"]
    for g in es:
        hs.upload(g, x0, v0)
        for _ in range(4):
            g.run_substeps(10, tl.DT, -1)
        g.gpu_sync()
        assert g.stats()["error_flags"] == 0
    assert es[0].stats()["rebuilds"] - before >= 2, es[0].stats()
    for g in es[1:]:
        hs.same_bits(hs.state(es[0]), hs.state(g), "set and cleared")
        assert es[0].stats()["resort_checks"] == g.stats()["resort_checks"]
    for g in es:
        g.destroy()


# ---- 6 -------------------------------------------------------------------------------------------------------------------
def test_refusals_and_the_guard():
    from drake_amd import SHELL_DTYPE, Collider, GpuMpm, MpmError

    def refused(call, says=()):
        with pytest.raises(MpmError) as e:
            call()
        assert e.value.code == -1, e.value
        for s in (says,) if isinstance(says, str) else says:
            assert s in str(e.value), e.value

    cloths, rest, H, ch = ss.scene()
    # before Finalize
    g0 = GpuMpm(6)
    for Xc, Tc in cloths:
        g0.add_qr_cloth(Xc, np.zeros_like(Xc), Tc)
    refused(lambda: g0.set_shell_bending([sb.K, sb.K]), says="finalize")
    g0.destroy()

    g = hs.engine(cloths, bodies=1)
    k = ss.scale_k(g, lambda k: g.set_shell_bending([k, k], rest), tl.DT, share=0.9)
    good = g.get_shell_bending()
    lim = g.shell_max_stable_dt()
    hs.upload(g, bd.perturbed(rest, seed=7).astype(np.float32))
    f_before, s_before, t_before = g.shell_forces(), g.shell_state(), g.shell_hinges()

    def table(ks, rests=(0, 0)):
        t = np.zeros(len(ks), SHELL_DTYPE)
        t["stiffness"], t["rest"] = ks, rests
        return t

    bad_rest = rest.copy()
    bad_rest[5, 1] = np.nan
    n0 = len(cloths[0][0])
    # the book's rest shape flat again, the third corner of its face 3 on the middle of the other two (exact on the sheet's
    # lattice): a zero rest area
    flat_face = rest.copy()
    flat_face[n0:] = cloths[1][0]
    i, j, m = cloths[1][1][3] + n0
    flat_face[m] = 0.5 * (flat_face[i] + flat_face[j])
    assert np.array_equal(flat_face[m].astype(np.float64), 0.5 * (flat_face[i].astype(np.float64) + flat_face[j]))
    zero_edge = rest.copy()                       # an interior edge of the tube collapsed
    h = H[np.flatnonzero(ch == 0)[7]]
    zero_edge[h[1]] = zero_edge[h[0]]
    calls = [
        (lambda: g.set_shell_bending([k]), "mpm_cloth_count"), (lambda: g.set_shell_bending([k, k, k]), "mpm_cloth_count"),
        (lambda: g.set_shell_bending([k, -k], rest), ("cloth 1", "stiffness")), (lambda: g.set_shell_bending([np.nan, k], rest), "cloth 0"),
        (lambda: g.set_shell_bending([k, np.inf], rest), "cloth 1"),
        (lambda: g.set_shell_bending(table([k, k], (0, 2)), rest), ("cloth 1", "rest")),
        (lambda: g.set_shell_bending(table([k, k], (0x80000000, 0)), rest), ("cloth 0", "rest")),
        (lambda: g.set_shell_bending([k, k], bad_rest), "rest_pos"),
        (lambda: g.set_shell_bending([k, k], flat_face), ("face", "zero rest area")),
        (lambda: g.set_shell_bending([k, k], zero_edge), "face"),
    ]
    for call, says in calls:
        refused(call, says=says)
        assert np.array_equal(g.get_shell_bending(), good) and g.shell_max_stable_dt() == lim
    # (the message names the face in the numbering of all faces: the book's faces come behind the tube's)
    with pytest.raises(MpmError) as e:
        g.set_shell_bending([k, k], flat_face)
    named = int(str(e.value).split("face ")[1].split()[0])
    assert named == len(cloths[0][1]) + 3
    # with k = 0 on the cloth nobody asks for its rest shape
    g.set_shell_bending([k, 0.0], flat_face)
    g.set_shell_bending([k, k], rest)
    assert np.array_equal(hs.bits(g.shell_forces()), hs.bits(f_before))
    s1, t1 = g.shell_state(), g.shell_hinges()
    assert all(np.array_equal(hs.bits(p), hs.bits(q)) for p, q in zip(s1[:2], s_before[:2])) and s1[2] == s_before[2]
    assert all(np.array_equal(hs.bits(p), hs.bits(q)) for p, q in zip(t1, t_before))
    # partitioned, halo, team and chain calls on an engine with shell bending
    nb = 64 // 4
    refused(lambda: g.dist_init(0, 1, [0, nb], 2, 2, 2), says="shell bending")
    refused(lambda: g.substep_mid_halo(tl.DT), says="shell bending")
    refused(lambda: g.team_prepare(), says="shell bending")
    refused(lambda: g.chain_substeps(1, tl.DT), says="shell bending")
    # a dt above the guard: every entry point that takes one, nothing enqueued
    before = g.stats()["substeps"]
    big = 1.01 * lim
    floor = [Collider(0, body=0, p_WB=(0.5, 0.5, 0.3))]
    for call in (lambda: g.run_substeps(2, big, -1), lambda: g.substep(big, -1), lambda: g.particle_to_grid(big),
                 lambda: g.profile_substeps(2, big, -1), lambda: g.run_coupled_substeps(2, big, floor, 0.5, 1e5, 1e-4),
                 lambda: g.substep_begin(big)):
        refused(call, says="mpm_shell_max_stable_dt")
    assert g.stats()["substeps"] == before
    g.run_substeps(2, tl.DT, -1)
    g.gpu_sync()
    assert g.stats()["error_flags"] == 0
    # off lifts the refusals; a partitioned engine refuses the call
    g.set_shell_bending([])
    g.run_substeps(1, big, -1)
    g.dist_init(0, 1, [0, nb], 2, 2, 2)
    refused(lambda: g.set_shell_bending([k, k], rest), says="partitioned")
    assert not g.get_shell_bending()["stiffness"].any()
    g.destroy()


# ---- 7 -------------------------------------------------------------------------------------------------------------------
FEATURES = ["pins", "materials", "force_fields", "bending", "damping", "links", "pressure", "default_engine", "fast_math", "coupled"]


@pytest.mark.parametrize("feature", FEATURES)
def test_works_with(feature):
    """the tube and the book, perturbed, with one other feature on: eight substeps, finite results, no error flag, and the
    shell forces still the model's"""
    from drake_amd import BodyMotion, Collider, ForceField, GpuMpm, Pin, links
    from tests import pressure as pr
    A = hs.ARR()
    cloths, rest, H, ch = ss.scene()
    mats = None
    if feature == "materials":      # (of the engine's float32 fields: the products round once, into the cloth's fields)
        m0 = GpuMpm.default_material()
        mats = [dict(youngs_modulus=m0.youngs_modulus * (1.0 + 0.25 * c), density=m0.density * (1.0 + 0.1 * c)) for c in range(len(cloths))]
    g = hs.engine(cloths, bodies=1, deterministic=feature != "default_engine", fast_math=True if feature == "fast_math" else None,
                  mats=mats)
    x0 = bd.perturbed(rest, seed=7).astype(np.float32)
    lims = []
    if feature == "pins":
        g.set_body_motions([BodyMotion(0, (0, 0, 0), np.eye(3).ravel(), (0, 0, 0), (0, 0, 0))])
        g.set_pins([Pin(v, 0, x0[v]) for v in (0, 30)])
    elif feature == "force_fields":
        g.set_force_fields([ForceField(u0=(0.3, 0.0, 0.5))])
    elif feature in ("bending", "damping"):
        g.set_bending([sb.K, sb.K])
        lims.append(g.bending_max_stable_dt())
        if feature == "damping":
            g.set_damping([(1e-5, 1e-5)] * 2)
            lims.append(g.damping_max_stable_dt())
    elif feature == "links":
        n0 = len(cloths[0][0])
        g.set_links(links([0, 1, 2], [n0, n0 + 1, n0 + 2], 0.5, 0.3, 0.001))
        lims.append(g.links_max_stable_dt())
    elif feature == "pressure":
        g.set_pressure(pr.make_table([(pr.CONSTANT, 20.0, 0, 0, 0), (pr.OFF, 0, 0, 0, 0)]))
    g.set_shell_bending([sb.K, sb.K], rest)
    dt = min([1e-4, 0.5 * g.shell_max_stable_dt()] + [0.5 * q for q in lims])
    hs.upload(g, x0)
    _check(g, H, f"with {feature}", ch, 2)
    if feature == "coupled":
        far = [Collider(1, body=0, p_WB=(0.9, 0.1, 0.1), dims=(0.02, 0, 0))]
        g.run_coupled_substeps(8, dt, far, 0.5, 1e5, 1e-4)
    else:
        g.run_substeps(6, dt, -1)
        for _ in range(2):
            g.substep(dt, -1)
    g.gpu_sync()
    assert g.stats()["error_flags"] == 0, g.stats()
    assert np.isfinite(g.download(A.VELOCITIES)).all() and np.isfinite(g.download(A.POSITIONS)).all()
    _check(g, H, f"with {feature}, after substeps", ch, 2)
    g.destroy()


# ---- 8 -------------------------------------------------------------------------------------------------------------------
def test_a_rolled_rest_shape_curls_a_flat_sheet():
    """Zero gravity, sheet(9, 8) added flat and at rest, rest_pos the sheet rolled onto a cylinder of radius 4 H0; dt is half
    of mpm_shell_max_stable_dt; 40 substeps.  sum_h (psi_h - psibar_h)^2 falls below its initial value, the mean of psi
    takes the sign of the mean of psibar, and the shell energy of mpm_shell_state falls.  Measured on an MI355X:
    sum (psi - psibar)^2 3.0466 -> 1.5743, mean psi 0 -> -1.904e-2 against mean psibar -7.986e-2, energy 3.4636e-2 ->
    1.8327e-2 J."""
    X, T = bd.sheet(9, 8)
    rest = bd.cylinder(X, 4 * sb.H0).astype(np.float32)
    g = hs.engine([(X, T)], material=dict(gravity=0.0))
    ss.scale_k(g, lambda k: g.set_shell_bending([k], rest), DT)
    _, _, psibar = g.shell_hinges()
    E0, psi0, _ = g.shell_state()
    assert not psi0.any() and np.abs(psibar).max() > 0.1 and E0[0] > 0
    g.run_substeps(40, DT, -1)
    g.gpu_sync()
    assert g.stats()["error_flags"] == 0
    E1, psi1, inactive = g.shell_state()
    d0, d1 = float(((psi0 - psibar).astype(np.float64) ** 2).sum()), float(((psi1 - psibar).astype(np.float64) ** 2).sum())
    print(f"curling: sum (psi - psibar)^2 {d0:.6e} -> {d1:.6e}; mean psi {psi1.mean():.4e}, mean psibar {psibar.mean():.4e}; "
          f"energy {E0[0]:.6e} -> {E1[0]:.6e}")
    assert inactive == 0 and np.isfinite(psi1).all()
    assert d1 < d0
    assert psi1.mean() != 0 and np.sign(psi1.mean()) == np.sign(psibar.mean())
    assert E1[0] < E0[0]
    g.destroy()


def test_a_tube_keeps_its_shape_under_this_model_and_not_under_the_flat_one():
    """Zero gravity, three twins of the tube at rest over 40 substeps, dt half of mpm_shell_max_stable_dt: no bending,
    mpm_set_bending(k), mpm_set_shell_bending(k).  The flat model's force on a tube is not zero, so its twin moves; the
    shell twin's largest vertex displacement must be at most a tenth of that, and no more than twice the twin's without
    bending plus 2^-20 H0.  Measured on an MI355X, the first run: none 0, flat 1.375109e-3 (17.6 % of H0), shell 0 -- the
    shell twin's forces are exact zeros, so nothing moves."""
    X, T, _ = sb.mesh("tube")
    es = [hs.engine([(X, T)], material=dict(gravity=0.0)) for _ in range(3)]
    k = ss.scale_k(es[2], lambda k: es[2].set_shell_bending([k]), DT)
    es[1].set_bending([k])
    assert es[1].bending_forces().any() and not es[2].shell_forces().any()
    moved = []
    for g in es:
        g.run_substeps(40, DT, -1)
        g.gpu_sync()
        assert g.stats()["error_flags"] == 0
        moved.append(float(np.abs(hs.vertices(g, hs.ARR().POSITIONS).astype(np.float64) - X).max()))
        g.destroy()
    none, flat, shell = moved
    print(f"tube: largest displacement after 40 substeps: none {none:.6e}, flat {flat:.6e}, shell {shell:.6e} (H0 = {sb.H0:.4e})")
    assert flat > 0
    assert shell <= 0.1 * flat, (shell, flat)
    assert shell <= 2 * none + 2.0 ** -20 * sb.H0, (shell, none)
