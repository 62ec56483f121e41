"""Every cloth feature at once on every host path that enqueues a substep (tests/test_feature_paths_gpu.py,
tests/test_feature_paths.py, scripts/substep_paths.py --features): the scene, the engine, the runners, the state that is
compared, and the float64 composition of the vertex-force chain.

The scene is that of tests/substep_paths.py -- GpuMpm(6), two sheets of 32 x 32 vertices and a fan of 12 faces, all moving
at 2 m/s along x: a cell every 16 substeps of DT, so re-sorts and owed substeps occur within the N substeps -- with a closed
cloth (the icosphere of tests/pressure.py, above the sheets) and every feature of the vertex-force chain
(launch_fem_vertices, mpm_engine.hip) and behind GridToParticle:

  cloth 0  sheet      material 0, membrane + hinge damping, quadratic bending, constant pressure, two pins on body 0
  cloth 1  sheet      material 1, membrane + hinge damping, quadratic bending AND shell bending about a rolled rest
                      shape, pressure off, two spring anchors to body 0
  cloth 2  icosphere  material 2, membrane damping, gas pressure, shell bending about its own shape, three cords to body 1
  cloth 3  fan        material 3, membrane damping, shell k = 0; its hub hangs on a cord from the icosphere, slack at first
  links    a seam of eight between the sheets, a hub of ten springs (a row longer than a batch of eight), a spring inside
           sheet 0, the cord
  bodies   0 translates with the cloth; 1 translates and spins; 2 is the contact collider's (a floor)
  field    linear drag against a wind u0

Every stiffness is set, its guard read, and rescaled so that DT is SHARE (a hair under one half, so that the rounding of
the guard itself cannot break DT <= guard / 2) of the guard: once, on a probe engine with everything on (PARAMS); every
other engine gets the same numbers, so that the engines of a composition differ in what is switched on and in nothing
else.  No GPU is touched at import."""
import numpy as np

from tests import harness
from tests import substep_paths as sp

DT = sp.DT
N = sp.N
BATCHES = sp.BATCHES
SHARE = 0.499
U = 2.0 ** -24                    # one rounding of a float sum, as the per-feature test_total_forces_include_* use it
DX = 1.0 / 64
RES = 32
NV_SHEET = RES * RES

FEATURES = ("materials", "damping", "bending", "bend_damping", "links", "pressure", "shell", "anchors", "pins", "fields")
EVERYTHING = frozenset(FEATURES)
NOTHING = frozenset()
# the stages behind k_vforce in launch order (launch_fem_vertices: k_bend, k_bend_damp, k_link, k_pressure_volume /
# k_pressure_gauge / k_pressure, k_hinge / k_hinge_gather, k_anchor_pose / k_anchor)
CHAIN = ("bending", "bend_damping", "links", "pressure", "shell", "anchors")
FACE_PASS = frozenset(("materials", "damping"))      # (k_fem_mat, k_damp: in every engine of a composition)

ICO_CENTRE = (0.5, 0.5, 0.66)
BODY0_V = (2.0, 0.0, 0.0)
BODY1_P, BODY1_V, BODY1_W = (0.5, 0.5, 0.72), (2.0, 0.0, 0.0), (0.0, 0.0, 3.0)
FLOOR_Z = 0.4985                  # tests/substep_paths._coupled's: the lower sheet reaches it after ~35 substeps
FAR = (0.9, 0.1, 0.1)             # a sphere nothing reaches
MU, K_CT, D_CT = 0.5, 1e5, 1e-3   # the contact parameters of tests/substep_paths._coupled
PINS = (0, RES - 1)                                   # vertices of sheet 0
SPRING_ANCHORS = (NV_SHEET, NV_SHEET + RES - 1)       # vertices of sheet 1
HUB = 500                                             # of sheet 0: ten springs into sheet 1
# (MPM_RESORT_EVERY, MPM_QUIET_FACTOR: the re-sort checks of mpm_run_substeps -- with no trust in the quiet time and a check
# with every 12th substep only, substeps meet a pending re-sort without their check, skip themselves and are owed; not 16:
# the cloth crosses a cell in 16 substeps, and a check that falls on the substep behind the one that asks for the re-sort
# leaves nothing to skip)
ENV_SWITCHES = ("MPM_DEFER_PHASES", "MPM_CT_GATE_ALWAYS", "MPM_CT_NO_WATCH", "MPM_RESORT_EVERY", "MPM_QUIET_FACTOR")
SPARSE_CHECKS = {"MPM_RESORT_EVERY": "12", "MPM_QUIET_FACTOR": "0"}

_SCENE = {}
PARAMS = {}


def chain_features(k):
    """the features of E_k: the face pass and the first k stages of the chain"""
    return FACE_PASS | frozenset(CHAIN[:k])


# ---- the scene, engine-free ---------------------------------------------------------------------------------------------
def _rolled(X, radius=0.5):
    """a sheet rolled about the line x = its first column, z = its plane, onto a cylinder of `radius` (float64)"""
    X = np.asarray(X, np.float64).copy()
    x0, z0 = X[:, 0].min(), X[:, 2].mean()
    a = (X[:, 0] - x0) / radius
    X[:, 0] = x0 + radius * np.sin(a)
    X[:, 2] = z0 + (X[:, 2] - z0) + radius * (1.0 - np.cos(a))
    return X


def scene():
    """dict: cloths [(pos, vel, T (n, 3))] in cloth order, first (vertex offsets, n_cloths + 1), X / V of all vertices as
    added, T of all faces in global vertex ids, cv / cf cloth of vertex / face, rest (the shell's rest positions), the link,
    anchor and pressure tables with unit-free base values (link_base, anchor_base: stiffness and damping per unit mass and
    DT, scaled by `params`), the pins, the motions of bodies 0 and 1 as tests/anchors.py states them, and `cord`, the
    index of the slack cord in the link table."""
    if _SCENE:
        return _SCENE
    from tests import anchors as an
    from tests import links as lk
    from tests import pressure as pr
    sh = sp.sheets(True)                      # sheet 0, sheet 1, the fan; all at +2 m/s along x
    fan = sh[2]
    fan[1][:, 2] -= 0.5                       # the fan falls away from the icosphere: its cord goes taut on the way
    Xi, Ti = pr.icosphere(ICO_CENTRE, pr.ICO_R)
    Vi = np.zeros_like(Xi)
    Vi[:, 0] = 2.0
    cloths = [(sh[0][0], sh[0][1], sh[0][2].reshape(-1, 3)), (sh[1][0], sh[1][1], sh[1][2].reshape(-1, 3)),
              (Xi, Vi, Ti.reshape(-1, 3)), (fan[0], fan[1], fan[2].reshape(-1, 3))]
    first = np.cumsum([0] + [len(c[0]) for c in cloths])
    X = np.concatenate([c[0] for c in cloths]).astype(np.float32)
    V = np.concatenate([c[1] for c in cloths]).astype(np.float32)
    T = np.concatenate([c[2] + o for c, o in zip(cloths, first)]).astype(np.int32)
    cv = np.concatenate([np.full(len(c[0]), k) for k, c in enumerate(cloths)])
    cf = np.concatenate([np.full(len(c[2]), k) for k, c in enumerate(cloths)])
    rest = X.astype(np.float64).copy()
    rest[first[1]:first[2]] = _rolled(X[first[1]:first[2]])
    rest = rest.astype(np.float32)
    # links (stiffness, damping in units of m_min / DT^2, m_min / DT; `params` scales them to the guard)
    ico0, fan0 = int(first[2]), int(first[3])
    low = ico0 + int(np.argmin(Xi[:, 2]))
    rows = [(40 + j, NV_SHEET + 40 + j, 1.0, 0.0, 1.0, 0) for j in range(8)]                     # the seam, cross-cloth
    rows += [(HUB, NV_SHEET + HUB - 5 + q, 1.0, 0.01, 1.0, 0) for q in range(10)]                # the hub: a row of ten
    rows += [(100, 103, 1.0, 0.9 * float(np.linalg.norm(X[103].astype(np.float64) - X[100])), 0.5, 0)]   # inside sheet 0
    l_cord = float(np.linalg.norm(X[low].astype(np.float64) - X[fan0]))
    rows += [(fan0, low, 0.05, l_cord + 0.002, 0.0, lk.TENSION)]                                 # the cord: slack by 2 mm
    link_base = lk.make_links(rows)
    # bodies and anchors
    motions = {0: an.motion32((0, 0, 0), np.eye(3), BODY0_V, (0, 0, 0)), 1: an.motion32(BODY1_P, np.eye(3), BODY1_V, BODY1_W)}
    top = ico0 + np.argsort(Xi[:, 2])[-3:]
    a_rows = [(SPRING_ANCHORS[0], 0, X[SPRING_ANCHORS[0]].astype(np.float64) + (0, 0, 0.005), 1.0, 0.0, 1.0, 0),
              (SPRING_ANCHORS[1], 0, X[SPRING_ANCHORS[1]].astype(np.float64) + (0, 0, 0.005), 1.0, 0.004, 1.0, 0)]
    a_rows += [(int(v), 1, X[v].astype(np.float64) + (0, 0, 0.02) - np.array(BODY1_P), 1.0, 0.018, 0.5, an.TENSION) for v in top]
    anchor_base = an.make_anchors(a_rows)
    pressure = pr.make_table([(pr.CONSTANT, 20.0, 0, 0, 0), (pr.OFF, 0, 0, 0, 0),
                              (pr.GAS, 0.0, np.float32(1.5 * 100.0 * pr.volume64(Xi, Ti)), 100.0, 1000.0), (pr.OFF, 0, 0, 0, 0)])
    _SCENE.update(cloths=cloths, first=first, X=X, V=V, T=T, cv=cv, cf=cf, rest=rest, link_base=link_base, cord=len(rows) - 1,
                  cord_vertex=fan0, anchor_base=anchor_base, motions=motions, pressure=pressure,
                  pins=[(v, 0, X[v].astype(np.float64)) for v in PINS])
    return _SCENE


def perturbed_state(seed=7):
    """(x0, v0) float32 per vertex: the scene a tenth of a spacing off its positions, velocities of 0.3 m/s about the drift"""
    s = scene()
    r = np.random.default_rng(seed)
    x0 = (s["X"].astype(np.float64) + 0.1 * (0.4 / RES) * r.normal(size=s["X"].shape)).astype(np.float32)
    v0 = (np.array([2.0, 0.0, 0.0]) + 0.3 * r.normal(size=s["X"].shape)).astype(np.float32)
    return x0, v0


# ---- the engine ---------------------------------------------------------------------------------------------------------
def _create(env):
    """GpuMpm(6) under the environment switches `env` (read per handle, at mpm_create)"""
    from drake_amd import GpuMpm
    assert set(env or {}) <= set(ENV_SWITCHES), env
    with harness.environ(env):
        return GpuMpm(6)


def vertices(g, which):
    """a per-particle array of the engine, for the vertices in original order"""
    from drake_amd import ARR as A
    a, pids = g.download(which), g.download(A.PIDS)
    out = np.zeros((g.n_verts,) + a.shape[1:], a.dtype)
    out[pids[pids >= g.n_faces] - g.n_faces] = a[pids >= g.n_faces]
    return out


def upload(g, x, v, F=None):
    """vertex positions and velocities (n_verts, 3) in original order; a face particle gets its corners' means; C = 0;
    F (n_faces, 9) in original face order, as MPM_ARR_DEFORMATION_GRADIENTS is downloaded, or None: left as it is"""
    from drake_amd import ARR as A
    T = scene()["T"]
    x, v = np.asarray(x, np.float32), np.asarray(v, np.float32)
    mean = lambda a: a[T].astype(np.float64).mean(axis=1).astype(np.float32)   # noqa: E731
    pos, vel = np.concatenate([mean(x), x]), np.concatenate([mean(v), v])
    pids = g.download(A.PIDS)
    g.upload_particle_state(pos[pids], vel[pids], np.zeros((len(pos), 9), np.float32), None,
                            F)


def _motions(motions):
    from drake_amd import BodyMotion
    return [BodyMotion(b, m[0], m[1].ravel(), m[2], m[3]) for b, m in motions.items()]


def cloth_material(c):
    """the material of cloth c on an engine with `materials`: stiffer and denser from cloth to cloth"""
    from drake_amd import ClothMaterial, GpuMpm
    m = ClothMaterial.of(GpuMpm.default_material())
    m.youngs_modulus *= 1.0 + 0.25 * c
    m.density *= 1.0 + 0.1 * c
    return m


def _base(g, features, materials=True):
    s = scene()
    g.set_deterministic(True)
    for c, (pos, vel, T) in enumerate(s["cloths"]):
        if "materials" in features and materials:
            g.add_qr_cloth(pos, vel, T.reshape(-1), cloth_material(c))
        else:
            g.add_qr_cloth(pos, vel, T.reshape(-1))
    g.finalize()
    g.reallocate_external_bodies(3)
    g.set_body_motions(_motions(s["motions"]))


def _scaled(table, s):
    """stiffness x s^2, damping x s: the guard W dt^2 + 2 G dt = 4 of links and anchors then holds at dt / s"""
    out = table.copy()
    out["stiffness"] = (table["stiffness"].astype(np.float64) * s * s).astype(np.float32)
    out["damping"] = (table["damping"].astype(np.float64) * s).astype(np.float32)
    return out


def params():
    """the stiffnesses of the scene, found once on a probe engine with everything on: each set, its guard read, and
    rescaled so that DT is SHARE of the guard"""
    if PARAMS:
        return PARAMS
    from drake_amd import ARR as A
    s = scene()
    g = _create(None)
    _base(g, EVERYTHING)
    m_min = float(vertices(g, A.MASSES).astype(np.float64).min())
    # quadratic bending on the sheets (the guard goes with 1 / sqrt(k))
    on = np.array([1.0, 1.0, 0.0, 0.0])
    g.set_bending(1e-5 * on)
    k_bend = (np.float32(1e-5 * (SHARE * g.bending_max_stable_dt() / DT) ** 2) * on).astype(np.float32)
    g.set_bending(k_bend)
    # damping: membrane on all cloths, hinges on the sheets (the guard goes with 1 / beta)
    d_on = np.array([[1.0, 1.0], [1.0, 1.0], [1.0, 0.0], [1.0, 0.0]])
    g.set_damping(d_on)
    betas = (d_on * (SHARE * g.damping_max_stable_dt() / DT)).astype(np.float32)
    g.set_damping(betas)
    # links and anchors: from the smallest vertex mass, then to the guard
    tables = {}
    for what, base, set_, lim in (("links", s["link_base"], g.set_links, g.links_max_stable_dt),
                                  ("anchors", s["anchor_base"], g.set_anchors, g.anchors_max_stable_dt)):
        t = base.copy()
        t["stiffness"] = (base["stiffness"].astype(np.float64) * 0.02 * m_min / DT ** 2).astype(np.float32)
        t["damping"] = (base["damping"].astype(np.float64) * 0.05 * m_min / DT).astype(np.float32)
        set_(t)
        t = _scaled(t, SHARE * lim() / DT)
        set_(t)
        tables[what] = t
    # shell bending on sheet 1 (rolled rest shape) and on the icosphere (its own); k = 0 elsewhere
    s_on = np.array([0.0, 1.0, 1.0, 0.0])
    g.set_shell_bending(s_on, s["rest"])
    k_shell = (np.float32((SHARE * g.shell_max_stable_dt() / DT) ** 2) * s_on).astype(np.float32)
    g.set_shell_bending(k_shell, s["rest"])
    guards = dict(bending=g.bending_max_stable_dt(), damping=g.damping_max_stable_dt(), links=g.links_max_stable_dt(),
                  shell=g.shell_max_stable_dt(), anchors=g.anchors_max_stable_dt())
    g.destroy()
    for k, lim in guards.items():
        assert np.isfinite(lim) and DT <= 0.5 * lim and DT >= 0.49 * lim, (k, lim)
    PARAMS.update(k_bend=k_bend, betas=betas, links=tables["links"], anchors=tables["anchors"], k_shell=k_shell, m_min=m_min,
                  guards=guards)
    return PARAMS


def null_anchors(anchors):
    out = anchors.copy()
    out["stiffness"] = out["damping"] = 0.0
    return out


CLOCK = 2 * float(np.float32(DT))     # where `clock` puts the bodies' clocks (added in double, as the engine adds them)


def engine(features=EVERYTHING, env=None, grid_bodies=False, clock=False, materials=True):
    """-> a finalised deterministic engine of the scene with the subset `features` on.  env: environment switches around
    GpuMpm() only.  grid_bodies: one grid body (a sphere on body 1 in the fan's way) for mpm_bc = BC_BODIES.  clock: the
    bodies' clocks at CLOCK -- two substeps with an anchor table that does nothing (tests/test_anchors_gpu._scene_engine)
    before anything else is switched on; the caller uploads the state afterwards.  materials = False: one material for
    all cloths whatever `features` says (the rest records of the damping reference)."""
    from drake_amd import FF_DRAG, Collider, ForceField, GridBody, Pin
    from drake_amd.capi import GC_SLIP_APPROACHING
    features = frozenset(features)
    assert features <= EVERYTHING, features - EVERYTHING
    assert "bend_damping" not in features or "bending" in features
    s, p = scene(), params()
    g = _create(env)
    _base(g, features, materials)
    if clock:
        g.set_anchors(null_anchors(p["anchors"]))
        assert g.anchors_max_stable_dt() == np.inf
        g.run_substeps(2, DT, -1)
        g.gpu_sync()
        g.set_anchors(p["anchors"][:0])
    guards = []
    if "bending" in features:
        g.set_bending(p["k_bend"])
        guards.append(g.bending_max_stable_dt())
    if "damping" in features or "bend_damping" in features:
        b = p["betas"].copy()
        if "damping" not in features:
            b[:, 0] = 0.0
        if "bend_damping" not in features:
            b[:, 1] = 0.0
        g.set_damping(b)
        guards.append(g.damping_max_stable_dt())
    if "links" in features:
        g.set_links(p["links"])
        guards.append(g.links_max_stable_dt())
    if "pressure" in features:
        g.set_pressure(s["pressure"])
    if "shell" in features:
        g.set_shell_bending(p["k_shell"], s["rest"])
        guards.append(g.shell_max_stable_dt())
    if "anchors" in features:
        g.set_anchors(p["anchors"])
        guards.append(g.anchors_max_stable_dt())
    if "pins" in features:
        g.set_pins([Pin(*q) for q in s["pins"]])
    if "fields" in features:
        g.set_force_fields([ForceField(FF_DRAG, gamma=2.0, u0=(0.3, 0.0, 0.5))])
    if grid_bodies:
        ball = Collider(1, body=1, p_WB=(0.56, 0.5, 0.5625), dims=(0.03, 0, 0))
        g.set_grid_bodies([GridBody(ball, mode=GC_SLIP_APPROACHING)])
    for lim in guards:
        assert DT <= 0.5 * lim, (lim, sorted(features))
    return g


def bc_of(grid_bodies):
    from drake_amd import BC_BODIES
    return BC_BODIES if grid_bodies else -1


# ---- runners ------------------------------------------------------------------------------------------------------------
def floor():
    from drake_amd import Collider
    return [Collider(0, body=2, p_WB=(0.5, 0.5, FLOOR_Z))]


def far_collider():
    from drake_amd import Collider
    return [Collider(1, body=2, p_WB=FAR, dims=(0.02, 0, 0))]


def _substeps(g, bc):
    for _ in range(N):
        g.substep(DT, bc)


def seven_calls(g, colliders, n, bc=-1):
    """the reference's seven calls per substep (tests/test_contact_noroundtrip_gpu._coupled) -> the per-substep results"""
    out = []
    for _ in range(n):
        g.rebuild_mapping(False)
        g.calc_fem_state_and_force(DT)
        g.particle_to_grid(DT)
        g.update_grid(bc)
        g.generate_contact_pairs(colliders, want_count=False)
        out.append(g.update_contact(DT, MU, K_CT, D_CT))
        g.grid_to_particle(DT)
    g.gpu_sync()
    return out


COUPLED_CALLS = (13, N - 13)      # run_coupled_substeps in two uneven calls


def coupled(g, colliders, bc=-1, calls=COUPLED_CALLS):
    out = []
    for n in calls:
        out += g.run_coupled_substeps(n, DT, colliders, MU, K_CT, D_CT, mpm_bc=bc)
    g.gpu_sync()
    return out


# name -> (runner(g, bc), environment switches)
FUSED = {
    "run_substeps": (lambda g, bc: sp._run_substeps(g, bc), None),
    "run_substeps_sparse_checks": (lambda g, bc: sp._run_substeps(g, bc), SPARSE_CHECKS),
    "substeps": (_substeps, None),
    "profile_substeps": (lambda g, bc: sp._profile_substeps(g, bc), None),
    "phase_calls": (lambda g, bc: sp._phase_calls(g, bc), None),
    "phase_calls_undeferred": (lambda g, bc: sp._phase_calls(g, bc), {"MPM_DEFER_PHASES": "0"}),
}


# ---- the state that is compared -----------------------------------------------------------------------------------------
def words(a):
    """the array's bits: uint32 / uint64 words of a plain 4- or 8-byte type, bytes of a record array"""
    a = np.ascontiguousarray(a)
    if a.dtype.kind in "fiu" and a.dtype.itemsize in (4, 8):
        return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64).copy()
    return np.frombuffer(a.tobytes(), np.uint8).copy()


def accessors(g):
    """every *_forces() accessor of the engine, float32 (n_verts, 3) in original vertex order"""
    return dict(bending=g.bending_forces(), damping=g.damping_forces(), links=g.link_forces(), pressure=g.pressure_forces(),
                shell=g.shell_forces(), anchors=g.anchor_forces())


def state(g):
    """everything a path may leave differently, as words: the particle arrays and PIDS, the bodies' accumulators, the
    pressure, anchor and shell states, every force accessor"""
    from drake_amd import ARR as A
    g.gpu_sync()
    out = {k: words(g.download(arr)) for k, arr in (("pos", A.POSITIONS), ("vel", A.VELOCITIES), ("C", A.AFFINE),
                                                    ("F", A.DEFORMATION_GRADIENTS), ("pids", A.PIDS))}
    tau, f = g.external_body_force_to_host()
    out["tau"], out["f"] = words(tau), words(f)
    out["pressure_state"] = words(g.pressure_state())
    if len(g.get_anchors()):
        a = g.anchor_state()
        out["anchor_energy"], out["anchor_length"], out["anchor_point"] = words(np.array([a["energy"]])), words(a["length"]), words(a["point"])
    E, psi, inactive = g.shell_state()
    out["shell_energy"], out["shell_psi"], out["shell_inactive"] = words(E), words(psi), np.array([inactive], np.uint32)
    for k, v in accessors(g).items():
        out["forces_" + k] = words(v)
    return out


def floats(st, key, dtype=np.float32):
    return st[key].view(dtype)


def run(name, features=EVERYTHING, grid_bodies=False):
    """fused path `name` on a fresh engine -> (state, stats, dict(owed: owed substeps at the end, cord0: the cord
    vertex's link force before the first substep, gauge0: the gauge pressures before the first substep, skipped: the
    substeps still owed when the runner returned))"""
    runner, env = FUSED[name]
    g = engine(features, env=env, grid_bodies=grid_bodies)
    more = dict(cord0=g.link_forces()[scene()["cord_vertex"]].copy(), gauge0=g.pressure_state()["gauge"].copy())
    runner(g, bc_of(grid_bodies))
    more["skipped"] = g.owed_substeps()       # (before the first synchronisation point: substeps that skipped themselves)
    st = state(g)
    stats = g.stats()
    more["owed"] = g.owed_substeps()
    g.destroy()
    return st, stats, more


def state_hash(st):
    import hashlib
    h = hashlib.sha256()
    for k in sorted(st):
        h.update(k.encode())
        h.update(np.ascontiguousarray(st[k]).tobytes())
    return h.hexdigest()[:16]


# ---- the float64 composition of the chain -------------------------------------------------------------------------------
def compose64(stages):
    """stages: the per-stage float32 vertex forces in launch order -- FEM + k_vforce, bend, bend_damp, link, pressure,
    shell, anchor --, each (n, 3).  -> (partial sums (n_stages, n, 3) float64, bound (n, 3)): partial k is stages 0 .. k
    added in float64, and the bound U sum_{k >= 1} |partial_k| allows one rounding of the sum for every stage that is added
    to the forces in DP::f (the first partial is k_vforce's own float: nothing is added to it)."""
    s = np.stack([np.asarray(a, np.float32).astype(np.float64) for a in stages])
    partial = np.cumsum(s, axis=0)
    return partial, U * np.abs(partial[1:]).sum(axis=0)


def compose_margin(total, stages):
    """|total - float64 sum of the stages| over compose64's bound, the worst vertex component (0 where the error vanishes)"""
    partial, bound = compose64(stages)
    err = np.abs(np.asarray(total, np.float32).astype(np.float64) - partial[-1])
    w = np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))
    return float(w.max())


def sum_margin(total, before, added):
    """the criterion of the per-feature test_total_forces_include_*: |total - (before + added)| in units of one rounding
    U |total|, the worst component (0 where the error vanishes)"""
    tot = np.asarray(before, np.float32).astype(np.float64) + np.asarray(added, np.float32).astype(np.float64)
    err = np.abs(np.asarray(total, np.float32).astype(np.float64) - tot)
    return float((err / np.maximum(U * np.abs(total).astype(np.float64), 1e-300))[err > 0].max()) if (err > 0).any() else 0.0
