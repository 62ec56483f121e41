"""The host lists of drake_amd/csrc/mpm_features.h on the engine: that feature_state (mpm_host.h) reads every feature
correctly, which tests/test_features.py (CPU, the table alone) cannot see.

Scene: GpuMpm(4); one sheet of 3 x 3 vertices (8 faces, interior hinges) and one tetrahedron (closed), two cloths.  One
engine per feature, the feature set with the smallest valid table:
  - a halo entry point refuses with the literal message (the rest shape: the halo substep runs, a set-up call refuses);
  - set_rest_shape refuses with the literal message or is accepted, as the feature caches rest-derived values or not;
  - run_substeps(1, dt) refuses the float above the feature's own *_max_stable_dt with the literal message and takes the
    float below it (a feature without a guard: DT);
  - after clearing, all three pass and every *_max_stable_dt reads inf;
  - stats()["substeps"] counts the accepted substeps only.
The messages are literals copied from the host lists as they stood before the table.  Stiffnesses are scaled so that every
guard lies at about DT: the guards go with 1 / sqrt(k) (bending, shell, weave, links and anchors without damping) or with
1 / beta (damping), so one probe of the guard gives the factor."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DT = 2e-4          # well below the membrane's own limit on this mesh (spacing 0.03 m, wave speed 14 m/s: 2e-3 s)
INVALID = -1       # MPM_ERR_INVALID
H = 0.03

# extensions_refused: "<what>: not available on " + ...
NOT_AVAILABLE_ON = {
    "pins": "an engine with pins (mpm_set_pins)",
    "materials": "a multi-material engine (mpm_add_qr_cloth_with_material)",
    "grid_bodies": "an engine with grid bodies (mpm_set_grid_bodies)",
    "force_fields": "an engine with force fields (mpm_set_force_fields)",
    "bending": "an engine with bending stiffness (mpm_set_bending)",
    "damping": "an engine with damping (mpm_set_damping)",
    "weave": "an engine with a weave (mpm_set_weave)",
    "tearing": "an engine with tearing (mpm_set_tearing, mpm_set_torn_faces)",
    "links": "an engine with links (mpm_set_links)",
    "pressure": "an engine with pressure (mpm_set_pressure)",
    "shell": "an engine with shell bending (mpm_set_shell_bending)",
    "anchors": "an engine with anchors (mpm_set_anchors)",
    "rest_shape": "an engine with a rest shape of its own (mpm_set_rest_shape; null restores the positions as added)",
}
# rest_shape_conflict
REST_PHRASE = {
    "bending": "bending stiffness (mpm_set_bending)",
    "shell": "shell bending (mpm_set_shell_bending)",
    "weave": "a weave (mpm_set_weave)",
    "damping": "damping (mpm_set_damping)",
    "pressure": "pressure (mpm_set_pressure)",
    "links": "links (mpm_set_links)",
    "anchors": "anchors (mpm_set_anchors)",
    "pins": "pins (mpm_set_pins)",
}
REST_REFUSAL = "mpm_set_rest_shape: the engine has %s, which holds values derived from the rest shape: clear it, set the rest shape, set it again"
# fields_stable: (feature, force, reduce) of dt_above_limit
GUARD_WORDS = {
    "anchors": ("anchors", "anchor", "dt, the stiffness or the damping"),
    "shell": ("shell", "shell bending", "dt or the stiffness"),
    "links": ("links", "link", "dt, the stiffness or the damping"),
    "weave": ("weave", "weave", "dt or the moduli"),
    "damping": ("damping", "damping", "dt or the coefficients"),
    "bending": ("bending", "bending", "dt or the stiffness"),
}
DT_REFUSAL = "%s: dt = %g is above the limit mpm_%s_max_stable_dt = %g: the explicit %s force is unstable -- reduce %s"
FEATURES = tuple(NOT_AVAILABLE_ON)


def _meshes():
    """(sheet positions (9, 3), sheet triangles (8, 3), tetrahedron positions (4, 3), its triangles (4, 3) wound outwards)"""
    ij = np.array([(i, j) for j in range(3) for i in range(3)], np.float64)
    Xs = np.column_stack([0.37 + H * ij[:, 0], 0.47 + H * ij[:, 1], np.full(9, 0.5)]).astype(np.float32)
    Ts = np.array([t for j in range(2) for i in range(2) for t in
                   ((3 * j + i, 3 * j + i + 1, 3 * j + i + 4), (3 * j + i, 3 * j + i + 4, 3 * j + i + 3))], np.int32)
    Xt = (np.array([0.6, 0.5, 0.5]) + 0.03 * np.array([(1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)], np.float64)).astype(np.float32)
    Tt = np.array([(0, 1, 2), (0, 3, 1), (0, 2, 3), (1, 3, 2)], np.int32)
    return Xs, Ts, Xt, Tt


def _engine(materials=False):
    from drake_amd import BodyMotion, ClothMaterial, GpuMpm, mesh_is_closed
    Xs, Ts, Xt, Tt = _meshes()
    assert mesh_is_closed(Tt.reshape(-1), 4)
    g = GpuMpm(4)
    m = ClothMaterial.of(GpuMpm.default_material()) if materials else None
    g.add_qr_cloth(Xs, np.zeros_like(Xs), Ts.reshape(-1), m)
    g.add_qr_cloth(Xt, np.zeros_like(Xt), Tt.reshape(-1), m)
    g.finalize()
    g.reallocate_external_bodies(1)
    g.set_body_motions([BodyMotion(0)])
    return g


def _to_guard(set_, guard, power):
    """sets the feature so that its guard lies within [DT / 2, 2 DT]: set_(1) is probed, the guard goes with scale^-1/power"""
    set_(1.0)
    set_((guard() / DT) ** power)
    assert 0.5 * DT <= guard() <= 2.0 * DT, guard()


def _feature(g, name):
    """(set, clear, the feature's *_max_stable_dt or None) on engine g"""
    from drake_amd import FF_ACCEL, PRESSURE_CONSTANT, PRESSURE_DTYPE, Anchor, Collider, ForceField, GridBody, Pin, links, weave
    Xs, _, Xt, _ = _meshes()
    const = np.zeros(2, PRESSURE_DTYPE)
    const["mode"][1], const["p"][1] = PRESSURE_CONSTANT, 1.0
    no_links = links([], [], 0.0)
    rest = (np.concatenate([Xs, Xt]).astype(np.float64) * 1.02).astype(np.float32)
    diagonal = float(np.linalg.norm(Xs[8].astype(np.float64) - Xs[0]))
    table = {
        "pins": (lambda: g.set_pins([Pin(0, 0, Xs[0])]), lambda: g.set_pins([]), None),
        "materials": (lambda: None, None, None),                      # (part of the engine from the first cloth on)
        "grid_bodies": (lambda: g.set_grid_bodies([GridBody(Collider(1, body=0, p_WB=(0.5, 0.5, 0.3), dims=(0.03, 0, 0)))]),
                        lambda: g.set_grid_bodies([]), None),
        "force_fields": (lambda: g.set_force_fields([ForceField(FF_ACCEL, u0=(0.0, 0.0, 1.0))]), lambda: g.set_force_fields([]), None),
        "bending": (lambda: _to_guard(lambda s: g.set_bending([1e-6 * s, 0.0]), g.bending_max_stable_dt, 2), lambda: g.set_bending([]),
                    g.bending_max_stable_dt),
        "damping": (lambda: _to_guard(lambda s: g.set_damping([[1e-4 * s, 0.0], [0.0, 0.0]]), g.damping_max_stable_dt, 1),
                    lambda: g.set_damping([]), g.damping_max_stable_dt),
        "weave": (lambda: _to_guard(lambda s: g.set_weave([weave(E_warp=1e4 * s), weave()]), g.weave_max_stable_dt, 2),
                  lambda: g.set_weave([]), g.weave_max_stable_dt),
        "tearing": (lambda: g.set_tearing([1.5, 0.0]), lambda: g.set_tearing([0.0, 0.0]), None),
        "links": (lambda: _to_guard(lambda s: g.set_links(links([0], [8], 1.0 * s, rest_length=diagonal)), g.links_max_stable_dt, 2),
                  lambda: g.set_links(no_links), g.links_max_stable_dt),
        "pressure": (lambda: g.set_pressure(const), lambda: g.set_pressure([]), None),
        "shell": (lambda: _to_guard(lambda s: g.set_shell_bending([1e-6 * s, 0.0]), g.shell_max_stable_dt, 2),
                  lambda: g.set_shell_bending([]), g.shell_max_stable_dt),
        "anchors": (lambda: _to_guard(lambda s: g.set_anchors([Anchor(0, 0, Xs[0], stiffness=1.0 * s)]), g.anchors_max_stable_dt, 2),
                    lambda: g.set_anchors([]), g.anchors_max_stable_dt),
        "rest_shape": (lambda: g.set_rest_shape(rest), lambda: g.set_rest_shape(None), None),
    }
    return table[name]


def _refused(call, message):
    from drake_amd import MpmError
    with pytest.raises(MpmError) as err:
        call()
    assert err.value.code == INVALID and str(err.value) == f"mpm_hip error {INVALID}: {message}", str(err.value)


def _halo_substep(g):
    from drake_amd import GpuMpm
    g.substep_begin_halo(DT, GpuMpm.halo_zone_args([], []), 0)
    g.substep_end_halo(DT, -1, GpuMpm.halo_buffer_args([]), 0)


@pytest.mark.parametrize("name", FEATURES)
def test_one_feature_in_force(name):
    from drake_amd import GpuMpm
    g = _engine(materials=name == "materials")
    Xs, _, Xt, _ = _meshes()
    other_rest = (np.concatenate([Xs, Xt]).astype(np.float64) * 0.98).astype(np.float32)
    set_, clear, guard = _feature(g, name)
    set_()
    accepted = 0
    # 1. the partitioned paths
    if name == "rest_shape":
        _halo_substep(g)
        accepted += 1
        _refused(lambda: g.team_prepare(), "mpm_team_prepare: not available on " + NOT_AVAILABLE_ON[name])
    else:
        _refused(lambda: g.substep_begin_halo(DT, GpuMpm.halo_zone_args([], []), 0), "halo substeps: not available on " + NOT_AVAILABLE_ON[name])
        _refused(lambda: g.team_prepare(), "mpm_team_prepare: not available on " + NOT_AVAILABLE_ON[name])
    # 2. a new rest shape
    if name in REST_PHRASE:
        _refused(lambda: g.set_rest_shape(other_rest), REST_REFUSAL % REST_PHRASE[name])
        assert not g.get_rest_shape()[1]
    else:
        g.set_rest_shape(other_rest)
        assert g.get_rest_shape()[1]
        if name != "rest_shape":
            g.set_rest_shape(None)
    # 3. the dt guard
    limits = dict(bending=g.bending_max_stable_dt(), damping=g.damping_max_stable_dt(), weave=g.weave_max_stable_dt(),
                  links=g.links_max_stable_dt(), shell=g.shell_max_stable_dt(), anchors=g.anchors_max_stable_dt())
    assert {k for k, v in limits.items() if np.isfinite(v)} == ({name} if guard else set()), limits
    if guard:
        lim = np.float32(guard())
        above, below = np.nextafter(lim, np.float32(np.inf)), np.nextafter(lim, np.float32(0))
        words = GUARD_WORDS[name]
        _refused(lambda: g.run_substeps(1, float(above)), DT_REFUSAL % (words[0], float(above), words[0], float(lim), words[1], words[2]))
        g.run_substeps(1, float(below))
    else:
        g.run_substeps(1, DT)
    accepted += 1
    g.gpu_sync()
    assert g.stats()["substeps"] == accepted and g.stats()["error_flags"] == 0, g.stats()
    # 4. cleared: everything passes
    if clear is not None:
        clear()
        _halo_substep(g)
        g.set_rest_shape(other_rest)
        g.set_rest_shape(None)
        g.run_substeps(1, float(np.nextafter(np.float32(2 * DT), np.float32(np.inf))))     # (above where the guard was)
        accepted += 2
        _refused(lambda: g.team_prepare(), "mpm_dist_init first")                       # (past extensions_refused)
        for read in (g.bending_max_stable_dt, g.damping_max_stable_dt, g.weave_max_stable_dt, g.links_max_stable_dt,
                     g.shell_max_stable_dt, g.anchors_max_stable_dt):
            assert read() == np.inf
    g.gpu_sync()
    assert g.stats()["substeps"] == accepted and g.stats()["error_flags"] == 0, g.stats()
    g.destroy()


def test_tearing_conflicts():
    """hinges and pressure do not compose with tearing, per cloth and in both orders; of two conflicting features of one
    cloth the first in the table's order (bending, pressure, shell bending) is named"""
    from drake_amd import PRESSURE_CONSTANT, PRESSURE_DTYPE
    g = _engine()
    on_sheet, on_tet = np.zeros(2, PRESSURE_DTYPE), np.zeros(2, PRESSURE_DTYPE)
    on_sheet["mode"][0], on_sheet["p"][0] = PRESSURE_CONSTANT, 1.0
    on_tet["mode"][1], on_tet["p"][1] = PRESSURE_CONSTANT, 1.0
    torn = "mpm_set_%s: cloth 0 has a tear limit or a torn face (mpm_set_tearing, mpm_set_torn_faces): hinges and pressure across torn faces are not available"
    # a limit on the sheet: bending, shell bending and pressure on it are refused, on the tetrahedron they are not
    g.set_tearing([1.5, 0.0])
    _refused(lambda: g.set_bending([1e-6, 0.0]), torn % "bending")
    _refused(lambda: g.set_shell_bending([1e-6, 0.0]), torn % "shell_bending")
    _refused(lambda: g.set_pressure(on_sheet), torn % "pressure")
    assert not g.get_bending().any() and not g.get_shell_bending()["stiffness"].any() and not g.get_pressure()["mode"].any()
    g.set_bending([0.0, 1e-6])
    g.set_shell_bending([0.0, 1e-6])
    g.set_pressure(on_tet)
    # the reverse: a limit or a cut on a cloth with one of them
    composes = "mpm_set_%s: cloth %d has %s, which tearing does not compose with"
    _refused(lambda: g.set_tearing([1.5, 1.5]), composes % ("tearing", 1, "bending stiffness (mpm_set_bending)"))
    cut = np.zeros(12, np.uint8)
    cut[8] = 1
    _refused(lambda: g.set_torn_faces(cut), composes % ("torn_faces", 1, "bending stiffness (mpm_set_bending)"))
    g.set_bending([])
    _refused(lambda: g.set_tearing([1.5, 1.5]), composes % ("tearing", 1, "pressure (mpm_set_pressure)"))
    g.set_pressure([])
    _refused(lambda: g.set_tearing([1.5, 1.5]), composes % ("tearing", 1, "shell bending (mpm_set_shell_bending)"))
    g.set_shell_bending([])
    g.set_tearing([1.5, 1.5])
    assert np.array_equal(g.get_tearing(), np.array([1.5, 1.5], np.float32))
    g.destroy()
