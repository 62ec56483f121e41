"""ParticleToGrid, UpdateGrid and GridToParticle of the engine on the layouts of tests/transfer_layouts.py, phase by
phase, against the float64 restatements of the same module, node by node and particle by particle:

    P2G   grid mass and momentum within K (L_n + 16) 2^-24 A_n + N_n q at every node (transfer_layouts docstring),
          GRID_TOUCHED_FLAGS bit-exact, total mass and momentum against the particle sums
    grid  GRID_V_STAR bit-exact: the float32 quotient of the engine's own raw sums, then the walls
    G2P   v, C and x within the per-particle bound over the 27 nodes

Each phase is judged on the engine's own inputs of that phase (downloaded after the phase before it), under the default
engine (double LDS tiles), deterministic mode (64-bit fixed-point tiles, canonical order) and MPM_P2G_FIXED=1 alone.
The fused vertex-force instance k_p2g<1, .> (what mpm_substep runs) is covered by a twin engine in deterministic mode:
its substep is bit-equal to the phase calls in positions, velocities and affine matrices."""
import numpy as np
import pytest

from tests import harness as hs
from tests import transfer_layouts as tl

pytestmark = pytest.mark.gpu

MODES = ("default", "deterministic", "p2g_fixed")
_RUNS = {}


def _engine(lay, mode):
    from drake_amd import ClothMaterial, GpuMpm
    env = {"MPM_ANTICIPATE": str(lay["anticipate"]), **lay["env"]}
    if mode == "p2g_fixed":
        env["MPM_P2G_FIXED"] = "1"
    with hs.environ(env):
        mat = GpuMpm.default_material()
        mat.gravity_axis = lay["gravity_axis"]
        g = GpuMpm(lay["bits"], mat)
        g.set_deterministic(mode == "deterministic")
        for c, (rest, vel, idx) in enumerate(lay["cloths"]):
            if lay["densities"]:
                cm = ClothMaterial.of(mat)
                cm.density = lay["densities"][c]
                g.add_qr_cloth(rest, vel, idx, material=cm)
            else:
                g.add_qr_cloth(rest, vel, idx)
        g.finalize()
        # (the anticipatory binning needs a known substep length: one FEM pass sets it)
        g.calc_fem_state_and_force(tl.DT)
        g.gpu_sync()
    from drake_amd import ARR as A
    pids = g.download(A.PIDS)
    # the uploaded positions force a re-sort at the next RebuildMapping
    g.upload_particle_state(lay["pos"][pids], lay["vel"][pids], lay["C"][pids], lay["vol"][pids], None)
    return g


def _run(name, mode):
    """the phase calls with a download after each phase; -> dict of what each phase got and gave (slot order)"""
    key = (name, mode)
    if key in _RUNS:
        return _RUNS[key]
    from drake_amd import ARR as A
    lay = tl.layout(name)
    g = _engine(lay, mode)
    g.rebuild_mapping(False)
    g.calc_fem_state_and_force(tl.DT)
    d = dict(lay=lay)
    for k, a in (("pids", A.PIDS), ("x", A.POSITIONS), ("v", A.VELOCITIES), ("C", A.AFFINE), ("m", A.MASSES),
                 ("taus", A.TAUS), ("f", A.FORCES)):
        d[k] = g.download(a)
    g.particle_to_grid(tl.DT)
    d["gm"], d["gmv"], d["flags"] = g.download(A.GRID_MASSES), g.download(A.GRID_MOMENTUM), g.download(A.GRID_TOUCHED_FLAGS)
    g.update_grid(-1)
    d["gvs"] = g.download(A.GRID_V_STAR)
    g.grid_to_particle(tl.DT)
    d["x1"], d["v1"], d["C1"] = g.download(A.POSITIONS), g.download(A.VELOCITIES), g.download(A.AFFINE)
    d["stats"] = g.stats()
    g.destroy()
    _RUNS[key] = d
    return d


def _p2g_inputs(d):
    face = d["pids"] < d["lay"]["nf"]
    taus = np.where(face[:, None], d["taus"], 0.0)     # (the kernel's face lanes take tau, vertex lanes the force)
    f = np.where(face[:, None], 0.0, d["f"])
    return d["x"], d["v"], d["C"], d["m"], taus, f


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", tl.NAMES)
def test_transfers_phase_by_phase(name, mode):
    from tests import helpers
    helpers.tag_default_engine(mode == "default")   # (particle order inside a cell from atomics: margins vary by run)
    d = _run(name, mode)
    lay = d["lay"]
    bits = lay["bits"]
    assert d["stats"]["error_flags"] == 0, d["stats"]
    # the layout's particles, all of them, in the engine
    assert np.array_equal(np.sort(d["pids"]), np.arange(lay["nf"] + lay["nv"]))
    x, v, C, m, taus, f = _p2g_inputs(d)
    r = tl.p2g64(x, v, C, m, taus, f, bits, lay["gravity_axis"])
    quanta = tl.fixed_quanta(m) if mode != "default" else None
    bm, bmv = tl.p2g_bounds(r, quanta)
    fails = []
    worst = {}

    def check(field, err, bound):
        w = tl.margin(err, bound)
        worst[field] = w
        hs.record(f"transfer layouts: {name} [{mode}] {field}", w)
        if not w <= 1.0:
            e = np.asarray(err, np.float64).reshape(len(err), -1).max(axis=1)
            b = np.asarray(bound, np.float64).reshape(len(bound), -1).max(axis=1)
            i = int(np.argmax(np.where(e == 0, 0.0, e / np.maximum(b, 1e-300))))
            fails.append(f"{field}: {w:.3g} x the bound at index {i} (err {e[i]:.3e}, bound {b[i]:.3e})")

    # ---- P2G
    check("p2g mass", np.abs(d["gm"] - r["m"]), bm)
    check("p2g momentum", np.abs(d["gmv"] - r["mv"]), bmv)
    assert np.array_equal(d["flags"], r["flags"]), "GRID_TOUCHED_FLAGS"
    # totals: the affine and stress terms cancel over a stencil, so the grid holds the particles' mass and momentum
    ext = np.asarray(m, np.float64)[:, None] * v + np.asarray(f, np.float64) * tl.DT32
    ext[:, lay["gravity_axis"]] += np.asarray(m, np.float64) * tl.GRAVITY * tl.DT32
    tot_m = float(np.sum(np.asarray(m, np.float64)))
    check("p2g total mass", np.array([abs(float(d["gm"].astype(np.float64).sum()) - tot_m)]),
          np.array([bm.sum() + 1e-12 * tot_m]))
    check("p2g total momentum", np.abs(d["gmv"].astype(np.float64).sum(axis=0) - ext.sum(axis=0)),
          bmv.sum(axis=0) + 1e-12 * np.abs(ext).sum(axis=0))
    # ---- grid update: bit-exact from the engine's own raw sums
    want = tl.grid32(d["gm"], d["gmv"], bits)
    got = d["gvs"].reshape(-1, 3)
    bad = np.flatnonzero((want.view(np.uint32) != got.view(np.uint32)).any(axis=1))
    assert bad.size == 0, (f"GRID_V_STAR differs from the float32 quotient at {bad.size} nodes, e.g. key {bad[0]}: "
                           f"{got[bad[0]]} vs {want[bad[0]]} (m {d['gm'][bad[0]]!r}, mv {d['gmv'][bad[0]]})")
    # ---- G2P on the engine's grid velocities and positions
    g = tl.g2p64(x, got, bits)
    check("g2p v", np.abs(d["v1"] - g["v"]), g["bv"])
    check("g2p C", np.abs(d["C1"] - g["C"]), g["bC"])
    check("g2p x", np.abs(d["x1"] - g["x"]), g["bx"])
    assert not fails, f"{name} [{mode}]:\n" + "\n".join(fails)


@pytest.mark.parametrize("name", tl.NAMES)
def test_substep_equals_phase_calls_on_layout(name):
    """deterministic mode: mpm_substep (FEM with the vertex forces summed inside k_p2g<1, 1>) is bit-equal to the phase
    calls (k_vforce, then k_p2g<0, 1>) on every layout"""
    from drake_amd import ARR as A
    d = _run(name, "deterministic")
    g = _engine(d["lay"], "deterministic")
    g.substep(tl.DT, -1)
    assert g.stats()["error_flags"] == 0
    assert np.array_equal(g.download(A.PIDS), d["pids"])
    for k, a in (("x1", A.POSITIONS), ("v1", A.VELOCITIES), ("C1", A.AFFINE)):
        got = g.download(a)
        assert np.array_equal(got.view(np.uint32), d[k].view(np.uint32)), (k, float(np.abs(got - d[k]).max()))
    g.destroy()


def test_gravity_on_every_axis():
    assert {tl.layout(n)["gravity_axis"] for n in tl.NAMES} == {0, 1, 2}
