"""The device-side contact front end -- k_ct_gen_count_scan, k_ct_gen_write and k_ct_watch -- on the layouts of
tests/pair_layouts.py against the float64 restatements of the same module, pair by pair.

Before every generation under test the pair buffers are poisoned: one generation with a half-space that contains every
particle, on body POISON_BODY, which no test collider uses.  Every test collider has a body of its own, so a row's body
names its collider.  Checked for every layout: the counts; every row (its body a test body, (slot, collider) strictly
ascending, dist < 0, pos / p_WB / vel bit-equal to what was uploaded, |normal| within 4 ulp of 1); membership (every
decided-in pair present, no decided-out pair present); and for EVERY decided pair dist, normal and rigid_v within the bounds
of the module.  Then what each layout is for: exact answers (conventions), consistency between generator, query and a second
generation where membership is undecidable (shell), the scan's structural slots in both slot orders (blocks), the
kernel-argument and the device table and all two count and four write instances (tables), the capacity boundary, and the
watch through mpm_debug_contact_watch: must-hit and must-not-hit states per kind 0-5 and for a mesh collider at the first
and the last active index, and "no hit => the generator makes no pair" after CalcFemStateAndForce with fast math off and
on.  A face whose centroid alone is inside exists for the sphere, the box corner and the capsule cap only: the other shapes,
the mesh ball among them, are too large or too flat for a triangle's corners to stay outside.

Not covered at these sizes: the grid-stride second pass of the watch (more than 262144 active particles)."""
import numpy as np
import pytest

from tests import harness as hs
from tests import pair_layouts as pl
from tests import sdf_mesh_reference as meshref

pytestmark = pytest.mark.gpu
F = np.float32
D = np.float64
DT = 1e-3
ROW_FIELDS = ("particle", "body", "dist", "normal", "pos", "rigid_v", "p_WB", "vel")
MESH_BODY_OFFSET = 1       # the mesh collider's body: one past the analytic ones


def _col(c):
    from drake_amd import Collider
    return Collider(c.kind, body=c.body, p_WB=c.p, R_WB=c.R, dims=c.dims, v=c.v, w=c.w)


def _engine(lay, sort=False, env=None, n_bodies=None):
    """-> (engine with the layout's rest mesh, PIDS: API slot -> original id)"""
    from drake_amd import ARR as A, GpuMpm
    with hs.environ(env):
        g = GpuMpm(lay["bits"])
    g.add_qr_cloth(lay["rest"], np.zeros_like(lay["rest"]), lay["idx"])
    g.finalize()
    g.reallocate_external_bodies(n_bodies or max(lay["n_bodies"], 64))
    if sort:
        g.rebuild_mapping(True)
    g.gpu_sync()
    pids = g.download(A.PIDS).astype(np.int64)
    assert np.array_equal(np.sort(pids), np.arange(lay["n"]))
    return g, pids


def _upload_layout(g, pids, pos, vel):
    g.upload_particle_state(pos[pids], vel[pids], None, None, None)


def _poison(g, lay):
    """a row of the poison body for every particle with mass (a vertex in no face has none and makes no pair)"""
    from drake_amd import Collider
    n = lay["n"] - lay["E"]
    mesh = getattr(g, "test_mesh_colliders", [])
    if mesh:       # (the engine's mesh colliders would add their rows)
        g.set_sdf_colliders([])
    assert g.generate_contact_pairs([Collider(0, body=pl.POISON_BODY, p_WB=(0.5, 0.5, 2.0))]) == n
    body = g.download_contact_pairs()[1]
    assert body.size == n and np.all(body == pl.POISON_BODY)
    if mesh:
        g.set_sdf_colliders(mesh)


def _generate(g, cols, poison=None):
    """-> dict of the rows (ROW_FIELDS) of one generation, with the count checks"""
    from drake_amd import ARR as A
    if poison is not None:
        _poison(g, poison)
    before = g.contact_counters()["repeated_overflow"]
    n = g.generate_contact_pairs([_col(c) for c in cols])
    assert n == g.contact_pair_count()
    got = g.download_contact_pairs()
    assert all(len(a) == n for a in got)
    vel = g.download(A.CONTACT_VEL).reshape(-1, 3)[:n] if n else np.zeros((0, 3), F)
    rows = dict(zip(ROW_FIELDS, (*got, vel)))
    rows["overflows"] = g.contact_counters()["repeated_overflow"] - before
    return rows


def _analytic_ev(lay, cols):
    ev = pl.evaluate(dict(lay, cols=cols))
    for e, c in zip(ev, cols):
        e.update(body=c.body, p=c.p, name=pl.KIND_NAMES[c.kind])
    return ev


def _mesh_ev(lay, lattice, mc):
    """the evaluation record of a mesh collider (SdfCollider mc) at the layout's particles"""
    p, R = np.array(mc.p_WB[:], F), np.array(mc.R_WB[:], F)
    phi, grad, _ = pl.mesh_sdf64(lattice, p, R, lay["pos"])
    b = pl.mesh_bounds(lattice, p, R, lay["pos"])
    d = lay["pos"].astype(D) - p.astype(D)
    v, w = np.array(mc.v[:], F).astype(D), np.array(mc.w[:], F).astype(D)
    b["rv"] = 4 * pl.U32 * (np.abs(v).max() + 2 * np.abs(w).max() * np.abs(d).max(1))
    din, dout = pl.classify(phi, b["phi"])
    din, dout = din & ~lay["massless"], dout | lay["massless"]
    return dict(phi=phi, grad=grad, rv=v + np.cross(w, d), b=b, din=din, dout=dout, body=int(mc.body), p=p, name="mesh")


def _check_rows(tag, lay, ev, rows, pids, values=True):
    """the row, membership and value checks of the module docstring; -> the set of (original id, collider index) present"""
    n = len(rows["particle"])
    fails = []
    by_body = {e["body"]: j for j, e in enumerate(ev)}
    assert pl.POISON_BODY not in by_body
    assert all(int(b) in by_body for b in rows["body"]), f"{tag}: a row of a body that is no test collider's (poison?)"
    s = rows["particle"].astype(np.int64)
    assert np.all(s < lay["n"])
    j = np.array([by_body[int(b)] for b in rows["body"]], np.int64)
    assert np.all(np.diff(s * (len(ev) + 1) + j) > 0), f"{tag}: (slot, collider) not strictly ascending"
    orig = pids[s]
    assert np.all(rows["dist"] < 0), f"{tag}: dist >= 0"
    assert np.array_equal(rows["pos"], lay["pos"][orig]), f"{tag}: pos"
    assert np.array_equal(rows["vel"], lay["vel"][orig]), f"{tag}: vel"
    assert np.array_equal(rows["p_WB"], np.array([ev[k]["p"] for k in j], F).reshape(-1, 3)), f"{tag}: p_WB"
    ln = np.linalg.norm(rows["normal"].astype(D), axis=1)
    assert np.all(np.abs(ln - 1) <= 4 * 2.0 ** -23), f"{tag}: |normal| {np.abs(ln - 1).max() if n else 0}"
    present = set(zip(orig.tolist(), j.tolist()))
    assert len(present) == n
    for k, e in enumerate(ev):
        have = np.zeros(lay["n"], bool)
        have[orig[j == k]] = True
        if np.any(e["din"] & ~have):
            fails.append(f"{e['name']} (collider {k}): decided-in pairs missing: particles {np.nonzero(e['din'] & ~have)[0][:8]}")
        if np.any(e["dout"] & have):
            fails.append(f"{e['name']} (collider {k}): decided-out pairs present: particles {np.nonzero(e['dout'] & have)[0][:8]}")
        if not values:
            continue
        m = (j == k) & (e["din"] | e["dout"])[orig]
        o = orig[m]
        if not len(o):
            continue
        for field, err, bound in (("dist", np.abs(rows["dist"][m] - e["phi"][o]), e["b"]["val"][o]),
                                  ("normal", np.abs(rows["normal"][m] + e["grad"][o]).max(1), e["b"]["grad"][o]),
                                  ("rigid_v", np.abs(rows["rigid_v"][m] - e["rv"][o]).max(1), e["b"]["rv"][o])):
            w = pl.margin(err, bound)
            hs.record(f"pair layouts: {tag} {e['name']} {field}", w)
            if not w <= 1.0:
                fails.append(f"{e['name']} (collider {k}) {field}: {w:.3g} x the bound")
    assert not fails, f"{tag}:\n" + "\n".join(fails)
    return present


def _same_rows(a, b, what):
    for f in ROW_FIELDS:
        assert np.array_equal(a[f], b[f]), f"{what}: {f}"


def _by_original(rows, pids):
    """the rows keyed and ordered by (original id, body): slot order taken out"""
    orig = pids[rows["particle"].astype(np.int64)]
    order = np.lexsort((rows["body"], orig))
    out = {f: rows[f][order] for f in ROW_FIELDS if f != "particle"}
    out["orig"] = orig[order]
    return out


# ---- every layout: counts, rows, membership, values -----------------------------------------------------------------

@pytest.mark.parametrize("name", ["features", "conventions", "shell", "tables", "tables_ell", "empty"])
def test_rows_membership_and_values(name):
    lay = pl.layout(name)
    g, pids = _engine(lay)
    _upload_layout(g, pids, lay["pos"], lay["vel"])
    rows = _generate(g, lay["cols"], poison=lay)
    ev = _analytic_ev(lay, lay["cols"])
    n = len(rows["particle"])
    assert rows["overflows"] == 0
    present = _check_rows(name, lay, ev, rows, pids)
    n_in = sum(int(e["din"].sum()) for e in ev)
    n_und = sum(int((~(e["din"] | e["dout"])).sum()) for e in ev)
    assert n_in <= n <= n_in + n_und
    if name == "features":
        assert n_und == 0 and n == n_in
        for j in range(6):
            assert sum(1 for _, k in present if k == j) >= 9
    if name == "empty":
        assert n == 0
        assert g.generate_contact_pairs([]) == 0 and g.contact_pair_count() == 0
    if name.startswith("tables"):
        assert sum(1 for o, _ in present if o == lay["where"][0]) == 17
    assert not lay["massless"][[o for o, _ in present]].any()
    g.destroy()


def test_count_left_on_the_device_is_the_solve_s_count():
    """want_count = False: the count never reaches the host before the solve reports it"""
    lay = pl.layout("empty")
    cols = [pl.Col(0, 1, p=(0.5, 0.5, 0.3), R=pl.rot((1, 0.2, 0), 0.3), v=(0, 0, 0.1), w=(0.1, 0, 0))]
    g, pids = _engine(lay)
    _upload_layout(g, pids, lay["pos"], lay["vel"] * F(0.01))
    ev = _analytic_ev(lay, cols)
    g.rebuild_mapping(False)
    g.calc_fem_state_and_force(DT)
    g.particle_to_grid(DT)
    g.update_grid(-1)
    _poison(g, lay)
    assert g.generate_contact_pairs([_col(c) for c in cols], want_count=False) is None
    g.update_contact(DT, 0.5, 1e5, 1e-3, max_newton_iterations=2)
    n = g.contact_stats()["contacts"]
    # (the vertices are where they were uploaded; the FEM has put the faces at their centroids, which the layout's are)
    lo, hi = int(ev[0]["din"].sum()), int((~ev[0]["dout"]).sum())
    assert 10 < lo <= n <= hi < lay["n"] - 10
    assert n == g.contact_pair_count()
    g.destroy()


# ---- conventions ------------------------------------------------------------------------------------------------------

def test_conventions_are_exact():
    lay = pl.layout("conventions")
    g, pids = _engine(lay)
    _upload_layout(g, pids, lay["pos"], lay["vel"])
    rows = _generate(g, lay["cols"], poison=lay)
    orig = pids[rows["particle"].astype(np.int64)]
    for k, j, phi, grad in lay["exact"]:
        k = int(lay["where"][k])
        c = lay["cols"][j]
        at = np.nonzero((orig == k) & (rows["body"] == c.body))[0]
        assert len(at) == 1, (k, j)
        assert rows["dist"][at[0]] == F(phi), (k, j, rows["dist"][at[0]])
        assert np.array_equal(rows["normal"][at[0]], -np.array(grad, F)), (k, j, rows["normal"][at[0]])
        p, gr = g.collider_signed_distance(_col(c), lay["pos"][k:k + 1])
        assert p[0] == F(phi) and np.array_equal(gr[0], np.array(grad, F)), (k, j, p, gr)
    for j, x, phi, grad in pl.CONVENTION_QUERIES:
        p, gr = g.collider_signed_distance(_col(lay["cols"][j]), np.array([x], F))
        assert p[0] == F(phi) and np.array_equal(gr[0], np.array(grad, F)), (j, x, p, gr)
    # exactly on a surface: phi == 0 is no pair (phi < 0 is); the container behind it has its pair
    for k, j in lay["on_surface"]:
        k = int(lay["where"][k])
        c = lay["cols"][j]
        assert not np.any((orig == k) & (rows["body"] == c.body)), (k, j)
        assert np.sum((orig == k) & (rows["body"] == lay["cols"][-1].body)) == 1, (k, j)
        assert g.collider_signed_distance(_col(c), lay["pos"][k:k + 1])[0][0] == 0, (k, j)
    _check_rows("conventions", lay, _analytic_ev(lay, lay["cols"]), rows, pids)
    g.destroy()


# ---- shell: generator, query and a second generation agree where membership is undecidable ---------------------------

MESH = dict(make=meshref.icosphere, cell=0.005)


def _mesh_engine(lay, p, R, body, v=(0.05, 0, -0.1), w=(0.3, 1.0, 0)):
    from drake_amd import SdfCollider
    g, pids = _engine(lay)
    verts, tris = MESH["make"]()
    sid = g.sdf_shape_from_mesh(verts, tris, MESH["cell"], 2)
    n, lo, cell = g.sdf_shape_info(sid)
    lattice = (g.sdf_shape_download(sid), n, lo, cell)
    mc = SdfCollider(sid, body=body, p_WB=p, R_WB=R, v=v, w=w)
    g.set_sdf_colliders([mc])
    g.test_mesh_colliders = [mc]
    return g, pids, lattice, mc


def test_shell_generator_query_and_regeneration_agree():
    lay = pl.layout("shell")
    g, pids = _engine(lay)
    _upload_layout(g, pids, lay["pos"], lay["vel"])
    rows = _generate(g, lay["cols"], poison=lay)
    ev = _analytic_ev(lay, lay["cols"])
    present = _check_rows("shell", lay, ev, rows, pids)
    for j, c in enumerate(lay["cols"]):
        phi, _ = g.collider_signed_distance(_col(c), lay["pos"])
        member = np.zeros(lay["n"], bool)
        member[[o for o, k in present if k == j]] = True
        own = lay["own"] == j
        want = (phi < 0) & ~lay["massless"]
        assert np.array_equal(member, want), (pl.KIND_NAMES[c.kind], np.nonzero(member != want)[0][:8])
        assert not own.any() or 0 < member[own].sum() < own.sum()      # both answers occur on a collider's own shell
    again = _generate(g, lay["cols"], poison=lay)
    _same_rows(rows, again, "second generation")
    g.destroy()


def test_shell_of_a_mesh_collider():
    probe = pl.layout("empty")
    p, R = (0.5, 0.5, 0.5), pl.rot((1, 2, 3), 0.9)
    g0, _, lattice, mc = _mesh_engine(probe, p, R, body=1)
    g0.destroy()
    pos = pl.mesh_shell_points(lattice, np.array(mc.p_WB[:], F), np.array(mc.R_WB[:], F), np.random.default_rng(21))
    lay = pl._from_points("shell mesh", 6, pos, [], [], seed=21, massless_at=[p])
    phi64 = pl.mesh_sdf64(lattice, np.array(mc.p_WB[:], F), np.array(mc.R_WB[:], F), pos)[0]
    assert np.abs(phi64).max() <= pl.SHELL_BAND and (phi64 < 0).any() and (phi64 > 0).any()
    g, pids, lattice2, mc = _mesh_engine(lay, p, R, body=1)
    assert np.array_equal(lattice[0], lattice2[0])
    _upload_layout(g, pids, lay["pos"], lay["vel"])
    rows = _generate(g, [], poison=lay)
    ev = [_mesh_ev(lay, lattice, mc)]
    present = _check_rows("shell mesh", lay, ev, rows, pids)
    phi, _ = g.sdf_collider_signed_distance(mc, lay["pos"])
    member = np.zeros(lay["n"], bool)
    member[[o for o, _ in present]] = True
    want = (phi < 0) & ~lay["massless"]
    assert phi[lay["massless"]][0] < 0 and np.array_equal(member, want), np.nonzero(member != want)[0][:8]
    assert 0 < member.sum() < lay["n"]
    _same_rows(rows, _generate(g, [], poison=lay), "second generation")
    g.destroy()


# ---- blocks -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", pl.BLOCK_NP)
def test_blocks_structural_slots_in_both_slot_orders(n):
    lay = pl.layout(f"blocks_{n}")
    engines = [_engine(lay, sort=False, n_bodies=32), _engine(lay, sort=True, n_bodies=32)]
    assert np.array_equal(engines[0][1], np.arange(n)) and not np.array_equal(engines[1][1], np.arange(n))
    for g, pids in engines:
        _upload_layout(g, pids, lay["pos"], lay["vel"])
    slots = pl.block_slots(n)
    for which, (_, pids_of_set) in enumerate(engines):       # the spheres about the structural slots of either order
        particles = pids_of_set[slots]
        for variant in range(3):
            cols, want = pl.block_colliders(lay, particles, variant)
            assert pl.blocks_claims_hold(lay, cols, want)
            ev = _analytic_ev(lay, cols)
            keyed = []
            for e, (g, pids) in enumerate(engines):
                rows = _generate(g, cols, poison=lay)
                tag = f"blocks {n} set {which} variant {variant} {'sorted' if e else 'identity'}"
                present = _check_rows(tag, lay, ev, rows, pids)
                assert len(rows["particle"]) == sum(int(x["din"].sum()) for x in ev) > 0 and rows["overflows"] == 0
                if e == which:      # here the spheres' particles sit at the structural slots: their pairs, in order
                    got = [(int(s), int(b)) for s, b in zip(rows["particle"], rows["body"]) if int(s) in slots]
                    expect = [(s, c.body) for s in slots for q, c in enumerate(cols)
                              if ev[q]["din"][pids[s]]]
                    assert got == expect and len(got) == len(rows["particle"]), tag
                keyed.append(_by_original(rows, pids))
            for f in keyed[0]:
                assert np.array_equal(keyed[0][f], keyed[1][f]), f"blocks {n} set {which} variant {variant}: {f} differs between slot orders"
    for g, _ in engines:
        g.destroy()


# ---- tables -------------------------------------------------------------------------------------------------------------

def _merge(a, b):
    m = {f: np.concatenate([a[f], b[f]]) for f in ROW_FIELDS}
    order = np.lexsort((m["body"], m["particle"]))
    return {f: m[f][order] for f in ROW_FIELDS}


def test_tables_sixteen_and_seventeen_colliders_in_all_instances():
    """(ELL, MESH) in {0, 1}^2: the two count and the four write instances; 16 colliders travel as a kernel argument, 17
    through the device table"""
    common = {}
    for ell in (False, True):
        lay = pl.layout("tables_ell" if ell else "tables")
        cols = lay["cols"]
        for mesh in (False, True):
            tag = f"tables ell={int(ell)} mesh={int(mesh)}"
            mesh_body = len(cols) + MESH_BODY_OFFSET
            if mesh:
                g, pids, lattice, mc = _mesh_engine(lay, tuple(pl.TABLE_CENTRE + (0.02, -0.01, 0.015)), pl.rot((2, 1, -1), 1.7),
                                                    body=mesh_body)
            else:
                g, pids = _engine(lay)
            _upload_layout(g, pids, lay["pos"], lay["vel"])
            ev = _analytic_ev(lay, cols) + ([_mesh_ev(lay, lattice, mc)] if mesh else [])
            all17 = _generate(g, cols, poison=lay)
            present = _check_rows(tag, lay, ev, all17, pids)
            assert sum(1 for o, _ in present if o == lay["where"][0]) == 17 + int(mesh)
            if mesh:
                assert 10 < np.sum(all17["body"] == mesh_body) < lay["n"] - 10
            first16 = _generate(g, cols[:16], poison=lay)
            _check_rows(tag + " first 16", lay, ev[:16] + ev[17:], first16, pids)
            last = _generate(g, cols[16:], poison=lay)
            _check_rows(tag + " the 17th", lay, ev[16:], last, pids)
            keep = last["body"] != mesh_body
            merged = _merge(first16, {f: last[f][keep] for f in ROW_FIELDS})
            _same_rows(all17, merged, tag + ": 17 colliders against 16 + 1")
            # 16 colliders again after 17: back from the device table to the kernel argument
            _same_rows(first16, _generate(g, cols[:16]), tag + ": 16 after 17")
            shared = np.isin(all17["body"], [c.body for k, c in enumerate(cols) if k != 5])
            common[ell, mesh] = {f: all17[f][shared] for f in ROW_FIELDS}
            g.destroy()
    ref = common[False, False]
    assert len(ref["particle"]) > 500
    for key, rows in common.items():
        _same_rows(ref, rows, f"instances (ELL, MESH) = {key} against (False, False) on their common colliders")


# ---- the capacity boundary ----------------------------------------------------------------------------------------------

def _initial_capacity_for(cap):
    """MPM_CT_INITIAL_CAPACITY that gives buffers of exactly `cap` pairs (the engine allocates a quarter more than asked:
    ensure_contact_capacity), or None"""
    for c in range(1, cap + 1):
        if c + c // 4 == cap:
            return c
    return None


def test_capacity_boundary_regrows_without_changing_a_row():
    full = pl.layout("features")
    ev_all = _analytic_ev(full, full["cols"])
    # the leading colliders of `features` whose pair count N and N - 1 are both capacities the engine can have; every pair
    # of the layout is decided, so N is known beforehand
    k = next(k for k in range(6, 0, -1) if _initial_capacity_for(sum(int(e["din"].sum()) for e in ev_all[:k])) and
             _initial_capacity_for(sum(int(e["din"].sum()) for e in ev_all[:k]) - 1))
    lay, ev = dict(full, cols=full["cols"][:k]), ev_all[:k]
    N = sum(int(e["din"].sum()) for e in ev)
    assert k >= 3 and 50 < N < lay["n"]
    g, pids = _engine(lay)
    _upload_layout(g, pids, lay["pos"], lay["vel"])
    ref = _generate(g, lay["cols"], poison=lay)
    g.destroy()
    assert len(ref["particle"]) == N
    for cap, overflows in ((N, 0), (N - 1, 1)):
        g, pids = _engine(lay, env=dict(MPM_CT_INITIAL_CAPACITY=str(_initial_capacity_for(cap))))
        _upload_layout(g, pids, lay["pos"], lay["vel"])
        rows = _generate(g, lay["cols"])              # (no poison: it would size the buffers)
        assert rows["overflows"] == overflows == g.contact_counters()["repeated_overflow"], (cap, rows["overflows"])
        _same_rows(ref, rows, f"capacity {cap}")
        _check_rows(f"capacity {cap}", lay, ev, rows, pids)
        # the regrown buffers, poisoned and generated again: nothing of the poison is left where a solve could read it
        again = _generate(g, lay["cols"], poison=lay)
        _same_rows(ref, again, f"capacity {cap}, after the poison")
        _check_rows(f"capacity {cap}, after the poison", lay, ev, again, pids)
        g.destroy()


# ---- the watch ----------------------------------------------------------------------------------------------------------

def _watch_engine(bits, mesh=None):
    """-> (layout, engine, PIDS, the original ids at the first and the last active index of the faces and of the vertices);
    mesh = (p_WB, R_WB): the engine gets the mesh collider there, and lattice and collider are returned as well"""
    lay = pl.layout("watch" if bits == 6 else "watch8")
    if mesh is None:
        g, pids = _engine(lay)
    else:
        g, pids, lattice, mc = _mesh_engine(lay, mesh[0], mesh[1], body=1)
    imap = g.resort_table("IMAP").astype(np.int64)          # original id -> internal slot
    Nf = g.resort_table("PARAMS")["Nf"]
    T, n = lay["T"], lay["n"]
    assert Nf >= T
    first_face, last_vertex = int(np.nonzero(imap == 0)[0][0]), int(np.nonzero(imap == Nf + (n - T) - 1)[0][0])
    last_face, first_vertex = int(np.nonzero(imap == T - 1)[0][0]), int(np.nonzero(imap == Nf)[0][0])
    assert first_face < T and last_face < T and first_vertex >= T and last_vertex >= T
    ends = dict(face=(first_face, last_face), vertex=(first_vertex, last_vertex))
    return (lay, g, pids, ends) if mesh is None else (lay, g, pids, ends, lattice, mc)


MESH_WATCH_POSE = ((0.5, 0.5, 0.92), pl.rot((1, 2, 3), 0.9))


class _MeshStates:
    """states of the watch layout with ONE vertex moved onto a ray from the mesh collider's body origin: the float64
    interpolant at the float32 state, and its bound, at every watched point"""

    def __init__(self, lay, lattice, mc):
        self.lay, self.lattice = lay, lattice
        self.p, self.R = np.array(mc.p_WB[:], F), np.array(mc.R_WB[:], F)
        self.direction = self.R.astype(D).reshape(3, 3) @ pl._unit((0.3, -0.5, 0.8))

    def at(self, v, r):
        """-> (positions, phi64 (n,), bound (n,)) with vertex v at distance r from the body origin"""
        pos = self.lay["pos"].copy()
        pos[v] = (self.p.astype(D) + r * self.direction).astype(F)
        pts = pl.watch_points(self.lay, pos)
        return pos, pl.mesh_sdf64(self.lattice, self.p, self.R, pts)[0], pl.mesh_bounds(self.lattice, self.p, self.R, pts)["phi"]

    def radius(self, v, reached):
        """the least r in [0.02, 0.08] (to 2^-40) at which reached(phi64 of v, its bound) holds; phi grows with r there"""
        a, b = 0.02, 0.08
        assert not reached(*[x[v] for x in self.at(v, a)[1:]]) and reached(*[x[v] for x in self.at(v, b)[1:]])
        for _ in range(40):
            m = 0.5 * (a + b)
            a, b = (a, m) if reached(*[x[v] for x in self.at(v, m)[1:]]) else (m, b)
        return a, b           # (the last radius where it does not hold, the first where it does)


def _point_bound(c, pts, is_face):
    """the part-1 bound of phi at the watched points, plus one ulp of the centroid the kernel forms for a face"""
    b = pl.bounds(c, pts)["phi"]
    return b + np.where(is_face, np.sqrt(3.0) * 2.0 ** -24, 0.0)      # (coordinates below 1: ulp <= 2^-24)


def _phi_at_watched(lay, c, pos):
    pts = pl.watch_points(lay, pos)
    is_face = np.arange(lay["n"]) < lay["T"]
    return pl.world_sdf64(c, pts)[0], _point_bound(c, pts, is_face)


@pytest.mark.parametrize("bits", [6, 8])
@pytest.mark.parametrize("kind", range(6))
def test_watch_hits_and_misses_per_kind(kind, bits):
    """Must hit: exactly one watched point with phi64 < margin - 8 x bound, at phi in {-0.5 dx, -1e-4 dx, 0.5 margin,
    margin - 8 x bound}, once a vertex and (sphere, box corner, capsule cap) once a face whose corners are decided out,
    at the first and the last active index of its kind.  Must not hit (kinds 0-4, exact): every watched point at
    phi64 >= margin + 8 x bound, one of them at that distance; the ellipsoid only when every point is outside the scaled
    ellipsoid of collider_near by the bound."""
    lay, g, pids, ends = _watch_engine(bits)
    c = lay["cols"][kind]
    ce = [_col(c)]
    margin = float(F(1e-3) * F(lay["dx"]))
    fails = []
    # nothing near: no hit (every kind: the layout keeps 0.03 away, far beyond the ellipsoid's scaling too)
    _upload_layout(g, pids, lay["pos"], lay["vel"])
    assert g.debug_contact_watch(ce) is False
    assert g.debug_contact_watch([_col(k) for k in lay["cols"]]) is False
    whos = ["vertex"] + (["face"] if kind in (1, 2, 3) else [])
    for who in whos:
        for particle in ends[who]:
            b0 = float(_phi_at_watched(lay, c, pl.watch_state(lay, c, margin, who, particle)[0])[1][particle])
            for target in (-0.5 * lay["dx"], -1e-4 * lay["dx"], 0.5 * margin, None):
                if target is None:      # just below margin - 8 x bound
                    target = margin - pl.DECIDE * b0 - 2.0 ** -22
                pos, got = pl.watch_state(lay, c, target, who, particle)
                phi, bnd = _phi_at_watched(lay, c, pos)
                below = phi < margin - pl.DECIDE * bnd
                assert below.sum() == 1 and below[particle] and phi[particle] == got, (who, particle, target, got, np.sort(phi)[:4])
                if who == "face":
                    corners = lay["T"] + lay["idx"][particle]
                    assert np.all(phi[corners] > margin + pl.DECIDE * bnd[corners])
                _upload_layout(g, pids, pos, lay["vel"])
                if g.debug_contact_watch(ce) is not True:
                    fails.append(f"no hit: {who} {particle} at phi64 = {got:.6g} (margin {margin:.6g}, bound {b0:.3g})")
            # must not hit: the same point at margin + 8 x bound, by as little as float32 allows
            floors = [margin + 1.001 * pl.DECIDE * b0]
            if kind == 5:     # (far enough to be outside the scaled ellipsoid as well)
                floors.append(margin + 2.0 * float(c.dims.max()) * margin / float(c.dims.min()))
            for floor in floors:
                pos, got = pl.at_least(lay, c, floor, who, particle)
                phi, bnd = _phi_at_watched(lay, c, pos)
                sure = bool(np.all(phi >= margin + pl.DECIDE * bnd))
                assert sure, (who, particle, got, np.sort(phi)[:3])
                if kind == 5:     # conservative by design: only outside the scaled ellipsoid s E, s = 1 + margin / min a_i
                    s = 1.0 + margin / float(c.dims.min())
                    scaled = pl.Col(5, c.body, p=c.p, R=c.R, dims=c.dims.astype(D) * s)
                    phis = pl.world_sdf64(scaled, pl.watch_points(lay, pos))[0]
                    sure = bool(np.all(phis > pl.DECIDE * bnd * s))
                    assert sure == (floor is floors[-1]), (floor, phis.min())
                _upload_layout(g, pids, pos, lay["vel"])
                if sure and g.debug_contact_watch(ce) is not False:
                    fails.append(f"hit: {who} {particle} at phi64 = {got:.6g} >= margin + 8 x bound (margin {margin:.6g}, bound {b0:.3g})")
    g.destroy()
    assert not fails, f"watch, {pl.KIND_NAMES[kind]}, 2^-{bits}:\n" + "\n".join(fails)


def test_watch_hits_and_misses_of_a_mesh_collider():
    """The mesh instance of the watch.  Must hit: exactly one watched point with phi64 < margin - 8 x bound, a vertex at
    the first and at the last active vertex index, swept over phi in {-0.5 dx, -1e-4 dx, 0.5 margin, margin - 8 x bound} of
    the interpolant.  Must not hit: the same vertex where the interpolant is at least margin + bound, by as little as
    float32 positions allow, and half a cell further out.  (No face state: the mesh is a ball of 0.05, far larger than
    a triangle, so a face's corners cannot all stay outside while its centroid is inside.)"""
    lay, g, pids, ends, lattice, mc = _watch_engine(6, MESH_WATCH_POSE)
    st = _MeshStates(lay, lattice, mc)
    margin = float(F(1e-3) * F(lay["dx"]))
    _upload_layout(g, pids, lay["pos"], lay["vel"])
    assert g.debug_contact_watch([]) is False
    fails = []
    for v in ends["vertex"]:
        for name, target in (("-0.5 dx", -0.5 * lay["dx"]), ("-1e-4 dx", -1e-4 * lay["dx"]), ("0.5 margin", 0.5 * margin),
                             ("margin - 8 x bound", None)):
            if target is None:
                r, _ = st.radius(v, lambda phi, b: phi >= margin - pl.DECIDE * b)      # the last radius below it
            else:
                r, _ = st.radius(v, lambda phi, b: phi >= target)
            pos, phi, bnd = st.at(v, r)
            below = phi < margin - pl.DECIDE * bnd
            assert below.sum() == 1 and below[v], (v, name, phi[v], bnd[v], np.sort(phi)[:3])
            if target is not None:
                assert abs(phi[v] - target) <= 2.0 ** -22, (v, name, phi[v])
            _upload_layout(g, pids, pos, lay["vel"])
            if g.debug_contact_watch([]) is not True:
                fails.append(f"no hit: vertex {v} at interpolant = {phi[v]:.6g} ({name}; margin {margin:.6g}, bound {bnd[v]:.3g})")
        _, r = st.radius(v, lambda phi, b: phi >= margin + b)                           # the first radius at or above it
        for r_out in (r, r + 0.5 * lay["dx"]):
            pos, phi, bnd = st.at(v, r_out)
            assert np.all(phi >= margin + bnd), (v, phi[v], bnd[v])
            _upload_layout(g, pids, pos, lay["vel"])
            if g.debug_contact_watch([]) is not False:
                fails.append(f"hit: vertex {v} at interpolant = {phi[v]:.6g} >= margin + bound (margin {margin:.6g}, bound {bnd[v]:.3g})")
    g.destroy()
    assert not fails, "\n".join(fails)


def test_watch_with_more_than_sixteen_colliders():
    """17 colliders travel through the debug entry's own device table"""
    lay, g, pids, _ = _watch_engine(6)
    _upload_layout(g, pids, lay["pos"], lay["vel"])
    far = [pl.Col(1, 1 + k, p=(0.1 + 0.04 * k, 0.5, 0.92), dims=(0.01, 0, 0)) for k in range(17)]
    assert g.debug_contact_watch([_col(c) for c in far]) is False
    far[16] = pl.Col(1, 17, p=lay["pos"][lay["T"] + 5], dims=(0.01, 0, 0))
    assert g.debug_contact_watch([_col(c) for c in far]) is True
    assert g.debug_contact_watch([_col(c) for c in far[:16]]) is False
    g.destroy()


def test_debug_watch_validates_like_the_generator_and_leaves_the_pairs_alone():
    from drake_amd import Collider, GpuMpm, MpmError
    lay = pl.layout("empty")
    raw = GpuMpm(lay["bits"])
    raw.add_qr_cloth(lay["rest"], np.zeros_like(lay["rest"]), lay["idx"])
    with pytest.raises(MpmError) as e:           # before Finalize's re-sort there are no active counts to walk
        raw.debug_contact_watch([Collider(0, p_WB=(0.5, 0.5, 0.5))])
    assert e.value.code == -1
    raw.destroy()
    g, pids = _engine(lay, n_bodies=8)
    _upload_layout(g, pids, lay["pos"], lay["vel"])
    inside = [pl.Col(0, 1, p=(0.5, 0.5, 0.3), R=pl.rot((1, 0.2, 0), 0.3))]
    rows = _generate(g, inside, poison=lay)
    assert len(rows["particle"]) > 10
    for bad in (Collider(6, dims=(0.1, 0.1, 0.1)), Collider(4, dims=(0.0, 0.1, 0)), Collider(5, dims=(0.1, float("nan"), 0.1)),
                Collider(1, body=8, dims=(0.1, 0, 0))):
        with pytest.raises(MpmError) as e:
            g.debug_contact_watch([_col(inside[0]), bad])
        assert e.value.code == -1
    # a hit on other colliders than the last generation's; the pairs and their colliders stay what they were
    assert g.debug_contact_watch([_col(inside[0])]) is True
    assert g.debug_contact_watch([_col(c) for c in lay["cols"]]) is False
    assert g.contact_pair_count() == len(rows["particle"])
    got = g.download_contact_pairs()
    for f, a in zip(ROW_FIELDS, got):
        assert np.array_equal(rows[f], a), f
    _same_rows(rows, _generate(g, inside), "the generation after the watch")
    g.destroy()


@pytest.mark.parametrize("fast", [False, True])
def test_watch_says_no_means_the_generator_makes_no_pair(fast):
    """The invariant: on every must-not-hit state, and on the same states with one face centroid inside by
    delta in {4 ulp, 0.1 margin, 0.9 margin}, after CalcFemStateAndForce (which forms the centroids the generator reads, by
    / 3 or, with fast math, by the product) no hit implies no pair; on the delta states the watch hits and the generator
    makes the pair."""
    lay, g, pids, ends = _watch_engine(6)
    g.set_fast_math(fast)
    margin = float(F(1e-3) * F(lay["dx"]))
    fails = []
    for kind in range(6):
        c = lay["cols"][kind]
        ce = [_col(c)]
        states = [("far", lay["pos"], None)]
        for who in ["vertex"] + (["face"] if kind in (1, 2, 3) else []):
            particle = ends[who][0]
            b0 = float(_phi_at_watched(lay, c, pl.watch_state(lay, c, margin, who, particle)[0])[1][particle])
            states.append((f"{who} at margin + 8 x bound", pl.at_least(lay, c, margin + 1.001 * pl.DECIDE * b0, who, particle)[0], None))
        if kind in (1, 2, 3):
            particle = ends["face"][1]
            for name, delta in (("4 ulp", 4 * 2.0 ** -24), ("0.1 margin", 0.1 * margin), ("0.9 margin", 0.9 * margin)):
                pos, got = pl.watch_state(lay, c, -delta, "face", particle)
                assert -2 * delta <= got <= -0.5 * delta, (name, got)
                states.append((f"face inside by {name}", pos, particle))
        for name, pos, inside in states:
            _upload_layout(g, pids, pos, lay["vel"] * F(0.0))
            hit = g.debug_contact_watch(ce)
            g.calc_fem_state_and_force(DT)
            n = g.generate_contact_pairs(ce)
            tag = f"{pl.KIND_NAMES[kind]}, {name}: hit = {hit}, pairs = {n}"
            if not hit and n != 0:
                fails.append(tag + " (no hit, yet pairs)")
            if inside is not None:
                rows = g.download_contact_pairs()
                if not hit or n != 1 or pids[int(rows[0][0])] != inside:
                    fails.append(tag + " (expected the hit and the one pair of the face)")
            elif n != 0 or (hit and kind != 5):
                fails.append(tag + " (expected neither)")
    g.destroy()
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("fast", [False, True])
def test_watch_says_no_means_no_pair_for_a_mesh_collider(fast):
    """The same invariant for the mesh instances (k_ct_watch<true> with mesh_below(.., margin) against
    k_ct_gen_count_scan<true> / k_ct_gen_write<*, true> with mesh_below(.., 0)): the far state and a corner of a triangle
    where the interpolant is at least margin + bound make no hit and, after CalcFemStateAndForce, no pair; the corner inside
    by delta in {4 ulp, 0.1 margin, 0.9 margin} makes the hit, never a pair without a hit, and the pair wherever the
    interpolant decides it (below -8 x bound)."""
    lay, g, pids, ends, lattice, mc = _watch_engine(6, MESH_WATCH_POSE)
    g.set_fast_math(fast)
    st = _MeshStates(lay, lattice, mc)
    margin = float(F(1e-3) * F(lay["dx"]))
    v = lay["T"] + lay["E"]            # the first corner of the first triangle: a vertex with mass
    assert not lay["massless"][v]
    states = [("far", lay["pos"], None)]
    _, r = st.radius(v, lambda phi, b: phi >= margin + b)
    for name, r_out in (("corner at margin + bound", r), ("corner half a cell further", r + 0.5 * lay["dx"])):
        pos, phi, bnd = st.at(v, r_out)
        assert np.all(phi >= margin + bnd), (name, phi[v], bnd[v])
        states.append((name, pos, None))
    for name, delta in (("4 ulp", 4 * 2.0 ** -24), ("0.1 margin", 0.1 * margin), ("0.9 margin", 0.9 * margin)):
        r, _ = st.radius(v, lambda phi, b: phi >= -delta)
        pos, phi, bnd = st.at(v, r)
        assert -2 * delta <= phi[v] < -0.5 * delta and np.sum(phi < margin + bnd) == 1, (name, phi[v])
        states.append((f"corner inside by {name}", pos, bool(phi[v] < -pl.DECIDE * bnd[v])))
    assert any(d is True for _, _, d in states)
    fails = []
    for name, pos, decided in states:
        _upload_layout(g, pids, pos, lay["vel"] * F(0.0))
        hit = g.debug_contact_watch([])
        g.calc_fem_state_and_force(DT)
        n = g.generate_contact_pairs([])
        tag = f"mesh, {name}: hit = {hit}, pairs = {n}"
        if not hit and n != 0:
            fails.append(tag + " (no hit, yet pairs)")
        if decided is None:
            if hit or n != 0:
                fails.append(tag + " (expected neither)")
        else:
            rows = g.download_contact_pairs()
            if not hit or n > 1 or (n == 1 and pids[int(rows[0][0])] != v) or (decided and n != 1):
                fails.append(tag + " (expected the hit, and the corner's pair where it is decided)")
    g.destroy()
    assert not fails, "\n".join(fails)
