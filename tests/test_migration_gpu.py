"""The partition's migration kernels (k_dist_init_roles, k_dist_classify, dist_emit, k_dist_apply, k_dist_mig_reduce of
drake_amd/csrc/mpm_dist.h) and their host side (mpm_dist_host.h: mpm_dist_init, mpm_dist_retune, plan_migration,
mpm_dist_migrate_pack / apply) against the exact restatement and the layouts of tests/migration.py, with all ranks in one process
(drake_amd.dist.LocalWorld).

One stage: upload_particle_state(pos, vel) on every rank (written where the rank has a slot; the role is left alone),
LocalWorld.migrate(), rebuild_mapping(False) on every rank.  An upload of positions itself forces the next re-sort, so
on the stages that keep the drift contract a rebuild_mapping(False) BEFORE the migration takes that re-sort: from
there the `rebuilds` counter moves exactly when the migration forces a re-sort (a release or an arriving record).  On the
stages that jump (thresholds, promotion) that extra re-sort is left out: it would judge an owned particle that sits
cells beyond the cut before the migration has handed it over.

After every stage, per rank: roles, error flags, both send buffers (header counts, the set of (id, role) from the first
two words of every record), the held counts, the slot space against mpm_dist_plan_migration, the `rebuilds` counter,
what arrived against the sender's copy bit for bit, and Ctl::mig_quiet within the rounding bound of the module.  After
the last stage one substep of the world against one substep of a single engine from the same state.

mpm_dist_retune needs a partitioned engine: the table of (quiet time, dt) pairs is here, not in tests/test_migration.py."""
import ctypes as C
import time

import numpy as np
import pytest

from tests import migration as mg

pytestmark = pytest.mark.gpu
DT = mg.DT
_IDS = [n if c is None else f"{n}-{c[0]}r-z{c[1]}-b{c[2]}{c[3]}" for n, c in mg.EXACT]


def _pin_env(monkeypatch, retune):
    """everything a result here depends on, so that the environment cannot change what is asserted"""
    monkeypatch.setenv("MPM_DIST_RETUNE", "1" if retune else "0")
    monkeypatch.setenv("MPM_DIST_DRIFT", "0.5")
    monkeypatch.setenv("MPM_MIG_SAFETY", "0.5")
    monkeypatch.setenv("MPM_DIST_INTERVAL", "16")
    monkeypatch.delenv("MPM_DIST_HEADROOM", raising=False)


def _engine(lay):
    from drake_amd import GpuMpm
    m = GpuMpm.default_material()
    m.gravity_axis = lay["gravity_axis"]
    m.gravity = lay["gravity"]
    g = GpuMpm(lay["bits"], m)
    rest, vel, idx = lay["cloth"]
    g.add_qr_cloth(rest.copy(), vel.copy(), idx.copy())
    g.finalize()
    return g


def _extra_state(lay):
    """affine matrices and deformation gradients that are not all alike, so that 'the particle arrived intact' says
    something: |C| <= 0.05 / s, F = I + 1e-3"""
    rng = np.random.default_rng(99)
    aff = (0.05 * rng.uniform(-1, 1, (lay["n"], 9))).astype(np.float32)
    F = (np.eye(3).reshape(1, 9) + 1e-3 * rng.uniform(-1, 1, (lay["nf"], 9))).astype(np.float32)
    return aff, F


class _World:
    def __init__(self, lay, capacity=None, capacity_blocks=512):
        import torch
        from drake_amd import ARR
        from drake_amd.dist import LocalWorld
        self.lay = lay
        self.ref = _engine(lay)
        self.pos0 = self.ref.download(ARR.POSITIONS)
        self.engines = [_engine(lay) for _ in range(len(lay["cuts"]) - 1)]
        # (a fixed cadence that never comes due: LocalWorld.migrate() then neither agrees on a quiet time nor re-tunes)
        self.w = LocalWorld(self.engines, lay["cuts"], lay["zone_blocks"], lay["ghost_cells"], lay["ghost_margin_cells"],
                            capacity_blocks=capacity_blocks, migrate_every=1000,
                            migrate_capacity=lay["capacity"] if capacity is None else capacity, device=torch.device("cuda", 0))
        self.roles0 = [e.dist_roles() for e in self.engines]
        self.aff, self.F = _extra_state(lay)
        for e in self.engines + [self.ref]:
            e.upload_particle_state(affine=self.aff, deformation_gradients=self.F)

    def rules(self):
        """band widths as every rank's engine reports them: bit for bit what the module derives from the mesh"""
        lay = self.lay
        for e in self.engines:
            g = e.dist_geometry()
            r = mg.rules_from_geometry(g, lay["zone_blocks"], lay["ghost_cells"], lay["ghost_margin_cells"])
            for k in ("ghost_w", "vert_w", "mig_delta", "mig_reach", "hyst", "reach", "longest_edge"):
                assert r[k] == lay["rules"][k], (k, float(r[k]), float(lay["rules"][k]), g)
        return r

    def destroy(self):
        for e in self.engines + [self.ref]:
            e.destroy()


def _records(buf, limit=None):
    """-> header (4 uint32), (n, 2) int array of (id, role) sorted by id; limit: the buffer's capacity, where the header
    counts more records than were written"""
    raw = buf.cpu().numpy()
    hdr = raw[:16].view(np.uint32).copy()
    n = int(hdr[0]) if limit is None else min(int(hdr[0]), limit)
    rec = raw[16:16 + n * 144].view(np.int32).reshape(n, 36)[:, :2].astype(np.int64)
    return hdr, rec[np.argsort(rec[:, 0], kind="stable")]


def _sorted(recs):
    recs = np.asarray(recs, np.int64).reshape(-1, 2)
    return recs[np.argsort(recs[:, 0], kind="stable")]


_ARRS = ("POSITIONS", "VELOCITIES", "AFFINE", "VOLUMES", "DEFORMATION_GRADIENTS")


def _snapshot(e):
    from drake_amd import ARR
    return {a: e.download(getattr(ARR, a)) for a in _ARRS}


def _plan_through_the_binding(hl, hr, cap, nf, nv, held, slots):
    from drake_amd import capi
    lib = capi.load_library()
    out = (C.c_size_t * 6)()
    a = None if hl is None else np.array([hl[0], hl[1], 0, 0], np.uint32)
    b = None if hr is None else np.array([hr[0], hr[1], 0, 0], np.uint32)
    rc = lib.mpm_dist_plan_migration(None if a is None else a.ctypes.data_as(C.c_void_p),
                                     None if b is None else b.ctypes.data_as(C.c_void_p), cap, nf, nv, held[0], held[1], slots[0],
                                     slots[1], C.c_float(1.5), out)
    assert rc == 0
    return list(out)


def _check_quiet(name, s, r, got, interval, worst):
    lo, hi = interval
    if not np.isfinite(lo):
        assert got == np.inf, (name, s, r, got)
        return
    assert np.isfinite(got), (name, s, r, got, interval)
    mid = 0.5 * (lo + hi)
    ratio = abs(got - mid) / (0.5 * (hi - lo))     # (the interval is [t (1 - K b), t (1 + K b)] of the particle that decides)
    worst.append((ratio, f"{name} stage {s} rank {r}"))
    print(f"quiet time {name} stage {s} rank {r}: engine {got!r} model [{lo!r}, {hi!r}] -> {ratio:.3f} of the bound")


def _run_stages(W, res, worst_quiet):
    """every stage of the layout through the world, asserting against `res` (migration.replay)"""
    import torch
    lay, w = W.lay, W.w
    name, nf, n = lay["name"], lay["nf"], lay["n"]
    world = len(W.engines)
    for r, e in enumerate(W.engines):
        assert np.array_equal(W.roles0[r], res[0][r]), (name, "roles after mpm_dist_init", r)
        assert e.stats()["error_flags"] == 0
    for s, st in enumerate(lay["stages"][1:], 1):
        if st["retune"] is not None:
            for r, e in enumerate(W.engines):
                changed = e.dist_retune(*st["retune"])
                assert changed == res[s][r]["retuned"], (name, s, r)
                g = e.dist_geometry()
                got = (np.float32(g["face_band_cells"]), np.float32(g["vertex_band_cells"]), np.float32(g["drift_budget_cells"]))
                assert got == tuple(res[s][r]["bands"]), (name, s, r, got, res[s][r]["bands"])
        for e in W.engines:
            e.upload_particle_state(pos=st["pos"], vel=st["vel"])
        if st["contract"]:
            for e in W.engines:
                e.rebuild_mapping(False)
        before = [_snapshot(e) for e in W.engines]
        stats0 = [e.stats() for e in W.engines]
        w.migrate()
        for e in W.engines:
            e.rebuild_mapping(False)
        w.sync()
        w.stream.synchronize()
        torch.cuda.synchronize()
        after = [_snapshot(e) for e in W.engines]
        for r, e in enumerate(W.engines):
            d = res[s][r]
            what = (name, "stage", s, "rank", r)
            st1 = e.stats()
            assert st1["error_flags"] == 0 and d["flags"] == 0, (what, st1)
            # the two send buffers, as packed (the copy to the neighbour does not touch them)
            c = w.chains[r]
            for side, key in (("l", "left"), ("r", "right")):
                hdr, rec = _records(c.mig_send[side])
                assert (int(hdr[0]), int(hdr[1])) == d["header_" + side] and hdr[2] == 0 and hdr[3] == 0, (what, side, hdr, d["header_" + side])
                assert np.array_equal(rec, _sorted(d[key])), (what, side, "records")
            roles = e.dist_roles()
            bad = np.nonzero(roles != d["roles"])[0]
            assert not len(bad), (what, "roles", bad[:8], roles[bad[:8]], d["roles"][bad[:8]])
            assert (st1["active_faces"], st1["active_vertices"]) == d["held"], (what, st1, d["held"])
            # slot space: what plan_migration says for the headers that arrived, grown only when the need exceeds it
            hl = res[s][r - 1]["header_r"] if r > 0 else None
            hr = res[s][r + 1]["header_l"] if r < world - 1 else None
            slots0 = (stats0[r]["face_slots"], stats0[r]["vertex_slots"])
            held0 = (stats0[r]["active_faces"], stats0[r]["active_vertices"])
            if st["contract"]:
                assert held0 == d["active_before"], (what, held0, d["active_before"])
            plan = _plan_through_the_binding(hl, hr, c.mig_cap, nf, n - nf, held0, slots0)
            assert plan[:2] == [d["in_f"], d["in_v"]], (what, plan, d["in_f"], d["in_v"])
            assert (st1["face_slots"], st1["vertex_slots"]) == (plan[4], plan[5]), (what, st1, plan)
            grew = (st1["face_slots"], st1["vertex_slots"]) != slots0
            assert grew == (plan[2] > slots0[0] or plan[3] > slots0[1]), (what, plan, slots0)
            assert plan[2:] == list(mg.plan(d["in_f"], d["in_v"], nf, n - nf, held0[0], held0[1], slots0[0], slots0[1]))
            if st["contract"]:
                assert st1["rebuilds"] - stats0[r]["rebuilds"] == int(d["forced"]), (what, "rebuilds", stats0[r]["rebuilds"], st1["rebuilds"], d["forced"])
            # what arrived is the sender's particle, bit for bit
            for src, key in ((r - 1, "right"), (r + 1, "left")):
                if src < 0 or src >= world or not len(res[s][src][key]):
                    continue
                ids = np.asarray(res[s][src][key])[:, 0]
                for a in _ARRS:
                    sel = ids[ids < nf] if a == "DEFORMATION_GRADIENTS" else ids
                    x, y = before[src][a][sel], after[r][a][sel]
                    assert not np.isnan(x).any() and x.tobytes() == y.tobytes(), (what, "arrived from", src, a)
            _check_quiet(name, s, r, e.dist_migration_quiet_time(), d["quiet_interval"], worst_quiet)


def _substep_against_a_single_engine(W, st):
    """one substep of the world and of a single engine from the layout's last state"""
    from drake_amd import ARR
    from tests.helpers import close
    from tests.test_world_gpu import _collect
    lay = W.lay
    W.ref.upload_particle_state(pos=st["pos"], vel=st["vel"])
    W.ref.substep(DT, -1)
    W.ref.gpu_sync()
    assert W.ref.stats()["error_flags"] == 0
    rp, rv = W.ref.download(ARR.POSITIONS), W.ref.download(ARR.VELOCITIES)
    W.w.substep(DT, -1)
    W.w.sync()
    pos, vel, F, per_rank = _collect(W.w, W.roles0, lay["n"], lay["nf"], every_rank_has_ghosts=False)
    vs = max(float(np.abs(rv).max()), 1.0)
    close(pos, rp, scale=1.0, rtol=1e-5, what=f"migration {lay['name']}: positions after a substep vs single engine")
    close(vel, rv, scale=vs, rtol=1e-4, what=f"migration {lay['name']}: velocities after a substep vs single engine")


@pytest.mark.parametrize("name,cfg", mg.EXACT, ids=_IDS)
def test_migration_against_the_restatement(name, cfg, monkeypatch):
    from tests import helpers
    t0 = time.time()
    lay = mg.layout(name, cfg)
    _pin_env(monkeypatch, retune=name == "retune")
    W = _World(lay, capacity_blocks=1024 if name == "bulk" else 512)
    try:
        rules = W.rules()
        res = mg.replay(lay, rules=rules, pos0=W.pos0)
        worst = []
        _run_stages(W, res, worst)
        if worst:
            ratio, where = max(worst)
            helpers.MARGINS.append((ratio, f"migration: quiet time {name}{'' if cfg is None else cfg} ({where})", 1.0, ratio, ratio))
            assert ratio <= 1.0, (ratio, where)
        if name.startswith("quiet"):
            assert len(worst) >= (6 if lay["gravity_axis"] == 0 else 4), worst
        _substep_against_a_single_engine(W, lay["stages"][-1])
    finally:
        W.destroy()
    print(f"{name} {cfg}: {time.time() - t0:.1f} s")


def test_retune_agrees_with_the_host_rule_on_a_table(monkeypatch):
    """mpm_dist_retune through the binding against MigrationModel.retune: 0, infinity, NaN, negative values, the
    clamps at both ends, the eighth-of-a-cell rounding and the 0.06 dead band (reached in the one-block zone, whose
    limit 0.2708 is 0.0208 from the eighth below it), each call from the state the one before left"""
    _pin_env(monkeypatch, retune=True)
    table = [(t, dt) for dt in (1e-3, 2.5e-4) for t in (0.0165, 0.0, float("inf"), float("nan"), -1.0, 1e-9, 0.004, 0.0165, 0.03,
                                                         0.0625, 0.1, 0.5, 3.0, 1e30, 0.016, 0.032, 0.0321, 0.0319)]
    table += [(0.0165, 0.0), (0.0165, -1.0), (0.0165, float("nan"))]
    dead = 0
    for name, cfg in (("retune", None), ("there_and_back", (2, 1, 0, 0))):
        lay = mg.layout(name, cfg)
        W = _World(lay)
        try:
            m = mg.model_of(lay, rules=W.rules())
            e = W.engines[0]
            for t, dt in table:
                was = m.ranks[0].mig_delta
                want_changed = m.retune(0, t, dt)
                assert e.dist_retune(t, dt) == want_changed, (name, t, dt)
                g = e.dist_geometry()
                R = m.ranks[0]
                got = tuple(np.float32(g[k]) for k in ("face_band_cells", "vertex_band_cells", "drift_budget_cells"))
                assert got == (R.ghost_w, R.vert_w, R.mig_delta), (name, t, dt, got, (R.ghost_w, R.vert_w, R.mig_delta))
                if not want_changed and dt > 0 and t > 0 and np.isfinite(t) and m.last_want != was:
                    dead += 1
            assert e.dist_geometry()["retunes"] >= 4
        finally:
            W.destroy()
    assert dead >= 1


def test_retune_switched_off_leaves_the_bands_alone(monkeypatch):
    _pin_env(monkeypatch, retune=False)
    lay = mg.layout("retune")
    W = _World(lay)
    try:
        g0 = W.engines[0].dist_geometry()
        assert not W.engines[0].dist_retune(0.0165, DT) and W.engines[0].dist_geometry() == g0
        m = mg.model_of(lay, retune_on=False)
        assert not m.retune(0, 0.0165, DT)
    finally:
        W.destroy()


def test_a_particle_beyond_the_neighbours_slab_raises_the_halo_flag_on_the_sender(monkeypatch):
    _pin_env(monkeypatch, retune=False)
    lay = mg.layout("contract_halo")
    W = _World(lay)
    try:
        res = mg.replay(lay, rules=W.rules(), pos0=W.pos0)
        st = lay["stages"][1]
        for e in W.engines:
            e.upload_particle_state(pos=st["pos"], vel=st["vel"])
        import torch
        with torch.cuda.stream(W.w.stream):
            for c in W.w.chains:
                c.e.dist_migrate_pack(c.mig_send["l"].data_ptr(), c.mig_send["r"].data_ptr(), c.mig_cap)
        W.w.stream.synchronize()
        flags = [e.stats()["error_flags"] for e in W.engines]
        assert [f & mg.ERR_HALO for f in flags] == [res[1][r]["flags"] & mg.ERR_HALO for r in range(3)] == [mg.ERR_HALO, 0, 0], flags
        assert all(f & ~mg.ERR_HALO == 0 for f in flags), flags
    finally:
        W.destroy()


def test_a_buffer_one_record_short_is_refused_by_the_receiver(monkeypatch):
    """the sender raises the capacity flag, its header still counts every record; dist_migrate_apply on the receiver
    returns the capacity error and stores nothing"""
    import torch
    from drake_amd import ARR, MpmError
    _pin_env(monkeypatch, retune=False)
    lay = mg.layout("contract_capacity")
    n_rec = mg.replay(lay)[1][0]["header_r"][0]
    W = _World(lay, capacity=n_rec - 1)
    try:
        res = mg.replay(lay, rules=W.rules(), pos0=W.pos0, cap=n_rec - 1)
        assert res[1][0]["header_r"][0] == n_rec and res[1][0]["flags"] == mg.ERR_CAPACITY
        st = lay["stages"][1]
        for e in W.engines:
            e.upload_particle_state(pos=st["pos"], vel=st["vel"])
            e.rebuild_mapping(False)
        w = W.w
        c0, c1 = w.chains
        roles1, pos1, st1 = c1.e.dist_roles(), c1.e.download(ARR.POSITIONS), c1.e.stats()
        with torch.cuda.stream(w.stream):
            for c in w.chains:
                c.e.dist_migrate_pack(c.mig_send["l"].data_ptr(), c.mig_send["r"].data_ptr(), c.mig_cap)
            w._move(lambda c, n: c.mig_send["l" if n == c.left else "r"], lambda c: c.mig_recv)
        w.stream.synchronize()
        hdr, rec = _records(c0.mig_send["r"], limit=n_rec - 1)
        full_hdr = c0.mig_send["r"][:16].cpu().numpy().view(np.uint32)
        assert (int(full_hdr[0]), int(full_hdr[1])) == res[1][0]["header_r"], full_hdr
        # the n - 1 records that fitted are records of the model's list
        want = _sorted(res[1][0]["right"])
        assert len(rec) == n_rec - 1 and all(tuple(x) in {tuple(y) for y in want} for x in rec)
        assert c0.e.stats()["error_flags"] == mg.ERR_CAPACITY and c1.e.stats()["error_flags"] == 0
        with pytest.raises(MpmError) as err:
            with torch.cuda.stream(w.stream):
                c1.e.dist_migrate_apply(c1.mig_recv[c1.left].data_ptr(), None, c1.mig_cap)
        assert err.value.code == -4, err.value       # MPM_ERR_CAPACITY
        w.stream.synchronize()
        st2 = c1.e.stats()
        assert np.array_equal(c1.e.dist_roles(), roles1) and c1.e.download(ARR.POSITIONS).tobytes() == pos1.tobytes()
        assert (st2["active_faces"], st2["active_vertices"], st2["face_slots"], st2["vertex_slots"]) == \
            (st1["active_faces"], st1["active_vertices"], st1["face_slots"], st1["vertex_slots"])
    finally:
        W.destroy()


def test_a_sheet_moving_leftwards_across_both_cuts_matches_a_single_engine(monkeypatch):
    """the mirror image of tests/test_domain_gpu.py's scene: a regular sheet drifts in -x over the two cuts of the
    three-rank partition by real substeps (owners hand particles to their LEFT neighbours)"""
    from drake_amd import ARR, GpuMpm, scenes
    from tests.helpers import close
    from tests.test_world_gpu import _collect, _populate, _run_world
    _pin_env(monkeypatch, retune=True)
    bits, steps = 6, 40
    sheets = scenes.cloth_stack(3, 40, bits, z0=0.5, side=0.4, seed=21, vel_amp=0.3)
    for pos, vel, idx in sheets:
        vel[:, 0] -= 1.2      # 0.077 cells per substep: 3 cells over the run
    ref = _populate(GpuMpm(bits), sheets)
    x0 = ref.download(ARR.POSITIONS)
    ref.run_substeps(steps, DT, -1)
    ref.gpu_sync()
    rp, rv, rF = ref.download(ARR.POSITIONS), ref.download(ARR.VELOCITIES), ref.download(ARR.DEFORMATION_GRADIENTS)
    n, nf = ref.n_particles, ref.n_faces
    geo = dict(cuts=[0, 6, 10, 16], zone_blocks=2, ghost_cells=0, ghost_margin_cells=0, migrate_every=0)
    roles0, w = _run_world(bits, sheets, geo, steps, capacity_blocks=512, migrate_capacity=8192)
    pos, vel, F, per_rank = _collect(w, roles0, n, nf)
    vs = max(float(np.abs(rv).max()), 1.0)
    close(pos, rp, scale=1.0, rtol=1e-5, what="leftward sheet: positions vs single engine")
    close(vel, rv, scale=vs, rtol=1e-4, what="leftward sheet: velocities vs single engine")
    close(F, rF, scale=1.0, rtol=1e-4, what="leftward sheet: F vs single engine")
    cell0 = np.minimum((x0[:, 0] * (1 << bits) - 0.5).astype(np.int64), (1 << bits) - 3)
    start_owner = np.searchsorted(np.array(geo["cuts"][1:-1]) * 4, cell0, side="right")
    end_owner = np.argmax(np.stack([pr[0] == 1 for pr in per_rank]), axis=0)
    assert np.count_nonzero(end_owner < start_owner) > n // 50 and not np.any(end_owner > start_owner)
    assert np.any((start_owner == 2) & (end_owner == 1)) and np.any((start_owner == 1) & (end_owner == 0))
    assert w.migrations >= 3, w.migrations
    for c in w.chains:
        c.e.destroy()
    ref.destroy()
