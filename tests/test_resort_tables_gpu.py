"""Every table of the conditional re-sort (drake_amd/csrc/mpm_rebuild.h), downloaded through mpm_debug_resort_tables,
against the numpy restatement of tests/resort_reference.py:

    binning layer   the engine's pkey equals the float64 key of the state downloaded before the re-sort (ambiguous
                    particles, within 2^(bits - 21) cells of a boundary, may take either neighbouring cell), and
                    Ctl::quiet_time lies within the rounding bound of its float64 value (ratio to tests.helpers.MARGINS)
    integer layer   from the engine's own pkey: home and active lists, look-up tables over the WHOLE grid, ranges,
                    destinations, wave groups, work items and their order, the three neighbour tables -- exactly
    finish checker  histograms and tickets cleared, control block, permutation, id map, corner references, free zones

on the static layouts of tests/transfer_layouts.py plus two interleaved previous orders (default and deterministic
mode), on sequences of re-sorts (shrink and move, a sheet in motion phase by phase, a batch of whole substeps), and on
the two ranks of a partitioned domain after migrations in both directions."""
import numpy as np
import pytest

from tests import harness as hs
from tests import resort_reference as rr
from tests import transfer_layouts as tl

pytestmark = pytest.mark.gpu
MODES = ("default", "deterministic")


def _before(g, with_state=True):
    """what the next re-sort will read, and the control block it starts from"""
    from drake_amd import ARR as A
    d = dict(ctl=g.resort_table("CTL"), pid=g.resort_table("PID").astype(np.int64))
    if with_state:
        pids = g.download(A.PIDS)
        n = len(pids)
        d["pos"], d["vel"] = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
        d["pos"][pids], d["vel"][pids] = g.download(A.POSITIONS), g.download(A.VELOCITIES)   # by original id
    return d


def _check(g, before, deterministic, where, gravity_axis=None, binning=True, max_ambiguous=0.0, dist=False):
    """the full check of the re-sort that ran since `before`; -> (tables, reference)"""
    from drake_amd import ARR as A
    from drake_amd import GpuMpm
    T = g.resort_tables()
    prm, ctl = T["params"], T["ctl"]
    Nf = prm["Nf"]
    b = before["ctl"]
    nf_in, nv_in = b["nfa"] + b["add_f"], b["nva"] + b["add_v"]
    slots = rr.listed_slots(Nf, nf_in, nv_in)
    prev_pid = before["pid"]
    corner_ids = g.download(A.INDICES).astype(np.int64)
    pos_prev = None
    if binning:
        nfg = len(corner_ids)
        x, v = rr.binned_state(before["pos"], before["vel"], nfg, corners=corner_ids, fem_fast=bool(prm["fem_fast"]))
        xs, vs = x[prev_pid[slots]], v[prev_pid[slots]]
        bn = rr.binning(xs, vs, prm["bits"], prm["anticip"])
        got = T["pkey"].astype(np.int64)[slots]
        ok = rr.accepted_keys(bn, prm["bits"], got)
        assert ok.all(), (f"pkey{where}: {int((~ok).sum())} keys differ from the float64 binning, first previous slot "
                          f"{slots[~ok][0]}: {got[~ok][0]} instead of {bn['key'][~ok][0]} ({bn['dist'][~ok][0]:.3g} cells from a boundary)")
        share = float(bn["ambiguous"].mean())
        assert share <= max_ambiguous, f"{where}: {share:.2%} of the particles are ambiguous"
        mat = GpuMpm.default_material()
        ref_q = rr.quiet_time(xs, vs, rr.key_cells(got), prm["bits"], mat.gravity, gravity_axis, np.ones(len(slots), bool))
        ratio = rr.quiet_ratio(ctl["quiet_time"], ref_q)
        print(f"quiet time{where}: engine {ctl['quiet_time']!r}, float64 {ref_q[0]!r}, allowed [{ref_q[1]!r}, {ref_q[2]!r}], ratio {ratio:.3g}")
        hs.record(f"re-sort tables: quiet time{where}", ratio)
        assert ratio <= 1.0, f"quiet_time{where}: {ctl['quiet_time']!r}, float64 {ref_q[0]!r}, allowed [{ref_q[1]!r}, {ref_q[2]!r}]"
        pos_prev = np.zeros((prm["Np"], 3))
        pos_prev[slots] = xs
    ref = rr.integer_layer(T["pkey"], nf_in, nv_in, prm)
    rr.check_tables(T, ref, prm, deterministic, where)
    rr.check_finish(T, ref, prm, b, where, quiet_is_zero=dist, old_pid=prev_pid, corner_ids=corner_ids, dist=dist,
                    pos_by_prev_slot=pos_prev)
    return T, ref


def _engine(lay, mode):
    from tests.test_transfer_layouts_gpu import _engine as make
    return make(lay, mode)


def _static(name, mode, item_groups_small=None):
    lay = rr.layout(name)
    if item_groups_small is not None:
        lay = dict(lay, env=dict(lay["env"], MPM_ITEM_GROUPS_SMALL=str(item_groups_small)))
    g = _engine(lay, mode)
    try:
        before = _before(g)
        if name.startswith("interleaved"):    # the previous order the layout was built for
            assert np.array_equal(before["pid"], rr.finalize_order(lay)), "Finalize's order is not the predicted one"
        g.rebuild_mapping(False)
        where = f" [{name}{'' if item_groups_small is None else f', items of {item_groups_small}'}, {mode}]"
        T, ref = _check(g, before, mode == "deterministic", where, gravity_axis=lay["gravity_axis"])
        assert T["ctl"]["rebuilds"] == before["ctl"]["rebuilds"] + 1
        return lay, T, ref
    finally:
        g.destroy()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", rr.STATIC_NAMES)
def test_static_layouts(name, mode):
    from tests import helpers
    helpers.tag_default_engine(mode == "default")
    lay, T, ref = _static(name, mode)
    # what the CPU claims promised of this layout, seen in the engine's own tables
    if name == "heavy":
        assert T["home_items"][:, 1].max() >= 2
    if name == "heavy_items":
        assert T["home_items"][:, 1].max() >= 7


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("igs", (16, 4, 1))
def test_heavy_block_split_into_items(igs, mode):
    from tests import helpers
    helpers.tag_default_engine(mode == "default")
    lay, T, ref = _static("heavy", mode, igs)
    assert T["params"]["item_groups_small"] == igs and ref["ig"] == igs
    assert T["home_items"][:, 1].max() >= {16: 2, 4: 7, 1: 25}[igs]


@pytest.mark.parametrize("mode", MODES)
def test_shrink_and_move(mode):
    """two re-sorts, the second with the whole cloth in other and fewer blocks: nothing of the first may survive in the
    look-up tables or the histograms"""
    from drake_amd import ARR as A
    from tests import helpers
    helpers.tag_default_engine(mode == "default")
    lay, second = rr.shrink_states()
    g = _engine(lay, mode)
    try:
        before = _before(g)
        g.rebuild_mapping(False)
        T1, ref1 = _check(g, before, mode == "deterministic", f" [shrink, first, {mode}]", gravity_axis=lay["gravity_axis"])
        pids = g.download(A.PIDS)
        g.upload_particle_state(second["pos"][pids], second["vel"][pids], None, None, None)
        before = _before(g)
        assert before["ctl"]["need_rebuild"] == 1
        g.rebuild_mapping(False)
        T2, ref2 = _check(g, before, mode == "deterministic", f" [shrink, second, {mode}]", gravity_axis=lay["gravity_axis"])
        assert len(T2["home_block"]) < len(T1["home_block"]) and not np.intersect1d(T1["home_block"], T2["home_block"]).size
        assert not np.intersect1d(T1["act_block"], T2["act_block"]).size
        assert g.stats()["error_flags"] == 0
    finally:
        g.destroy()


def _moving_sheet(env, deterministic):
    """a 24 x 24 sheet on the 64^3 grid moving at 0.3 cells per substep along x"""
    from drake_amd import GpuMpm, scenes
    with hs.environ(env):
        g = GpuMpm(6)
    g.set_deterministic(deterministic)
    sheets = scenes.cloth_stack(1, 24, 6, z0=0.5, side=0.25, seed=21, vel_amp=0.2, center=(0.3, 0.5))
    for pos, vel, idx in sheets:
        vel[:, 0] += 4.8
    return scenes.populate(g, sheets)


@pytest.mark.parametrize("mode", MODES)
def test_resorts_of_a_sheet_in_motion(mode):
    """phase calls one by one; every re-sort that happens is checked in full against the state downloaded before it"""
    from tests import helpers
    helpers.tag_default_engine(mode == "default")
    g = _moving_sheet({}, mode == "deterministic")
    try:
        resorts = 0
        for step in range(80):
            before = _before(g)
            g.rebuild_mapping(False)
            if g.resort_table("CTL")["rebuilds"] > before["ctl"]["rebuilds"]:
                resorts += 1
                _check(g, before, mode == "deterministic", f" [motion, substep {step}, {mode}]", gravity_axis=2,
                       max_ambiguous=0.01)
            g.calc_fem_state_and_force(tl.DT)
            g.particle_to_grid(tl.DT)
            g.update_grid(-1)
            g.grid_to_particle(tl.DT)
            if resorts >= 4:
                break
        assert g.stats()["error_flags"] == 0
        assert resorts >= 3, resorts
    finally:
        g.destroy()


@pytest.mark.parametrize("mode", MODES)
def test_tables_after_a_batch_of_substeps(mode):
    """mpm_run_substeps with the re-sort launches before every fourth substep (the lean path): whatever re-sort ran last,
    its tables follow from its own keys and k_rb_finish left everything clean"""
    g = _moving_sheet({"MPM_RESORT_EVERY": "4"}, mode == "deterministic")
    try:
        first = g.resort_table("CTL")
        g.run_substeps(48, tl.DT, -1)
        g.gpu_sync()
        from drake_amd import ARR as A
        T = g.resort_tables()
        prm, ctl = T["params"], T["ctl"]
        assert ctl["rebuilds"] >= first["rebuilds"] + 2, ctl
        ref = rr.integer_layer(T["pkey"], ctl["nfa"], ctl["nva"], prm)
        where = f" [batch, {mode}]"
        rr.check_tables(T, ref, prm, mode == "deterministic", where)
        # (the control block before the last re-sort was not observable: one re-sort earlier, the other particle set)
        rr.check_finish(T, ref, prm, dict(rebuilds=ctl["rebuilds"] - 1, cur=ctl["cur"] ^ 1), where,
                        corner_ids=g.download(A.INDICES).astype(np.int64))
        assert g.stats()["error_flags"] == 0
    finally:
        g.destroy()


def test_partitioned_ranks_after_migrations():
    """two ranks of one domain, one sheet drifting across the cut in each direction: after every re-sort that follows a
    migration, per rank, the integer layer on the listed ranges (active plus appended), the released particles dropped,
    the corner references rebuilt from the id map, and a clean finish without a quiet time"""
    import torch
    from drake_amd import GpuMpm, scenes
    from drake_amd.dist import LocalWorld
    bits = 6
    a = scenes.cloth_stack(1, 20, bits, z0=0.45, side=0.2, seed=31, vel_amp=0.1, center=(0.42, 0.5))
    b = scenes.cloth_stack(1, 20, bits, z0=0.6, side=0.2, seed=32, vel_amp=0.1, center=(0.58, 0.5))
    for pos, vel, idx in a:
        vel[:, 0] += 3.0
    for pos, vel, idx in b:
        vel[:, 0] -= 3.0
    engines = [scenes.populate(GpuMpm(bits), [(p.copy(), v.copy(), i.copy()) for p, v, i in a + b]) for _ in range(2)]
    w = LocalWorld(engines, [0, 8, 16], 2, 0, 0, capacity_blocks=512, migrate_every=0, migrate_capacity=8192,
                   device=torch.device("cuda", 0))
    sent = {0: 0, 1: 0}      # records rank r has sent to the other one
    checked = dropped = 0
    try:
        with torch.cuda.stream(w.stream):
            for step in range(48):
                if all([c.migration_due(tl.DT) for c in w.chains]):
                    w._migrate()
                    w.stream.synchronize()
                    sent[0] += int(w.chains[0].mig_send["r"][:4].cpu().view(torch.int32)[0])
                    sent[1] += int(w.chains[1].mig_send["l"][:4].cpu().view(torch.int32)[0])
                befores = [_before(c.e, with_state=False) for c in w.chains]
                # (LocalWorld._substep, with a look at the tables between the two halves)
                for c in w.chains:
                    c.steps += 1
                    c.mig_elapsed += tl.DT
                    if c._fast_args is None:
                        zones = c._zones()
                        c._fast_args = (c.e.halo_zone_args([z[:3] for z in zones], [c.send[z[3]].data_ptr() for z in zones]),
                                        c.e.halo_buffer_args([c.recv[n].data_ptr() for n in c.recv]))
                    c.e.substep_begin_halo(tl.DT, c._fast_args[0], c.cap)
                for r, c in enumerate(w.chains):
                    bf = befores[r]["ctl"]
                    if bf["need_rebuild"] and (bf["add_f"] or bf["add_v"] or sent[r]):
                        T, ref = _check(c.e, befores[r], False, f" [rank {r}, substep {step}]", binning=False, dist=True)
                        checked += 1
                        dropped += int((ref["seg_lo"] < 0).sum())
                        assert T["params"]["dist_on"] == 1
                w._move(lambda c, n: c.send[n], lambda c: c.recv)
                for c in w.chains:
                    c.e.substep_end_halo(tl.DT, -1, c._fast_args[1], c.cap)
                if sent[0] and sent[1] and checked >= 4 and dropped:
                    break
        w.sync()
        for c in w.chains:
            assert c.e.stats()["error_flags"] == 0
        assert sent[0] > 0 and sent[1] > 0, sent
        assert checked >= 4 and dropped > 0, (checked, dropped)
    finally:
        for g in engines:
            g.destroy()
