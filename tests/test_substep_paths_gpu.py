"""Every host path that enqueues a whole substep goes through one statement of the kernel sequence (mpm_engine.hip:
enqueue_substep_front, enqueue_substep_rest).  On the scene of tests/substep_paths.py -- re-sorts and owed substeps on the
way, a vertex of twelve faces so that k_vforce is a launch of its own -- the paths of one family leave the same bits in
positions, velocities, affine and F, with pins behind GridToParticle and with bending stiffness too; the profiler counts
k_vforce under "vforce" whenever it is launched.  (The two families -- fused grid update; gather, then update from sums
-- are not compared with each other.)"""
import numpy as np
import pytest

from tests import substep_paths as sp

pytestmark = pytest.mark.gpu

_CACHE = {}


def _result(name, **scene):
    key = (name, tuple(sorted(scene.items())))
    if key not in _CACHE:
        _CACHE[key] = sp.run(name, **scene)
    return _CACHE[key]


def _same(a, b, what):
    (sa, ta), (sb, tb) = a, b
    for st in (ta, tb):
        assert st["error_flags"] == 0 and st["substeps"] == sp.N, st
        assert st["rebuilds"] > 1, st   # (above Finalize's one: re-sorts on the way)
    assert ta["rebuilds"] == tb["rebuilds"], (what, ta, tb)
    for k in sa:
        assert sa[k].size and np.array_equal(sa[k], sb[k]), (what, k, int((sa[k] != sb[k]).sum()))


@pytest.mark.parametrize("name", ["profile_substeps", "phase_calls", "phase_calls_undeferred"])
def test_fused_family_equals_run_substeps(name):
    _same(_result("run_substeps"), _result(name), name)


def test_sums_family_begin_end_equals_halo_without_zones():
    _same(_result("substep_begin_end"), _result("substep_begin_end_halo"), "halo, no zones")


def test_pinned_profile_equals_run_substeps():
    """two pins on a moving body: k_pin follows k_g2p in both"""
    a, b = _result("run_substeps", pins=True), _result("profile_substeps", pins=True)
    _same(a, b, "pinned")
    assert not np.array_equal(a[0]["pos"], _result("run_substeps")[0]["pos"])   # (the pins do act)


def test_bending_profile_equals_run_substeps_and_times_vforce():
    a, b = _result("run_substeps", bending=True), _result("profile_substeps", bending=True)
    _same(a, b, "bending")
    assert not np.array_equal(a[0]["vel"], _result("run_substeps")[0]["vel"])   # (the stiffness does act)
    g = sp.engine(bending=True)
    ph, total = g.profile_substeps(2, sp.DT, -1)
    g.destroy()
    assert ph["vforce"] > 0 and total > 0, ph


def test_profile_counts_vforce_wherever_it_is_launched():
    """a vertex of more than eight faces, no bending: k_vforce runs, and is the "vforce" phase (not part of "p2g")"""
    g = sp.engine()
    ph, _ = g.profile_substeps(2, sp.DT, -1)
    g.destroy()
    assert ph["vforce"] > 0, ph
