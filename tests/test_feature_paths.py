"""tests/feature_paths.py without an engine: the scene covers what tests/test_feature_paths_gpu.py says it does, and
compose64's bound holds for a float32 sum and fails for a sum with a stage dropped or added twice."""
import numpy as np

from tests import feature_paths as fp
from tests import links as lk
from tests import shell_bending as sb


def test_the_scene_has_every_kind_of_link_and_anchor():
    s = fp.scene()
    L, cv = s["link_base"], s["cv"]
    seam = (L["rest_length"] == 0) & (L["flags"] == 0)
    spring = (L["rest_length"] > 0) & (L["flags"] == 0)
    cord = (L["flags"] & lk.TENSION) != 0
    cross = cv[L["a"]] != cv[L["b"]]
    assert seam.sum() >= 8 and (seam & cross).any()                       # the seam between the two sheets
    assert (spring & ~cross).any() and (spring & cross).any()             # a spring inside a sheet, springs between them
    assert cord.sum() == 1 and cord[s["cord"]] and L["a"][s["cord"]] == s["cord_vertex"]
    assert not lk.acts(L, s["X"])[s["cord"]] and lk.acts(L, s["X"])[~cord].all()     # the cord is slack at the start
    rows = np.bincount(np.concatenate([L["a"], L["b"]]), minlength=len(s["X"]))
    assert rows.max() > 8 and rows[fp.HUB] == rows.max()                  # a row longer than a batch of eight
    assert rows[s["cord_vertex"]] == 1                                    # (the cord vertex's link force is the cord's)
    A = s["anchor_base"]
    from tests import anchors as an
    zero = (A["rest_length"] == 0) & (A["flags"] == 0)
    assert zero.any() and ((A["rest_length"] > 0) & (A["flags"] == 0)).any() and ((A["flags"] & an.TENSION) != 0).sum() == 3
    assert set(A["body"][(A["flags"] & an.TENSION) == 0].tolist()) == {0} and set(A["body"][(A["flags"] & an.TENSION) != 0].tolist()) == {1}
    assert set(cv[A["vertex"][A["body"] == 0]].tolist()) == {1} and set(cv[A["vertex"][A["body"] == 1]].tolist()) == {2}
    # every anchor acts at the start: the cords are taut, the springs off their rest lengths
    y = an.points(A, s["motions"], 0.0)[0]
    l = np.linalg.norm(y - s["X"][A["vertex"]].astype(np.float64), axis=1)
    assert (l > A["rest_length"] + 5e-4).all()
    assert {q[0] for q in s["pins"]} == set(fp.PINS) and all(cv[q[0]] == 0 and q[1] == 0 for q in s["pins"])


def test_the_bodies_move_as_stated():
    m = fp.scene()["motions"]
    assert set(m) == {0, 1}                                               # (body 2 is the contact collider's: no motion)
    assert np.array_equal(m[0][2], np.array(fp.BODY0_V, np.float32)) and not m[0][3].any()       # translates with the cloth
    assert m[1][2].any() and m[1][3].any()                                # translates and spins
    assert np.array_equal(m[0][1], np.eye(3, dtype=np.float32))


def test_the_meshes():
    from drake_amd import GpuMpm
    s = fp.scene()
    cloths, first = s["cloths"], s["first"]
    closed = [GpuMpm.mesh_is_closed(T, len(X))[0] for X, _, T in cloths]
    assert closed == [False, False, True, False]
    assert s["pressure"]["mode"].tolist() == [1, 0, 2, 0]                 # constant on an open sheet, off, gas, off
    assert np.bincount(cloths[3][2].reshape(-1))[0] == 12                 # the fan's hub: more than k_vforce's eight records
    # the shell's rest shape: curved on sheet 1, nowhere degenerate
    for c in (1, 2):
        X, _, T = cloths[c]
        rest = s["rest"][first[c]:first[c + 1]].astype(np.float64)
        area = 0.5 * np.linalg.norm(np.cross(rest[T[:, 1]] - rest[T[:, 0]], rest[T[:, 2]] - rest[T[:, 0]]), axis=1)
        H = sb.hinges(T)
        edge = np.linalg.norm(rest[H[:, 1]] - rest[H[:, 0]], axis=1)
        assert len(H) and area.min() > 1e-6 and edge.min() > 1e-3, (c, area.min(), edge.min())
        psi = sb.psi64(rest, H)
        assert np.abs(psi).max() > 1e-3, c                                # (curved: the rest angles are not zero)
    # (sheet 1 as added is jittered, not flat; its rest shape is that rolled up: other rest angles than the mesh's own)
    H = sb.hinges(cloths[1][2])
    added, rest = s["X"][first[1]:first[2]].astype(np.float64), s["rest"][first[1]:first[2]].astype(np.float64)
    assert np.abs(sb.psi64(rest, H) - sb.psi64(added, H)).max() > 1e-2
    assert np.array_equal(s["rest"][first[2]:], s["X"][first[2]:]) and np.array_equal(s["rest"][:first[1]], s["X"][:first[1]])
    # everything drifts at 2 m/s along x
    assert abs(float(s["V"][:, 0].mean()) - 2.0) < 0.05
    assert fp.N * fp.DT * 2.0 > 2 * fp.DX                                 # more than two cells on the way: re-sorts


def test_chain_features():
    assert fp.chain_features(0) == fp.FACE_PASS and fp.chain_features(len(fp.CHAIN)) == fp.FACE_PASS | set(fp.CHAIN)
    assert [len(fp.chain_features(k)) for k in range(7)] == list(range(2, 9))
    assert sum(fp.BATCHES) == fp.N and sum(fp.COUPLED_CALLS) == fp.N and fp.COUPLED_CALLS[0] != fp.COUPLED_CALLS[1]


def _stages(n=10_000, seed=1):
    r = np.random.default_rng(seed)
    # seven stages of very different sizes and signs, as the chain's are
    return [(s * r.normal(size=(n, 3))).astype(np.float32) for s in (3.0, 0.5, 1e-2, 2.0, 0.7, 1e-3, 1.5)]


def _sum32(stages):
    tot = stages[0].copy()
    for a in stages[1:]:
        tot = (tot + a).astype(np.float32)           # numpy's float32 addition: one rounding per stage
    return tot


def test_compose64_bounds_a_float32_sum_and_catches_a_stage_dropped_or_doubled():
    stages = _stages()
    tot = _sum32(stages)
    partial, bound = fp.compose64(stages)
    assert partial.shape == (7, 10_000, 3) and bound.shape == (10_000, 3) and (bound > 0).all()
    assert np.array_equal(partial[0], stages[0].astype(np.float64))
    w = fp.compose_margin(tot, stages)
    assert 0.0 < w <= 1.0, w
    for k in range(1, 7):
        dropped = _sum32(stages[:k] + stages[k + 1:])
        doubled = _sum32(stages[:k + 1] + stages[k:])
        assert fp.compose_margin(dropped, stages) > 100, k
        assert fp.compose_margin(doubled, stages) > 100, k
    # the order is part of it only through the partial sums: the same stages in another order still sum within ITS bound
    assert fp.compose_margin(_sum32(stages[::-1]), stages[::-1]) <= 1.0
    # sum_margin: one rounding of one addition
    a, b = stages[0], stages[3]
    assert fp.sum_margin((a + b).astype(np.float32), a, b) <= 1.0
    assert fp.sum_margin((a + b + b).astype(np.float32), a, b) > 1e3
