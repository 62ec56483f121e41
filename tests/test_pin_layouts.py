"""tests/pin_layouts.py on the CPU: every regime and body class is present, the layouts stay inside their premises, and
each deliberately wrong restatement of k_pin misses the reference by more than 100 times the stated bound somewhere."""
import numpy as np
import pytest

from tests import anchors as an
from tests import pin_layouts as pl
from tests.pin_reference import pin_target


def _inside(x):
    u = np.asarray(x, np.float64) * pl.DXINV - 0.5
    return bool(np.all((u >= 0) & (u < 2 ** pl.BITS - 2)))


def _clocks_of_schedule(name):
    """the clocks in front of the substeps that tests/test_pin_layouts_gpu.py compares on `many`, `regimes` and `materials`
    (fresh; after 1 + 2 substeps; after 1 + 2 + 1 + 8), and one substep later"""
    return [pl.clock_after([pl.DT] * k) for k in (0, 3, 12, 13)]


def test_many_has_three_workgroups_and_every_body_class():
    for name in ("many", "materials"):
        lay = pl.layout(name)
        c = pl.coverage(lay)
        assert c["n"] == 625 and c["n"] > 512 and c["groups"] == 3
        assert c["bodies"] == [0, 1, 31, 32, 33, 40] and not c["monotone"] and c["cloths"] == [0, 1]
        assert pl.BODY_FAR in c["bodies"] and pl.BODY_NONE in c["bodies"]
        for b in c["bodies"]:
            assert len(c["groups_of"][b]) == 3, (b, c["groups_of"][b])
        assert lay["n_bodies"] == 34 and pl.BODY_NONE >= lay["n_bodies"] > pl.BODY_FAR >= pl.CT_LDS_BODIES
        assert len(set(lay["table"]["vertex"].tolist())) == c["n"]
    d = pl.layout("materials")["densities"]
    assert max(d) / min(d) >= 3


def test_regimes_are_present():
    lay = pl.layout("regimes")
    th = pl.regime_angles(lay)
    assert len(th) == 6
    count = dict(zero=0, series=0, above=0, one=0, pi=0, far=0)
    for b, a in th.items():
        kind = ("zero" if a == 0 else "series" if a < 1e-8 else "above" if a < 2e-8 else "one" if 0.5 < a < 2 else
                "pi" if abs(a - np.pi) < 1e-3 else "far" if a >= 40 else None)
        count[kind] += 1
        p, R, v, w = lay["motions"][b]
        assert np.abs(R - np.eye(3)).max() > 0.1 and np.all(v != 0)
        assert a == 0 or np.all(w != 0)                                   # an oblique axis
        assert (lay["table"]["body"] == b).sum() >= 2
    assert count == dict(zero=1, series=1, above=1, one=1, pi=1, far=1), count
    # the device's branch: th2 < 1e-16 on the angle at t + dt
    assert th[1] ** 2 < 1e-16 < th[2] ** 2


@pytest.mark.parametrize("name", ["many", "regimes", "materials"])
def test_targets_stay_inside_the_domain_and_near_their_vertices(name):
    lay = pl.layout(name)
    t = lay["table"]
    for k, clock in enumerate(_clocks_of_schedule(name)):
        r = pl.restate(t, lay["motions"], clock, lay["dt"])
        assert _inside(r["x"])
        drifted = lay["X"][t["vertex"]].astype(np.float64) + r["t"][0] * np.asarray(pl.DRIFT)
        far = np.abs(r["x"] - drifted).max() * pl.DXINV
        assert far < (2.0 if name == "regimes" else 1.0), (name, k, far)
        assert np.all(r["bx"] < 2.0 ** -24) and np.all(r["bx"] > 0)
    assert len(t) == len(set(t["vertex"].tolist()))


def test_restatement_agrees_with_pin_reference():
    lay = pl.layout("many")
    t = lay["table"][lay["table"]["body"] == 31]
    r = pl.restate(t, lay["motions"], 0.25, lay["dt"])
    x, vq, C = pin_target(lay["motions"][31], t["p_BQ"], 0.25 + float(np.float32(lay["dt"])))
    assert np.array_equal(r["x"], x) and np.array_equal(r["vq"], vq) and np.array_equal(r["C"][0], C.astype(np.float32))
    xb, vb, Cb, bx, bv = pl.pin_bounds(lay["motions"][31], t["p_BQ"], 0.25 + float(np.float32(lay["dt"])))
    assert np.array_equal(xb, x) and np.array_equal(bx, r["bx"]) and np.array_equal(bv, r["bv"])
    assert pl.quantum_of(3.7) == 2.0 ** -45 and pl.quantum_of(4.0) == 2.0 ** -45 and pl.quantum_of(4.1) == 2.0 ** -44


def test_clock_schedule():
    lay = pl.layout("clocks")
    f = lambda d: float(np.float32(d))                                    # noqa: E731
    e = lay["expected"]
    assert len(e) == 18 and len(set(lay["table"]["body"].tolist())) == 18
    assert e[0] == ((((((f(1e-3) + f(5e-4)) + f(7.5e-4)) + f(2.5e-4)) + f(1e-3)) + f(5e-4)) + f(1.25e-4))
    assert e[10] == (((f(2.5e-4) + f(1e-3)) + f(5e-4)) + f(1.25e-4)) and e[17] == e[10] and e[9] == e[0]
    assert e[3] == f(5e-4) + f(1.25e-4)
    assert len({e[0], e[10], e[3]}) == 3
    dts = [d for part in pl.CLOCK_STEPS for d, _ in part]
    assert len(set(dts[:3])) == 3                                         # unequal
    # the second motion of body 3 starts where the first one is
    x_old = pl.restate(lay["table"], lay["motions"], pl.clock_after(dts[:5]), 0.0)["x"]
    x_new = pl.restate(lay["table"], lay["final"], 0.0, 0.0)["x"]
    sel = lay["table"]["body"] == pl.CLOCK_RESET
    assert sel.sum() == 4 and np.abs(x_old[sel] - x_new[sel]).max() < 1e-6
    # a substep more or less, on any body, is far outside the bound
    r = pl.restate(lay["table"], lay["final"], e, 0.0)
    less = pl.restate(lay["table"], lay["final"], {b: t - f(1.25e-4) for b, t in e.items()}, 0.0)
    miss = (np.abs(less["x"] - r["x"]) / r["bx"]).max(axis=1)
    for b in range(18):
        assert miss[lay["table"]["body"] == b].max() > 100, b
    assert _inside(r["x"]) and np.abs(r["x"] - lay["X"][lay["table"]["vertex"]]).max() * pl.DXINV < 0.1


def test_tile_fit_layout():
    lay = pl.layout("tile_fit")
    assert lay["material"]["gravity"] == 0.0 and not lay["v0"].any()      # at rest: k_g2p alone raises nothing
    X, t = lay["X"], lay["table"]
    for x in X:                                                            # every particle well inside its own tile
        fits, inside = pl.tile_verdict(x, pl.block_of(x))
        assert fits and inside
    assert _inside(X)
    blocks = [pl.block_of(X[v]) for v in t["vertex"]]
    assert blocks == [(0, 0, 0), (15, 6, 7), (12, 7, 7)]
    names = [v[0] for v in lay["variants"]]
    assert len(names) == 1 + 12 + 4 and len(set(names)) == len(names)
    seen = set()
    for var in lay["variants"]:
        name, pin, u, left, outside = var
        tab = pl.tile_fit_table(lay, var)
        changed = np.nonzero((tab["p_BQ"] != t["p_BQ"]).any(axis=1))[0]
        assert len(changed) == (0 if name == "fits" else 1) and (name == "fits" or changed[0] == pin)
        r = pl.restate(tab, lay["motions"], 0.0, lay["dt"])
        x32 = r["x"].astype(np.float32)
        assert np.array_equal(x32, tab["p_BQ"]) and np.array_equal(x32.astype(np.float64), r["x"]) and not r["vq"].any()
        verdicts = [pl.tile_verdict(x32[k], blocks[k]) for k in range(3)]
        assert [not (f and i) for f, i in verdicts] == [k == pin and left for k in range(3)], name
        assert [not i for _, i in verdicts] == [k == pin and outside for k in range(3)], name
        # the margins: the moved coordinate is 2^-10 cell from its threshold, every other at least 1/8 cell from any
        uu = x32[pin].astype(np.float64) * pl.DXINV - 0.5
        o = 4 * np.asarray(blocks[pin]) - pl.FREE_ZONE
        edges = np.concatenate([o + pl.GUARD, o + pl.TILE_W - 2 - pl.GUARD, [0.0] * 3, [62.0] * 3]).reshape(4, 3)
        dist = np.abs(uu[None] - edges).min(axis=0)
        near = dist < 0.125
        assert near.sum() == (0 if name == "fits" else 1) and np.all(dist[near] == pl.EPS), (name, dist)
        seen.add((name.split(" ")[0], name.split(" ")[-1]))
    assert len(seen) == 1 + 2 * 2 + 2                                      # fits; lower / upper x -+; domain x -+
    # the six faces and both limits, each from both sides
    faces = {n.rsplit(" ", 1)[0] for n in names if "face" in n}
    assert faces == {f"{s} face {a}" for s in ("lower", "upper") for a in "xyz"}
    assert pl.block_coords(0b111000) == (2, 2, 2) and pl.block_coords(0b100) == (1, 0, 0) and pl.block_coords(0b001) == (0, 0, 1)
    assert pl.tile_verdict(X[0], None) == (False, True)


def _miss(ref, got, what):
    """the worst |got - ref| / bound over the pins (x, vq) or the bodies (f, tau)"""
    b = ref["b" + {"x": "x", "vq": "v", "f": "f", "tau": "tau"}[what]]
    err = np.abs(got[what] - ref[what])
    if what in ("f", "tau"):
        err, ok = err.max(axis=1), b > 0
        return float((err[ok] / b[ok]).max())
    return float((err / b).max())


SENSITIVITY = [   # (wrong restatement, layout, the clock before the substep, the quantities that may show it)
    ("torque_about_pt", "many", 0.0, ("tau",)),
    ("arm_at_t", "many", 0.0, ("x", "vq")),
    ("arm_at_t", "regimes", 0.0, ("x", "vq")),
    ("clock_per_workgroup", "many", pl.clock_after([pl.DT]), ("x", "vq", "f", "tau")),
    ("other_mass", "materials", 0.0, ("f", "tau")),
    ("series_above", "regimes", 0.0, ("x", "vq")),
    ("drop_far", "many", 0.0, ("f", "tau")),
    ("none_into_far", "many", 0.0, ("f", "tau")),
]


@pytest.mark.parametrize("wrong,name,clock,seen_in", SENSITIVITY)
def test_wrong_restatements_are_seen(wrong, name, clock, seen_in):
    lay = pl.layout(name)
    t = lay["table"]
    mass = pl.stand_in_mass(lay)
    q = pl.quantum_of(1250 * mass.max())
    args = dict(n_bodies=lay["n_bodies"], v_g2p=lay["v0"][t["vertex"]], quantum=q)
    ref = pl.restate(t, lay["motions"], clock, lay["dt"], mass=mass, **args)
    got = pl.restate(t, lay["motions"], clock, lay["dt"], mass=pl.stand_in_mass(lay, other=wrong == "other_mass"),
                     wrong=None if wrong == "other_mass" else wrong, **args)
    ratios = {w: _miss(ref, got, w) for w in seen_in}
    print(f"{wrong} on {name}: miss over bound " + ", ".join(f"{w} {r:.3g}" for w, r in ratios.items()))
    assert max(ratios.values()) > 100, ratios
    if wrong == "series_above":                                            # seen on the body at |w| t of about 1
        one = t["body"] == 3
        assert (np.abs(got["x"] - ref["x"]) / ref["bx"])[one].max() > 100
    if wrong in ("drop_far", "none_into_far"):                             # ... on body 33, and nowhere else
        err = np.abs(got["f"] - ref["f"]).max(axis=1)
        assert err[pl.BODY_FAR] > 100 * ref["bf"][pl.BODY_FAR] and not np.delete(err, pl.BODY_FAR).any()
    # the check sees the impulses: every body's sums are far above their bounds
    for b in range(lay["n_bodies"]):
        if ref["count"][b]:
            assert np.abs(ref["f"][b]).max() > 1e3 * ref["bf"][b] and np.abs(ref["tau"][b]).max() > 1e3 * ref["btau"][b], b


def test_bodies_beyond_the_count_receive_nothing():
    lay = pl.layout("many")
    t = lay["table"]
    r = pl.restate(t, lay["motions"], 0.0, lay["dt"], n_bodies=lay["n_bodies"], mass=pl.stand_in_mass(lay),
                   v_g2p=lay["v0"][t["vertex"]], quantum=0.0)
    assert r["f"].shape == (34, 3) and sorted(np.nonzero(r["count"])[0].tolist()) == [0, 1, 31, 32, 33]
    assert r["count"].sum() == len(t) - (t["body"] == pl.BODY_NONE).sum()
    pts = an.points(np.array([(0, 33, t["p_BQ"][4])], an.ANCHOR_DTYPE[["vertex", "body", "p_BQ"]]), lay["motions"], r["t"][33])
    assert t["body"][4] == 33 and np.array_equal(pts[0][0], r["x"][4]) and np.array_equal(pts[1][0], r["vq"][4])
