"""tests/pair_layouts.py on the CPU: every claim of every layout holds under the float64 restatements; a float32 numpy
restatement of the device code, with separate multiplies and adds and with the fused order the device compiles to, stays
inside the module's bounds on every layout and decides every decided pair the way float64 does; `features` has no
undecidable pair.  The worst ratios per layout, kind and field go to tests.helpers.MARGINS."""
import numpy as np
import pytest

from tests import pair_layouts as pl

D = np.float64
NAMES = sorted(pl.LAYOUTS)


def _with_colliders(name):
    """the layout; `blocks` with the spheres about the particles at the structural slots of the identity slot order"""
    lay = pl.layout(name)
    if name.startswith("blocks"):
        lays = []
        for variant in range(3):
            cols, want = pl.block_colliders(lay, pl.block_slots(lay["n"]), variant)
            assert pl.blocks_claims_hold(lay, cols, want), (name, variant)
            lays.append(dict(lay, cols=cols))
        return lays
    return [lay]


@pytest.mark.parametrize("name", NAMES)
def test_every_claim_holds(name):
    lay = pl.layout(name)
    assert lay["claims"], name
    for text, check in lay["claims"]:
        assert check(lay), f"{name}: {text}"
    assert lay["n"] == 4 * lay["T"] + lay["E"] == len(lay["pos"]) == len(lay["vel"]) and lay["massless"].sum() == lay["E"]
    assert len(np.unique(lay["vel"], axis=0)) == lay["n"]
    assert len({c.body for c in lay["cols"]}) == len(lay["cols"]) and all(c.body != pl.POISON_BODY for c in lay["cols"])


def test_features_has_no_undecidable_pair():
    lay = pl.layout("features")
    for j, ev in enumerate(pl.evaluate(lay)):
        und = ~(ev["din"] | ev["dout"])
        assert not und.any(), (j, np.nonzero(und)[0][:5], ev["phi"][und][:5], ev["b"]["phi"][und][:5])
    # every kind has pairs, at every depth
    for j in range(6):
        own = lay["aim_col"] == j
        assert (pl.evaluate(lay)[j]["din"] & own).sum() >= 9


def _check32(lay, tag):
    from tests import helpers
    fails = []
    for c in lay["cols"]:
        phi, grad = pl.world_sdf64(c, lay["pos"])
        b = pl.bounds(c, lay["pos"])
        rv = pl.rigid_v64(c, lay["pos"])
        din, dout = pl.classify(phi, b["phi"])
        for fused in (False, True):
            r = pl.restate32(c, lay["pos"], fused)
            what = f"pair layouts (float32 restatement, {'fused' if fused else 'separate'}): {tag} {pl.KIND_NAMES[c.kind]}"
            ratios = dict(rigid_v=pl.margin(np.abs(r["rv"] - rv).max(1), b["rv"]))
            if r["phi"] is not None:
                ratios["phi"] = pl.margin(np.abs(r["phi"] - phi), b["phi"])
                ratios["grad"] = pl.margin(np.abs(r["grad"] - grad).max(1), b["grad"])
            for field, w in ratios.items():
                helpers.MARGINS.append((w, f"{what} {field}", 1.0, w, w))
                if not w <= 1.0:
                    fails.append(f"{what} {field}: {w:.3g} x the bound")
            if np.any(din & ~r["inside"]) or np.any(dout & r["inside"]):
                fails.append(f"{what}: a decided pair is decided the other way in float32")
    return fails


@pytest.mark.parametrize("name", NAMES)
def test_float32_restatement_stays_inside_the_bounds(name):
    fails = []
    for k, lay in enumerate(_with_colliders(name)):
        fails += _check32(lay, f"{name}/{k}" if name.startswith("blocks") else name)
    assert not fails, "\n".join(fails)


def test_conventions_are_exact_in_float32_too():
    lay = pl.layout("conventions")
    pts = lay["pos"][lay["where"]].astype(D)
    assert np.array_equal(pts, np.round(pts * 8) / 8)
    for fused in (False, True):
        for k, j, phi, g in lay["exact"]:
            k = lay["where"][k]
            r = pl.restate32(lay["cols"][j], lay["pos"][k:k + 1], fused)
            assert r["phi"][0] == phi and np.array_equal(r["grad"][0], np.array(g, np.float32)), (k, j, fused, r["phi"], r["grad"])
    for j, x, phi, g in pl.CONVENTION_QUERIES:
        p64, g64 = pl.world_sdf64(lay["cols"][j], np.array([x], D))
        assert p64[0] == phi and np.array_equal(g64[0], np.array(g, D)), (j, x, p64, g64)


@pytest.mark.parametrize("bits", [6, 8])
@pytest.mark.parametrize("kind", range(6))
def test_watch_states_reach_their_distances(kind, bits):
    """watch_state / at_least put exactly one watched point where they say; everything else stays far"""
    lay = pl.layout("watch" if bits == 6 else "watch8")
    c = lay["cols"][kind]
    margin = pl.WATCH_MARGIN * lay["dx"]
    T, n = lay["T"], lay["n"]
    cases = [("vertex", n - 1), ("vertex", T)] + ([("face", 0), ("face", T - 1)] if kind in (1, 2, 3) else [])
    for who, idx in cases:
        for target in (-0.5 * lay["dx"], -1e-4 * lay["dx"], 0.5 * margin):
            pos, got = pl.watch_state(lay, c, target, who, idx)
            assert abs(got - target) <= 2.0 ** -22, (who, idx, target, got)
            pts = pl.watch_points(lay, pos)
            phi = pl.world_sdf64(c, pts)[0]
            assert phi[idx] == got and np.sum(phi < 0.25 * lay["dx"]) == 1, (who, idx, target, np.sort(phi)[:4])
            if who == "face":       # the corners are decided out, by a wide margin
                corners = T + lay["idx"][idx]
                assert np.all(phi[corners] > 0.25 * lay["dx"]), phi[corners]
        pos, got = pl.at_least(lay, c, 2 * margin, who, idx)
        assert 2 * margin <= got <= 2 * margin + 2.0 ** -22
