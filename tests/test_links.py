"""Links between cloth vertices on the CPU: mpm_link_force -- the inline function the link kernel calls, compiled for the
host -- against the float64 restatement of tests/links.py inside the per-link bound R_link 2^-24 S on random links of
every branch; the bitwise antisymmetry that lets a gather kernel conserve momentum; the seam's linearity; the
tension-only gate at l == L and one ulp either side; the zero below |d|^2 = 1e-30; and the restatement itself against
its own energy by central differences."""
import numpy as np
import pytest

from tests import links as lk

U = lk.U


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _force(link, xa, xb, va, vb):
    from drake_amd import link_force
    return link_force(link, xa, xb, va, vb)


def test_exports():
    from drake_amd import capi
    lib = capi.load_library()
    for name in ("mpm_set_links", "mpm_get_links", "mpm_link_forces", "mpm_link_energy", "mpm_links_max_stable_dt",
                 "mpm_link_force"):
        assert name in capi.SYMBOLS and hasattr(lib, name), name
    assert capi.LINK_DTYPE == lk.LINK_DTYPE and capi.LINK_TENSION_ONLY == lk.TENSION


def _random_links(n, seed):
    """links of every branch between the vertices 2 i and 2 i + 1 of a random cloud: ends 0.2 .. 3 H0 apart"""
    r = np.random.default_rng(seed)
    xa = (0.5 + 0.1 * r.normal(size=(n, 3))).astype(np.float32)
    dirs = r.normal(size=(n, 3))
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    dist = lk.H0 * r.uniform(0.2, 3.0, n)
    xb = (xa + dirs * dist[:, None]).astype(np.float32)
    x = np.empty((2 * n, 3), np.float32)
    x[0::2], x[1::2] = xa, xb
    v = (0.5 * r.normal(size=(2 * n, 3))).astype(np.float32)
    v[: n // 2] = 0.0                                             # a quarter of the links at rest
    branch = r.integers(0, 5, n)                                    # seam, spring, cord, cord, tension-only seam
    L = np.where((branch == 0) | (branch == 4), 0.0, dist * r.uniform(0.3, 1.7, n))   # stretched and compressed alike
    flags = np.where(branch >= 2, lk.TENSION, 0)
    rows = [(2 * i, 2 * i + 1, r.uniform(1, 100), L[i], r.uniform(0, 0.1) * (i % 3 != 0), flags[i]) for i in range(n)]
    return lk.make_links(rows), x, v


def test_host_function_against_float64():
    links, x, v = _random_links(3000, 1)
    f64, S, _, on = lk.link_forces64(links, x, v)
    spring = links["rest_length"] > 0
    tens = (links["flags"] & lk.TENSION) != 0
    for name, sel in (("seam", ~spring), ("spring", spring & ~tens), ("cord, taut", spring & tens & on),
                      ("cord, slack", spring & tens & ~on), ("tension-only seam", ~spring & tens)):
        assert sel.sum() > 50, (name, int(sel.sum()))
    worst = 0.0
    for i, q in enumerate(links):
        a, b = int(q["a"]), int(q["b"])
        fa = _force(q, x[a], x[b], v[a], v[b])
        fb = _force(q, x[b], x[a], v[b], v[a])
        # from b's side: the negative, bit for bit (a link that does not act gives +0 on both sides)
        assert np.isfinite(fa).all() and np.array_equal(fa, -fb), (i, fa, fb)
        nz = fa != 0
        assert np.array_equal(_bits(fa)[nz] ^ np.uint32(0x80000000), _bits(fb)[nz]), (i, fa, fb)
        if not on[i]:
            assert not fa.any(), (i, fa)
            continue
        err = np.abs(fa.astype(np.float64) - f64[i]).max()
        worst = max(worst, err / (lk.R_LINK * U * S[i]))
    print(f"mpm_link_force: {worst:.3g} of the per-link bound")
    assert worst <= 1.0, worst
    assert worst > 0.0


def test_seam_is_linear():
    """the seam law is k d + c w: exact under a scaling by a power of two, additive in (k, c) within the roundings, and
    blind to the direction"""
    r = np.random.default_rng(2)
    z = np.zeros(3, np.float32)
    for _ in range(200):
        d, w = (lk.H0 * r.normal(size=3)).astype(np.float32), r.normal(size=3).astype(np.float32)
        k, c = np.float32(r.uniform(1, 100)), np.float32(r.uniform(0, 0.1))
        q = lk.make_links([(0, 1, k, 0.0, c, 0)])[0]
        f = _force(q, z, d, z, w)
        assert np.array_equal(_bits(_force(q, z, 4 * d, z, 4 * w)), _bits(4 * f))
        assert np.array_equal(_bits(_force(q, z, 0.5 * d, z, 0.5 * w)), _bits(0.5 * f))
        fk = _force(lk.make_links([(0, 1, k, 0.0, 0.0, 0)])[0], z, d, z, w)
        fc = _force(lk.make_links([(0, 1, 0.0, 0.0, c, 0)])[0], z, d, z, w)
        assert np.array_equal(_bits(fk), _bits(k * d))               # one product, one rounding
        assert np.array_equal(_bits(fc), _bits(c * w))
        s = np.abs(k * d.astype(np.float64)) + np.abs(c * w.astype(np.float64))
        assert (np.abs(f.astype(np.float64) - (fk.astype(np.float64) + fc)) <= 2 * U * s).all()
        # a translation of both ends changes nothing but the rounding of the difference
        assert np.array_equal(_bits(_force(q, d, d + d, w, w + w)), _bits(f))


def test_tension_only_gate():
    """d = (3, 4, 0) H0: l2 and l = 5 H0 are exact floats"""
    h = np.float32(lk.H0)
    z, d, w = np.zeros(3, np.float32), np.array([3 * h, 4 * h, 0], np.float32), np.array([0.1, 0.2, -0.3], np.float32)
    l = np.float32(5 * h)
    below, above = np.nextafter(l, np.float32(0)), np.nextafter(l, np.float32(1))
    for L, acts in ((below, True), (l, False), (above, False)):
        cord = lk.make_links([(0, 1, 50.0, L, 0.05, lk.TENSION)])[0]
        spring = lk.make_links([(0, 1, 50.0, L, 0.05, 0)])[0]
        f, fs = _force(cord, z, d, z, w), _force(spring, z, d, z, w)
        assert fs.any()                                              # (the damping part acts whatever the length)
        if acts:
            assert np.array_equal(_bits(f), _bits(fs))               # a taut cord is the spring, to the bit
        else:
            assert not f.any(), (L, f)                               # elastic and damping part gated together
    # the restatement decides the same
    x = np.stack([z, d])
    for L, acts in ((below, True), (l, False), (above, False)):
        assert bool(lk.acts(lk.make_links([(0, 1, 50.0, L, 0.05, lk.TENSION)]), x)[0]) == acts
    # a tension-only seam acts wherever the ends differ, and not where they coincide
    seam = lk.make_links([(0, 1, 50.0, 0.0, 0.05, lk.TENSION)])[0]
    assert _force(seam, z, d, z, w).any() and not _force(seam, d, d, z, w).any()


def test_short_spring_gives_zero():
    z, w = np.zeros(3, np.float32), np.array([0.1, 0.2, -0.3], np.float32)
    spring = lk.make_links([(0, 1, 50.0, lk.H0, 0.05, 0)])[0]
    seam = lk.make_links([(0, 1, 50.0, 0.0, 0.05, 0)])[0]
    for d in (np.zeros(3, np.float32), np.array([5e-16, 0, 0], np.float32), np.array([3e-16, -4e-16, 5e-16], np.float32)):
        f = _force(spring, z, d, z, w)
        assert not f.any() and np.isfinite(f).all(), (d, f)          # |d|^2 < 1e-30: nothing, and nothing infinite
        want = 50.0 * d.astype(np.float64) + 0.05 * w.astype(np.float64)   # (the seam has no such floor)
        assert (np.abs(_force(seam, z, d, z, w) - want) <= 3 * U * np.abs(want)).all()
    d = np.array([2e-15, 0, 0], np.float32)                          # |d|^2 = 4e-30: the spring acts
    f = _force(spring, z, d, z, np.zeros(3, np.float32))
    assert f[0] < 0 and abs(f[0] / (50.0 * lk.H0) + 1.0) < 1e-6, f   # compressed to nothing: k L, pushing the ends apart


@pytest.mark.parametrize("name", list(lk.SCENES))
def test_restatement_is_the_gradient_of_its_energy(name):
    """-dE/dx by central differences in float64 (on states where no gate sits within the step), for the elastic part"""
    _, links, X = lk.scene(name)
    links = links.copy()
    links["damping"] = 0.0
    x, v = lk.state("random", name, X)
    F, _, _ = lk.vertex_forces64(links, x, np.zeros_like(x), len(X))
    on = lk.acts(links, x)

    def energy(xx):
        d = xx[links["b"]] - xx[links["a"]]
        l = np.sqrt((d * d).sum(axis=1))
        return float((0.5 * links["stiffness"].astype(np.float64) * (l - links["rest_length"]) ** 2 * on).sum())

    x64, h = x.astype(np.float64), 1e-7
    scale = float(np.abs(F).max())
    assert scale > 0
    r = np.random.default_rng(4)
    linked = np.unique(np.concatenate([links["a"], links["b"]]))
    for i in r.choice(linked, 40, replace=False):
        if i in lk.COINCIDENT and name == "mixed":
            continue                                                 # (|d| = 0: the spring's energy has a kink there)
        for j in range(3):
            xp, xm = x64.copy(), x64.copy()
            xp[i, j] += h
            xm[i, j] -= h
            g = -(energy(xp) - energy(xm)) / (2 * h)
            assert abs(g - F[i, j]) <= 1e-6 * scale, (i, j, g, F[i, j])
    e, bound, l = lk.energy64(links, x)
    assert abs(e - energy(x64)) <= bound + 1e-15 * abs(e)


def test_scenes_cover_the_layouts():
    """what the GPU tests rely on: more than 64 linked rows with a partial last slice, a hub wider than two batches, a
    link inside one cloth, a duplicate pair, every link mix in the rest state"""
    cloths, links, X = lk.scene("mixed")
    rows = np.unique(np.concatenate([links["a"], links["b"]]))
    assert len(rows) > 128 and len(rows) % 64 != 0
    n = np.bincount(np.concatenate([links["a"], links["b"]]), minlength=len(X))
    assert n.max() > 16 and n[0] == n.max()
    nv = len(cloths[0][0])
    assert ((links["a"] < nv) & (links["b"] < nv)).any()
    pairs = [tuple(sorted((int(q["a"]), int(q["b"])))) for q in links]
    assert len(set(pairs)) < len(pairs)
    x, v = lk.state("rest", "mixed", X)
    f, S, l, on = lk.link_forces64(links, x, v)
    L, tens = links["rest_length"], (links["flags"] & lk.TENSION) != 0
    assert ((L == 0) & ~tens).any() and ((L > 0) & ~tens & (l > L)).any() and ((L > 0) & ~tens & (l < L) & (l > 0)).any()
    assert (tens & (l < L)).any() and (tens & (l > L) & (L > 0)).any() and (tens & (l == L) & ~on).any()
    assert ((L > 0) & (l == 0) & ~on).any()
    cloths, links, X = lk.scene("seam")
    assert len(links) == 24 and all(len(Xc) == 24 * 24 for Xc, _ in cloths)
    assert np.allclose(lk.link_forces64(links, X, np.zeros_like(X))[2], lk.SEAM_GAP)
