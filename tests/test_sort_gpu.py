"""The device radix sort (drake_amd/csrc/mpm_sort.h) through mpm_debug_sort_pairs against np.argsort(kind="stable"):
every digit width (8 - 11 bits), pass count (1 - 4), both tile sizes and both result locations the cost model picks on
the grid of tests/resort_reference.py (SORT_N x SORT_BITS; tests/test_resort_reference.py shows on the CPU that the
grid reaches them all), seven key distributions, the contact sort's sentinel keys, and device-side counts below the
launch bound.  Integer code: every comparison is exact."""
import numpy as np
import pytest

from tests import resort_reference as rr

pytestmark = pytest.mark.gpu

# byte patterns mpm_debug_sort_pairs fills the buffers with before the upload (include/mpm_hip.h)
FILL = dict(ka=0xA5A5A5A5, va=0x5A5A5A5A, kb=0xB6B6B6B6, vb=0x6B6B6B6B)


@pytest.fixture(scope="module")
def eng():
    from drake_amd import GpuMpm
    g = GpuMpm(4)
    yield g
    g.destroy()


def _expect(keys, bits):
    order = np.argsort(keys & np.uint32((1 << bits) - 1) if bits < 32 else keys, kind="stable")
    return keys[order], order.astype(np.uint32)


def _check_info(info, n, bits):
    pl = rr.sort_plan(n, bits)
    assert (info["digit_bits"], info["passes"], info["tiles"]) == (pl["digit_bits"], pl["passes"], pl["tiles"]), (n, bits, info, pl)
    return pl


def _sorted_pair(eng, keys, bits, in_place, what):
    """runs one sort; -> (keys, vals) of the pair that holds the result, checked to be where it was asked for"""
    n = len(keys)
    ko, vo, info = eng.debug_sort_pairs(keys, np.arange(n, dtype=np.uint32), bits, want_in_place=in_place)
    pl = _check_info(info, n, bits)
    if in_place:
        assert not info["in_b"], what
        where = 0
    else:
        assert info["in_b"] == pl["in_b"], (what, info, pl)
        where = 1 if info["in_b"] else 0
    return ko[where], vo[where], info


@pytest.mark.parametrize("n", rr.SORT_N)
def test_sort_matches_a_stable_sort(eng, n):
    dists = rr.SORT_DISTS if n < rr.SORT_LARGE else rr.SORT_DISTS_LARGE
    for bits in rr.SORT_BITS:
        for dist in dists:
            keys = rr.sort_keys(dist, n, bits)
            want_k, want_v = _expect(keys, bits)
            for in_place in (True, False):
                what = f"n {n}, {bits} bits, {dist}, {'in place' if in_place else 'either buffer'}"
                got_k, got_v, info = _sorted_pair(eng, keys, bits, in_place, what)
                bad = np.flatnonzero((got_k != want_k) | (got_v != want_v))
                assert bad.size == 0, (f"{what} ({info}): {bad.size} pairs differ from the stable sort, first at {bad[0]}: "
                                       f"({got_k[bad[0]]:#x}, {got_v[bad[0]]}) instead of ({want_k[bad[0]]:#x}, {want_v[bad[0]]})")


def test_grid_reaches_every_path(eng):
    """what info_out reports over the grid: every digit width, pass count, tile size and result location"""
    seen = dict(digit_bits=set(), passes=set(), items=set(), in_b=set())
    for n in rr.SORT_N:
        for bits in rr.SORT_BITS:
            _, _, info = eng.debug_sort_pairs(np.zeros(n, np.uint32), np.arange(n, dtype=np.uint32), bits, want_in_place=False)
            _check_info(info, n, bits)
            seen["digit_bits"].add(info["digit_bits"])
            seen["passes"].add(info["passes"])
            seen["items"].add(-(-n // (64 * info["tiles"])) > 16)     # more than 16 chunks per tile: the large tile
            seen["in_b"].add(info["in_b"])
    assert seen["digit_bits"] == {8, 9, 10, 11} and seen["passes"] == {1, 2, 3, 4}, ("move the grid with the cost model", seen)
    assert seen["items"] == {False, True} and seen["in_b"] == {False, True}, seen


@pytest.mark.parametrize("bits", (19, 22, 31))
@pytest.mark.parametrize("n", (4097, 2 ** 18 + 1))
def test_sentinel_keys_go_last_in_input_order(eng, n, bits):
    """the contact sort: a random third of the keys is 0xFFFFFFFF (pairs to drop), the others are below the mask"""
    rng = np.random.default_rng([n, bits])
    keys = rng.integers(0, (1 << bits) - 1, n, dtype=np.uint64).astype(np.uint32)
    drop = rng.random(n) < 1.0 / 3.0
    keys[drop] = 0xFFFFFFFF
    real = np.flatnonzero(~drop)
    want_v = np.concatenate([real[np.argsort(keys[real], kind="stable")], np.flatnonzero(drop)]).astype(np.uint32)
    for in_place in (True, False):
        got_k, got_v, info = _sorted_pair(eng, keys, bits, in_place, f"sentinels, n {n}, {bits} bits")
        assert np.array_equal(got_v, want_v), (n, bits, in_place, info)
        assert np.array_equal(got_k, keys[want_v])


@pytest.mark.parametrize("bits", (9, 22))
@pytest.mark.parametrize("n", (4097, 2 ** 18 + 4097))
def test_device_count_below_the_launch_bound(eng, n, bits):
    """the count comes from device memory: the first `count` outputs are the stable sort of the first `count` inputs, and
    nothing at or beyond `count` is written in either buffer pair"""
    keys = rr.sort_keys("uniform", n, bits, seed=3)
    vals = np.arange(n, dtype=np.uint32)
    for count in (0, 1, 63, n // 2, n - 1, n):
        want_k, want_v = _expect(keys[:count], bits)
        for in_place in (True, False):
            what = f"n {n}, {bits} bits, device count {count}, {'in place' if in_place else 'either buffer'}"
            ko, vo, info = eng.debug_sort_pairs(keys, vals, bits, device_count=count, want_in_place=in_place)
            pl = _check_info(info, n, bits)
            assert info["in_b"] == (pl["in_b"] and not in_place), what
            w = 1 if info["in_b"] else 0
            assert np.array_equal(ko[w][:count], want_k) and np.array_equal(vo[w][:count], want_v), what
            # the tails: pair b keeps its fill; pair a keeps its own, or -- in place after an odd number of passes --
            # holds the copy of pair b's, which radix_sort_pairs makes over the whole launch bound
            copied = in_place and pl["in_b"]
            for name, arr, fill in (("keys a", ko[0], FILL["kb"] if copied else FILL["ka"]),
                                    ("values a", vo[0], FILL["vb"] if copied else FILL["va"]),
                                    ("keys b", ko[1], FILL["kb"]), ("values b", vo[1], FILL["vb"])):
                bad = np.flatnonzero(arr[count:] != fill)
                assert bad.size == 0, (f"{what}: {name} written at index {count + bad[0]} >= the device count "
                                       f"({arr[count + bad[0]]:#x}, fill {fill:#x}; {bad.size} entries)")
