"""Tearing cloth (mpm_set_tearing) without a GPU: the library's host entry point mpm_tear_face (no handle, no device) against
tests/tearing.py's float32 restatement to the bit and against its float64 values within the rounding bound, the verdicts
on every decided face, their invariance under exact rigid motions, the rounding of L and the refusal of bad limits by the table builder, the cap
on undecided faces per scene and state, and a stand-alone host program built with the address and undefined-behaviour
sanitizers from mpm_tear.h.  The rest records of a scene are tests/damping.py's rest_records."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import tearing as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "drake_amd", "csrc")
U = tr.U
_CACHE = {}


def _scene(name):
    if name not in _CACHE:
        s = dict(tr.scene(name))
        s["dm"] = tr.rest_records(s["X"], s["T"])[0]
        _CACHE[name] = s
    return _CACHE[name]


def _xc(s, st):
    return tr.corners(s["T"], tr.state(st, s))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_library_exports_the_tearing_entry_points():
    from drake_amd import capi
    lib = capi.load_library()
    names = ("mpm_set_tearing", "mpm_get_tearing", "mpm_set_torn_faces", "mpm_tear_state", "mpm_tear_measure", "mpm_tear_face")
    for name in names:
        assert hasattr(lib, name), name
        assert name in capi.SYMBOLS
    for name in ("set_tearing", "get_tearing", "set_torn_faces", "tear_state", "tear_measure"):
        assert hasattr(capi.GpuMpm, name), name
    text = open(os.path.join(ROOT, "include", "gpu_mpm.hpp")).read()
    for name in ("SetTearing", "SetTornFaces", "TearState", "TearMeasure"):
        assert name in text, name


@pytest.mark.parametrize("name", list(tr.SCENES))
def test_undecided_faces_stay_under_the_cap(name):
    """from float64 alone: in every state at most 5 % of the scene's faces are undecided, the sweeps have faces on both
    sides of the limit, and the rest state fails nowhere"""
    s = _scene(name)
    for st in tr.STATES:
        fails, decided = tr.verdict64(s["dm"], _xc(s, st), s["L_f"])
        share = 1.0 - decided.mean()
        print(f"tearing {name} {st}: {int((~decided).sum())} of {len(decided)} faces undecided, {int(fails.sum())} fail")
        assert share <= tr.CAP, (name, st, share)
        tears = s["L_f"] > 0
        if st.startswith("rest"):
            assert not fails.any()
        else:
            assert fails[tears].any() and not fails[tears].all(), (name, st)
        assert not fails[~tears].any()


@pytest.mark.parametrize("name", list(tr.SCENES))
def test_host_function_bits_bound_and_verdicts(name):
    """mpm_tear_face: m, q and the verdict are tear_face32's bits; m and q lie within the
    first-order bounds d_m, d_q of float64 (tests/tearing.py's errors64); the verdict is float64's on every decided face"""
    from drake_amd import tear_face
    s = _scene(name)
    L = np.where(s["L_f"] > 0, s["L_f"], tr.limit_squared(tr.LIMIT)).astype(np.float32)   # (the formula on every face)
    worst = [0.0, 0.0]
    for st in tr.STATES:
        xc = _xc(s, st)
        mq, fails = tear_face(s["dm"], xc, L)
        mq32, fails32 = tr.tear_face32(s["dm"], xc, L)
        assert np.array_equal(_bits(mq), _bits(mq32)) and np.array_equal(fails, fails32), (name, st)
        m, q, _ = tr.values64(s["dm"], xc)
        d_m, d_q, _, _ = tr.errors64(s["dm"], xc, L)
        wm = float((np.abs(mq[:, 0] - m) / (tr.UB * d_m)).max())
        wq = float((np.abs(mq[:, 1] - q) / np.maximum(tr.UB * d_q, 1e-300)).max())
        worst = [max(worst[0], wm), max(worst[1], wq)]
        assert wm <= 1.0 and wq <= 1.0, (name, st, wm, wq)
        ref, decided = tr.verdict64(s["dm"], xc, L)
        assert np.array_equal(fails[decided], ref[decided]), (name, st, int((fails != ref)[decided].sum()))
    print(f"tearing host function, {name}: m {worst[0]:.3g}, q {worst[1]:.3g} of the bound")


@pytest.mark.parametrize("name", list(tr.SCENES))
def test_verdict_is_invariant_under_exact_rigid_motions(name):
    """a quarter turn about z, (x, y, z) -> (-y, x, z), and a shift by -1/4 along every axis are exact in float32 at the
    scenes' positions (0.4 .. 0.6): float64's lambda1 is unchanged, the float chains run in another order; the verdict
    on decided faces is the same"""
    from drake_amd import tear_face
    s = _scene(name)
    L = tr.limit_squared(tr.LIMIT)
    for st in tr.STATES:
        x = tr.state(st, s)
        turned = np.stack([-x[:, 1], x[:, 0], x[:, 2]], 1)
        shifted = x - np.float32(0.25)
        assert np.array_equal(shifted.astype(np.float64), x.astype(np.float64) - 0.25)
        ref, decided = tr.verdict64(s["dm"], tr.corners(s["T"], x), L)
        base = tear_face(s["dm"], tr.corners(s["T"], x), L)[1]
        for y in (turned, shifted):
            ref_y, decided_y = tr.verdict64(s["dm"], tr.corners(s["T"], y), L)
            both = decided & decided_y
            assert np.array_equal(ref[both], ref_y[both])
            got = tear_face(s["dm"], tr.corners(s["T"], y), L)[1]
            assert np.array_equal(got[both], base[both]), (name, st)


# ---- the stand-alone host program ------------------------------------------------------------------------------------------
FLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#include "mpm_tear.h"
// in: n_cloths, then per cloth: first face, face count, the limit as a hex word; then n_faces, then per face 3 dminv and
// 9 corner words
// out: one line "T <ok> <L words ...>", one line of the cloth of every face, one of the ranges; then per face
// "<fails> <m word> <q word>" against its cloth's L
static float rd(FILE* f) { unsigned u = 0; if (fscanf(f, "%x", &u) != 1) u = 0; float x; memcpy(&x, &u, 4); return x; }
static unsigned wd(float x) { unsigned u; memcpy(&u, &x, 4); return u; }
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    int nc = 0, nf = 0;
    if (fscanf(f, "%d", &nc) != 1 || nc < 0) return 2;
    std::vector<size_t> first(nc), count(nc);
    std::vector<float> limit(nc), L(nc);
    for (int c = 0; c < nc; ++c) {
        unsigned long a = 0, b = 0;
        if (fscanf(f, "%lu %lu", &a, &b) != 2) return 2;
        first[c] = a; count[c] = b; limit[c] = rd(f);
    }
    if (fscanf(f, "%d", &nf) != 1 || nf < 0) return 2;
    std::vector<int> cloth(nf, -1), ranges(2 * nc, -1);
    const bool ok = mpm::tear_tables((size_t)nc, first.data(), count.data(), limit.data(), (size_t)nf, L.data(), cloth.data(), ranges.data());
    printf("T %d", ok ? 1 : 0);
    for (int c = 0; c < nc; ++c) printf(" %08x", wd(L[c]));
    printf("\n");
    for (int i = 0; i < nf; ++i) printf("%d ", cloth[i]);
    printf("\n");
    for (int c = 0; c < 2 * nc; ++c) printf("%d ", ranges[c]);
    printf("\n");
    std::vector<float> row(12);
    for (int i = 0; i < nf; ++i) {
        for (float& x : row) x = rd(f);
        float x[3][3], mq[2];
        memcpy(x, &row[3], 36);
        const float Lf = ok && cloth[i] >= 0 ? L[cloth[i]] : 0.f;
        const bool fails = mpm::tear_face(row[0], row[1], row[2], Lf, x, mq);
        printf("%d %08x %08x\n", fails ? 1 : 0, wd(mq[0]), wd(mq[1]));
    }
    fclose(f);
    return 0;
}
"""


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cc = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cc is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("tear_host")
    src, exe = str(d / "tear.cc"), str(d / "tear")
    open(src, "w").write(PROGRAM)
    subprocess.check_call([cc, *FLAGS, "-I", CSRC, src, "-o", exe])
    return exe, d


def _run(program, tag, cloths, dm, xc):
    exe, d = program
    path = str(d / f"{tag}.txt")
    rows = np.concatenate([dm, xc.reshape(-1, 9)], axis=1).astype(np.float32)
    with open(path, "w") as f:
        f.write(f"{len(cloths)}\n")
        for first, count, lim in cloths:
            f.write(f"{first} {count} {int(np.float32(lim).view(np.uint32)):08x}\n")
        f.write(f"{len(rows)}\n")
        for r in rows.view(np.uint32):
            f.write(" ".join(f"{w:08x}" for w in r) + "\n")
    # (a sanitizer report ends the program with a non-zero status: check_output raises)
    return subprocess.check_output([exe, path]).decode().split("\n")


@pytest.mark.parametrize("name,st", [("quad12", "uniaxial"), ("hub", "shear_rot"), ("pair", "random"), ("sliver", "uniaxial_rot")])
def test_standalone_program_reproduces_tables_and_verdicts(program, name, st):
    """mpm_tear.h in a host program of its own, under the address and undefined-behaviour sanitizers: the table builder's
    L, cloth of face and ranges, and the library's m, q and verdicts, word for word"""
    from drake_amd import tear_face
    s = _scene(name)
    xc = _xc(s, st)
    nfc = np.bincount(s["cof"], minlength=len(s["limits"]))
    firsts = np.concatenate([[0], np.cumsum(nfc)[:-1]])
    out = _run(program, f"{name}_{st}", list(zip(firsts, nfc, s["limits"])), s["dm"], xc)
    head = out[0].split()
    assert head[:2] == ["T", "1"]
    assert np.array_equal(np.array([int(w, 16) for w in head[2:]], np.uint32), _bits(tr.limit_squared(s["limits"])))
    assert np.array_equal(np.array(out[1].split(), int), s["cof"])
    assert np.array_equal(np.array(out[2].split(), int).reshape(-1, 2), np.stack([firsts, firsts + nfc], 1))
    got = [ln.split() for ln in out[3:] if ln]
    mq, fails = tear_face(s["dm"], xc, s["L_f"])
    assert len(got) == len(xc)
    assert np.array_equal(np.array([[int(w, 16) for w in g[1:]] for g in got], np.uint32), _bits(mq))
    assert np.array_equal(np.array([g[0] == "1" for g in got]), fails)


@pytest.mark.parametrize("bad", [1.0, 0.5, -1.2, np.nan, np.inf, -0.0 + 1e-30, 3e19])
def test_table_builder_refuses_bad_limits(program, bad):
    """a limit that is neither 0 nor a finite number > 1 with a finite float square: tear_tables says no (the engine's
    refusal of the same values is tests/test_tearing_gpu.py's)"""
    s = _scene("hub")
    out = _run(program, "bad", [(0, len(s["T"]), bad)], s["dm"], _xc(s, "rest"))
    assert out[0].split()[:2] == ["T", "0"]


def test_limit_rounding_of_the_table_builder(program):
    """tear_limit through the stand-alone program, 4000 random limits as 4000 cloths without faces: L is the float
    nearest to the exact square of the float limit (the square of a float is exact in double, so one rounding), the
    words of tests/tearing.py's limit_squared and of the binding's tear_limit_squared; 0 stays 0"""
    from drake_amd import tear_limit_squared
    lim = np.random.default_rng(5).uniform(1.0001, 3.0, 4000).astype(np.float32)
    lim[::500] = 0.0
    out = _run(program, "limits", [(0, 0, x) for x in lim], np.zeros((0, 3), np.float32), np.zeros((0, 3, 3), np.float32))
    head = out[0].split()
    assert head[:2] == ["T", "1"]
    L = np.array([int(w, 16) for w in head[2:]], np.uint32).view(np.float32)
    assert np.array_equal(_bits(L), _bits(tr.limit_squared(lim))) and np.array_equal(_bits(L), _bits(tear_limit_squared(lim)))
    exact = lim.astype(np.float64) ** 2
    assert np.all(np.abs(L.astype(np.float64) - exact) <= 0.5 * np.spacing(L).astype(np.float64))
    assert not L[::500].any() and np.all(L[lim > 0] > 1.0)
