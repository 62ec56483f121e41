"""Creases (mpm_set_creases) without a GPU: the library's host entry point mpm_crease_hinge (no handle, no device) against
tests/creases.py's float32 restatement to the bit and against its float64 values within the counted bounds, the
verdicts on every decided hinge, psi bit-equal to mpm_shell_hinge's, the invariants of the return mapping, the cases'
own conditions (the cap on undecided hinges, hinges on both sides of the yield), the refusals of the host function, and
a stand-alone host program built with the address and undefined-behaviour sanitizers from mpm_shell.h."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import creases as cr
from tests import shell_bending as sb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "drake_amd", "csrc")
U, F = cr.U, np.float32


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _x4(x32, H):
    return np.asarray(x32, F)[H].reshape(-1, 4, 3)


def test_library_exports_the_crease_entry_points():
    from drake_amd import capi
    lib = capi.load_library()
    names = ("mpm_set_creases", "mpm_get_creases", "mpm_set_crease_state", "mpm_crease_state", "mpm_crease_measure", "mpm_crease_hinge")
    for name in names:
        assert hasattr(lib, name), name
        assert name in capi.SYMBOLS
    for name in ("set_creases", "get_creases", "set_crease_state", "crease_state", "crease_measure", "crease_hinge"):
        assert hasattr(capi.GpuMpm, name), name
    text = open(os.path.join(ROOT, "include", "gpu_mpm.hpp")).read()
    for name in ("SetCreases", "GetCreases", "SetCreaseState", "CreaseState", "CreaseMeasure"):
        assert name in text, name
    text = open(os.path.join(ROOT, "include", "mpm_hip.h")).read()
    for name in names + ("mpm_cloth_crease_t",):
        assert name in text, name


def test_y_and_P_are_rounded_once():
    """chord = float(2 sin(angle / 2)) of the float angle: the binding's and the model's are the same words, within
    half a unit in the last place of the exact value; pi gives exactly 2"""
    from drake_amd import crease_chord
    a = np.random.default_rng(1).uniform(1e-6, np.pi, 2000).astype(F)
    y = crease_chord(a)
    assert np.array_equal(_bits(y), _bits(cr.chord(a)))
    exact = 2.0 * np.sin(0.5 * a.astype(np.float64))
    assert np.all(np.abs(y.astype(np.float64) - exact) <= 0.5 * np.spacing(y).astype(np.float64) * 1.0000001)
    assert crease_chord(np.pi) == F(2) and crease_chord(0.0) == F(0)


@pytest.mark.parametrize("angle", cr.YIELD_ANGLES)
@pytest.mark.parametrize("name,st", cr.CASES)
def test_cases_hold_their_own_conditions(name, st, angle):
    """from float64 alone: at most 2 % of a case's active hinges are undecided; a state that bends the mesh holds a
    decided yielding and a decided holding hinge (every `perturbed` case; the strip's one hinge cannot hold both); the
    rest, rigid and affine-of-flat states yield nowhere"""
    x, H, psibar = cr.case(name, st)
    if len(H) == 0:
        return
    act = sb.active(x, H)
    y = cr.chord(angle)
    yields, decided = cr.verdict64(x, H, psibar, y, act)
    t = cr.values64(x, H, psibar)[2]
    n_act = max(int(act.sum()), 1)
    print(f"creases {name} {st} at {angle}: {int(yields.sum())} of {len(H)} yield, {int((~decided).sum())} undecided, max t {np.nanmax(t):.3g}")
    assert (~decided).sum() <= cr.CAP * n_act, (name, st, int((~decided).sum()))
    if st == "perturbed" and len(H) > 1:
        assert (~decided).sum() == 0
        assert (yields & decided).any() and (~yields & decided & act).any(), (name, st)
    flat = sb.mesh(name)[2] is None and name in ("strip", "fan", "jittered")
    if st in ("rest", "rigid") or (st == "affine" and flat):
        assert np.nanmax(t) <= 3.2e-5 and not yields.any(), (name, st, float(np.nanmax(t)))
    if st == "collinear":
        assert not act.any() and not yields.any()


@pytest.mark.parametrize("angle", cr.YIELD_ANGLES)
@pytest.mark.parametrize("name,st", cr.CASES)
def test_host_function_bits_bound_and_verdicts(name, st, angle):
    """mpm_crease_hinge: psi, dpsi, psibar' and the verdict are the float32 restatement's bits; psi is mpm_shell_hinge's
    bits and so is the gate; t lies within R_T W 2^-24 of float64, psibar' within R_PB W / dpsi 2^-24; the verdict is
    float64's on every decided hinge; with eta = 0 and 0.5 alike"""
    from drake_amd import crease_hinge, shell_hinge
    x, H, psibar = cr.case(name, st)
    if len(H) == 0:
        return
    act = sb.active(x, H)
    y = cr.chord(angle)
    psi32, dpsi32, on32 = cr.angle32(x, H)
    assert np.array_equal(on32, act)
    for h in range(len(H)):
        _, psi_h, on_h = shell_hinge(_x4(x, H)[h], 1.0, psibar[h])
        assert _bits(psi_h)[0] == _bits(psi32[h])[0] and on_h == bool(act[h]), (name, st, h)
    # (psi itself against float64, within the bound mpm_shell.h counts for it)
    psi64, _, _, _ = cr.values64(x, H, psibar)
    kA, kB = sb.kappas(x.astype(np.float64), H)
    assert np.all(np.abs(psi32.astype(np.float64) - psi64)[act] <= (sb.R_PSI * U * (kA + kB) * (1.0 + np.abs(psi64)))[act])
    worst = [0.0, 0.0]
    for eta, P in ((0.0, 2.0), (0.5, 2.0), (0.5, float(cr.chord(1.0)))):
        P = max(P, float(np.abs(psibar).max()))
        psi, dpsi, nxt, yields = crease_hinge(_x4(x, H), psibar, y, eta, P)
        nxt32, yields32, t32 = cr.return32(psi32, dpsi32, on32, psibar, y, eta, P)
        assert np.array_equal(_bits(psi), _bits(psi32)) and np.array_equal(_bits(dpsi), _bits(dpsi32)), (name, st)
        assert np.array_equal(_bits(nxt), _bits(nxt32)) and np.array_equal(yields, yields32), (name, st)
        ref, decided = cr.verdict64(x, H, psibar, y, act)
        assert np.array_equal(yields[decided], ref[decided]), (name, st, int((yields != ref)[decided].sum()))
        _, _, t64, W = cr.values64(x, H, psibar)
        wt = float(np.max(np.where(act, np.abs(t32.astype(np.float64) - t64) / (cr.R_T * U * W), 0.0)))
        want, bound = cr.return64(x, H, psibar, y, eta, P, act)
        both = decided & (yields == ref)
        err = np.abs(nxt.astype(np.float64) - want)[both]
        assert np.all(err[~ref[both]] == 0)
        wp = float(np.max(np.where(ref[both], err / np.maximum(bound[both], 1e-300), 0.0))) if both.any() else 0.0
        worst = [max(worst[0], wt), max(worst[1], wp)]
        assert wt <= 1.0 and wp <= 1.0, (name, st, eta, wt, wp)
        # the invariants: psibar' lies between psibar and psi and within [-P, P]; what does not yield is unchanged
        lo, hi = np.minimum(psibar, psi), np.maximum(psibar, psi)
        assert np.all((nxt >= lo) & (nxt <= hi))
        assert np.all(np.abs(nxt) <= F(P))
        assert np.array_equal(_bits(nxt[~yields]), _bits(psibar[~yields])) and not yields[~act].any()
        if eta == 0.0:   # ... and with eta = 0 the moment left is the yield moment, within t's bound
            left = np.abs(psi.astype(np.float64) - nxt.astype(np.float64)) * dpsi.astype(np.float64)
            assert np.all(left[yields] <= float(y) + cr.R_T * U * W[yields]), (name, st)
    print(f"creases host function, {name} {st} at {angle}: t {worst[0]:.3g}, psibar' {worst[1]:.3g} of the bound")


def test_theta_sweep_of_the_strip_across_the_threshold():
    """the strip's one hinge from theta = -3.1 to 3.1, flat rest: it yields beyond the yield angle in both signs and
    holds below it; at theta = +-3.1, where |psi - psibar| is about 2, t is 0.0416 and the hinge does NOT yield at 0.05"""
    from drake_amd import crease_hinge
    H = sb.hinges(sb.mesh("strip")[1])
    for angle in cr.YIELD_ANGLES:
        y = cr.chord(angle)
        for theta in cr.SWEEP:
            x = cr.sweep_state(theta)
            act = sb.active(x, H)
            ref, decided = cr.verdict64(x, H, np.zeros(1, F), y, act)
            psi, dpsi, nxt, yields = crease_hinge(_x4(x, H), 0.0, y, 0.0, 2.0)
            assert decided[0], (angle, theta)
            assert yields[0] == ref[0], (angle, theta)
            # |psi| cos(theta / 2) = |sin theta| against 2 sin(angle / 2)
            assert ref[0] == (abs(np.sin(theta)) > float(y)), (angle, theta)
            if yields[0]:
                want, bound = cr.return64(x, H, np.zeros(1, F), y, 0.0, 2.0, act)
                assert abs(float(nxt[0]) - want[0]) <= bound[0]
                assert np.sign(nxt[0]) == np.sign(theta)
        x = cr.sweep_state(3.1)
        psi, dpsi, nxt, yields = crease_hinge(_x4(x, H), 0.0, cr.chord(0.05), 0.0, 2.0)
        assert abs(float(psi[0]) * float(dpsi[0]) - 0.0416) < 1e-4 and abs(float(psi[0])) > 1.99 and not yields[0]


def test_clamp_nan_and_inactive_hinges():
    """the clamp holds psibar' at +-P; NaN positions, a NaN psibar and an inactive hinge change nothing"""
    from drake_amd import crease_hinge
    H = sb.hinges(sb.mesh("strip")[1])
    x = cr.sweep_state(1.2)
    P = cr.chord(0.5)
    for sign in (1.0, -1.0):
        psi, dpsi, nxt, yields = crease_hinge(_x4(cr.sweep_state(sign * 1.2), H), 0.0, cr.chord(0.05), 0.0, P)
        assert yields[0] and _bits(nxt)[0] == _bits(F(sign) * P)
    bad = x.copy()
    bad[3, 1] = np.nan
    psi, dpsi, nxt, yields = crease_hinge(_x4(bad, H), 0.25, cr.chord(0.05), 0.5, 2.0)
    assert not yields[0] and _bits(nxt)[0] == _bits(F(0.25))
    psi, dpsi, nxt, yields = crease_hinge(_x4(x, H), np.nan, cr.chord(0.05), 0.5, 2.0)
    assert not yields[0] and np.isnan(nxt[0])
    col = sb.state("strip", "collinear")
    psi, dpsi, nxt, yields = crease_hinge(_x4(col, H), 0.25, cr.chord(0.05), 0.0, 2.0)
    assert not yields[0] and _bits(nxt)[0] == _bits(F(0.25)) and psi[0] == 0 and dpsi[0] == 0
    # y = 0: elastic, whatever the state
    psi, dpsi, nxt, yields = crease_hinge(_x4(x, H), 0.0, 0.0, 0.0, 2.0)
    assert not yields[0] and nxt[0] == 0


@pytest.mark.parametrize("n_faces", cr.STRIPS)
def test_layout_strips_hold_both_verdicts(n_faces):
    """the layout scenes of the GPU tests: n_faces - 1 hinges, at both yield angles hinges on both sides and at most 2 %
    undecided"""
    X, T, x = cr.strip(n_faces)
    H = sb.hinges(T)
    assert len(H) == n_faces - 1
    act = sb.active(x, H)
    assert act.all()
    for angle in cr.YIELD_ANGLES:
        yields, decided = cr.verdict64(x, H, np.zeros(len(H), F), cr.chord(angle), act)
        assert (~decided).sum() <= cr.CAP * len(H)
        assert (yields & decided).any() and (~yields & decided).any(), (n_faces, angle)


def test_host_function_refuses_null_arguments():
    from drake_amd import capi
    lib = capi.load_library()
    a = np.zeros(12, F)
    s = np.zeros(1, F)
    args = [a.ctypes.data, s.ctypes.data, s.ctypes.data, s.ctypes.data, s.ctypes.data]
    for k in range(5):
        bad = list(args)
        bad[k] = None
        assert lib.mpm_crease_hinge(1, *bad, None, None, None, None) == -1 and "null" in lib.mpm_last_error().decode()
    assert lib.mpm_crease_hinge(1, *args, None, None, None, None) == 0      # (every output may be NULL)
    assert lib.mpm_crease_hinge(0, None, None, None, None, None, None, None, None, None) == 0


# ---- the stand-alone host program ------------------------------------------------------------------------------------------
FLAGS = ["-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
PROGRAM = r"""
#include <cstdio>
#include <cstring>
#include <vector>
#include "mpm_shell.h"
// in: n_cloths, then per cloth the three words yield_angle, hardening, max_angle; then n, then per hinge 12 position
// words, psibar and the hinge's cloth
// out: one line "C <ok> <y eta P words per cloth ...>"; then per hinge "<on> <yields> <psi> <dpsi> <psibar'>" as words
static float rd(FILE* f) { unsigned u = 0; if (fscanf(f, "%x", &u) != 1) u = 0; float x; memcpy(&x, &u, 4); return x; }
static unsigned wd(float x) { unsigned u; memcpy(&u, &x, 4); return u; }
int main(int argc, char** argv) {
    if (argc < 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    int nc = 0, n = 0;
    if (fscanf(f, "%d", &nc) != 1 || nc < 0) return 2;
    std::vector<mpm::ClothCrease> t(nc);
    for (int c = 0; c < nc; ++c) {
        t[c].yield_angle = rd(f); t[c].hardening = rd(f); t[c].max_angle = rd(f); t[c].reserved = 0.f;
    }
    std::vector<float> yep(3 * (nc > 0 ? nc : 1), 0.f);
    const std::string why = mpm::crease_params(t.data(), (size_t)nc, yep.data());
    printf("C %d", why.empty() ? 1 : 0);
    for (int c = 0; c < 3 * nc; ++c) printf(" %08x", wd(yep[c]));
    printf("\n");
    if (fscanf(f, "%d", &n) != 1 || n < 0) return 2;
    for (int i = 0; i < n; ++i) {
        float x[12];
        for (float& v : x) v = rd(f);
        const float psibar = rd(f);
        int c = 0;
        if (fscanf(f, "%d", &c) != 1 || c < 0 || c >= nc) return 2;
        float psi, dpsi;
        bool yields;
        const bool on = mpm::shell_angle(x, x + 3, x + 6, x + 9, &psi, &dpsi);
        const float next = mpm::crease_return(psi, dpsi, on, psibar, yep[3 * c], yep[3 * c + 1], yep[3 * c + 2], &yields);
        printf("%d %d %08x %08x %08x\n", on ? 1 : 0, yields ? 1 : 0, wd(psi), wd(dpsi), wd(next));
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
    d = tmp_path_factory.mktemp("crease_host")
    src, exe = str(d / "crease.cc"), str(d / "crease")
    open(src, "w").write(PROGRAM)
    subprocess.check_call([cc, *FLAGS, "-I", CSRC, src, "-o", exe])
    return exe, d


def _run(program, tag, rows, x4, psibar, cloth):
    exe, d = program
    path = str(d / f"{tag}.txt")
    with open(path, "w") as f:
        f.write(f"{len(rows)}\n")
        for r in np.asarray(rows, F).reshape(-1, 3):
            f.write(" ".join(f"{w:08x}" for w in r.view(np.uint32)) + "\n")
        f.write(f"{len(x4)}\n")
        words = np.concatenate([np.asarray(x4, F).reshape(-1, 12), np.asarray(psibar, F).reshape(-1, 1)], axis=1).view(np.uint32)
        for r, c in zip(words, cloth):
            f.write(" ".join(f"{w:08x}" for w in r) + f" {int(c)}\n")
    # (a sanitizer report ends the program with a non-zero status: check_output raises)
    return subprocess.check_output([exe, path]).decode().split("\n")


@pytest.mark.parametrize("name,st", [("icosphere2", "perturbed"), ("book", "perturbed"), ("jittered", "affine"),
                                     ("strip", "folded+"), ("strip", "collinear")])
def test_standalone_program_reproduces_parameters_and_returns(program, name, st):
    """mpm_shell.h in a host program of its own, under the address and undefined-behaviour sanitizers: y, eta, P of three
    cloths and psi, dpsi, psibar' and the verdicts of the library, word for word"""
    from drake_amd import crease_hinge
    x, H, psibar = cr.case(name, st)
    rows = [(0.05, 0.0, 0.0), (0.0, 0.0, 0.0), (0.3, 0.5, 3.0)]
    cloth = np.arange(len(H)) % 3
    out = _run(program, f"{name}_{st}", rows, _x4(x, H), psibar, cloth)
    head = out[0].split()
    assert head[:2] == ["C", "1"]
    y, eta, P = cr.hinge_records(cloth, rows)
    yep = np.array([int(w, 16) for w in head[2:]], np.uint32).reshape(3, 3)
    want = np.stack(cr.hinge_records(np.arange(3), rows), axis=1)
    assert np.array_equal(yep, _bits(want))
    psi, dpsi, nxt, yields = crease_hinge(_x4(x, H), psibar, y, eta, P)
    got = [ln.split() for ln in out[1:] if ln]
    assert len(got) == len(H)
    assert np.array_equal(np.array([g[0] == "1" for g in got]), sb.active(x, H))
    assert np.array_equal(np.array([g[1] == "1" for g in got]), yields)
    words = np.array([[int(w, 16) for w in g[2:]] for g in got], np.uint32)
    assert np.array_equal(words, np.stack([_bits(psi), _bits(dpsi), _bits(nxt)], axis=1))


@pytest.mark.parametrize("row", [(-0.1, 0, 0), (np.nan, 0, 0), (np.pi, 0, 0), (3.2, 0, 0), (np.inf, 0, 0),
                                 (0.1, -0.1, 0), (0.1, 1.0, 0), (0.1, np.nan, 0), (0.1, 0, -1.0), (0.1, 0, 3.2), (0.1, 0, np.nan)])
def test_parameter_check_refuses_bad_rows(program, row):
    """crease_params says no to a yield_angle outside {0} u (0, pi) or NaN, a hardening outside [0, 1), a max_angle
    outside {0} u (0, pi] (the engine's refusal of the same values is tests/test_creases_gpu.py's)"""
    out = _run(program, "bad", [row], np.zeros((0, 4, 3), F), np.zeros(0, F), [])
    assert out[0].split()[:2] == ["C", "0"]
