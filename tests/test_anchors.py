"""Anchors (mpm_set_anchors) on the CPU: no GPU is touched.

1. The entry points are declared in include/mpm_hip.h, bound in drake_amd.capi and exported; mpm_anchor_t is 36 bytes.
2. mpm_anchor_point -- pin_pose and the two formulas of the attachment point, compiled for the host -- against the float64
   Rodrigues formula of tests/pin_reference.py on both branches (|w| t < 1e-8 and above), and a quarter turn.  Bound: the
   double arithmetic is far below the one float rounding of the result, so every component lies within one float ulp at
   the scale of the vector, 2^-23 max|y| (2^-23 max|v_Q|).
3. The restatement's force (tests/anchors.py) is the negative gradient of its energy with respect to x, by central
   differences, on the scenes -- with c = 0: damping has no potential.  Step h = 1e-6: the difference quotient of
   1/2 k (l - L)^2 errs by O(k h^2 / l) from the third derivative and by 2^-52 E / h from the roundings of E; the test
   allows 1e-6 of the largest |k (l + L)| of the vertex's anchors.
4. The scenes cover the layouts the kernels' paths need; asserted so that the coverage cannot erode.
5. The table k_anchor reads, word for word.  The table is host code that compiles without HIP, so a small stand-alone
   program (its own main, the host compiler, address and undefined-behaviour sanitizers, as tests/test_row_tables.py
   builds its program) includes mpm_anchors.h, reads the cases from a file and prints row_pid, slice_off, every record's
   raw 32-bit words (padding included), the per-anchor records, the guard's sums, rates and limit.  Expected, stated here:
   one row per anchored vertex in ascending id, a row's entries in anchor order,
   (motion slot | flag in bit 31, k, L, c, p_BQ, body), padding (0, 0, 0, 0, 0, 0, 0, 0xFFFFFFFF); a body without a motion
   has slot 0x7FFFFFFF and marks the table unresolved.  Nothing is preloaded."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import anchors as an
from tests import links as lk
from tests import test_row_tables as rt
from tests.pin_reference import rodrigues

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "drake_amd", "csrc")
NAMES = ["mpm_set_anchors", "mpm_get_anchors", "mpm_anchor_forces", "mpm_anchor_state", "mpm_anchors_max_stable_dt", "mpm_anchor_point"]


# ---- 1 -------------------------------------------------------------------------------------------------------------
def test_symbols_and_layout():
    import ctypes
    from drake_amd import capi
    text = open(os.path.join(ROOT, "include", "mpm_hip.h")).read()
    declared = set(re.findall(r"MPM_API\s+[\w\s\*]+?\b(mpm_\w+)\s*\(", text))
    lib = capi.load_library()
    for name in NAMES:
        assert name in declared and name in capi.SYMBOLS and hasattr(lib, name), name
    assert ctypes.sizeof(capi.Anchor) == 36 and capi.ANCHOR_DTYPE.itemsize == 36 and an.ANCHOR_DTYPE == capi.ANCHOR_DTYPE
    assert capi.Anchor.p_BQ.offset == 8 and capi.Anchor.stiffness.offset == 20 and capi.Anchor.flags.offset == 32
    assert "#define MPM_ANCHOR_TENSION_ONLY 1u" in text and capi.ANCHOR_TENSION_ONLY == 1


# ---- 2 -------------------------------------------------------------------------------------------------------------
def _host_point(motion, t, q):
    from drake_amd import BodyMotion, anchor_point
    p, R, v, w = motion
    return anchor_point(BodyMotion(0, p, R, v, w), t, q)


@pytest.mark.parametrize("body", [0, 1, 2, 3, an.BODY_FAR])
def test_anchor_point_against_float64(body):
    _, anchors, motions, _ = an.scene("mixed")
    m = motions[body]
    th = an.CLOCK * float(np.linalg.norm(m[3].astype(np.float64)))
    assert {0: th == 0, 1: th == 0, 2: 0.5 < th < 2, 3: 0 < th < 1e-8, an.BODY_FAR: th > 1e-8}[body]
    sel = anchors[anchors["body"] == body]
    assert len(sel)
    y64, vq64, _, _ = an.points(sel, motions, an.CLOCK)
    for i in range(min(len(sel), 12)):
        y, vq = _host_point(m, an.CLOCK, sel["p_BQ"][i])
        assert np.abs(y - y64[i]).max() <= 2.0 ** -23 * np.abs(y64[i]).max()
        assert np.abs(vq - vq64[i]).max() <= 2.0 ** -23 * max(np.abs(vq64[i]).max(), 1e-300)


def test_anchor_point_quarter_turn():
    m = an.motion32((1.0, 2.0, 3.0), np.eye(3), (0.5, 0.0, 0.0), (0.0, 0.0, np.pi / 2))
    y, vq = _host_point(m, 1.0, (1.0, 0.0, 0.0))
    # R(1) turns e_x into e_y: y = p_WB + v + e_y, v_Q = v + w x e_y = v - (pi / 2) e_x
    assert np.abs(y - np.array([1.5, 3.0, 3.0])).max() <= 2.0 ** -23 * 3.0
    assert np.abs(vq - np.array([0.5 - np.pi / 2, 0.0, 0.0])).max() <= 2.0 ** -23 * (np.pi / 2)
    # and the restatement says the same
    y64, vq64, _, _ = an.points(an.make_anchors([(0, 0, (1.0, 0.0, 0.0), 1.0, 0.0, 0.0, 0)]), {0: m}, 1.0)
    assert np.abs(y - y64[0]).max() <= 2.0 ** -23 * 3.0 and np.abs(vq - vq64[0]).max() <= 2.0 ** -23 * 2.0
    assert np.allclose(rodrigues((0, 0, np.pi / 2)) @ (1, 0, 0), (0, 1, 0), atol=1e-15)


# ---- 3 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,st", [("mixed", "random"), ("mixed", "rotation"), ("hung", "random")])
def test_force_is_the_negative_gradient_of_the_energy(name, st):
    _, anchors, motions, X = an.scene(name)
    a = anchors.copy()
    a["damping"] = 0.0
    x, v = an.state(st, name, X)
    F, _, y32, _ = an.vertex_forces64(a, x, v, motions, an.CLOCK)
    assert np.abs(F).max() > 0

    def energy(xx):
        # (float64 positions: the energy as a smooth function, the gates as decided at x)
        d = y32.astype(np.float64) - xx[a["vertex"]]
        l = np.sqrt((d * d).sum(axis=1))
        return float((0.5 * a["stiffness"].astype(np.float64) * (l - a["rest_length"]) ** 2 * on).sum())

    _, _, l0, on = an.anchor_forces64(a, x, v, y32, np.zeros_like(y32))
    scale = np.zeros(len(X))
    np.maximum.at(scale, a["vertex"], a["stiffness"].astype(np.float64) * (l0 + a["rest_length"]))
    h, x64 = 1e-6, x.astype(np.float64)
    for vtx in np.unique(a["vertex"])[::7]:
        for j in range(3):
            xp, xm = x64.copy(), x64.copy()
            xp[vtx, j] += h
            xm[vtx, j] -= h
            g = (energy(xp) - energy(xm)) / (2 * h)
            assert abs(F[vtx, j] + g) <= 1e-6 * scale[vtx] + 1e-12, (vtx, j, F[vtx, j], g)


# ---- 4 -------------------------------------------------------------------------------------------------------------
def test_scenes_cover_the_layouts():
    c = an.coverage("hung")
    assert c["n"] == 4 and c["n_rows"] == 4 and c["bodies"] == [0]
    cloths, anchors, motions, X = an.scene("hung")
    x, _ = an.state("rest", "hung", X)
    _, _, y32, _ = an.points(anchors, motions, 0.0)
    assert np.array_equal(np.linalg.norm(y32.astype(np.float64) - x[anchors["vertex"]], axis=1), anchors["rest_length"].astype(np.float64))
    c = an.coverage("mixed")
    cloths, anchors, motions, X = an.scene("mixed")
    assert len(X) == 288 and c["n"] >= 200 and c["n_rows"] > 128 and c["n_rows"] % 64 and c["bare"] > 0
    assert set(c["lengths"]) >= {1, 2, 8, 9, 17}
    assert c["bodies"] == [0, 1, 2, 3, an.BODY_FAR, an.BODY_NONE] and an.BODY_FAR >= 32 and an.BODY_NONE >= an.N_BODIES > an.BODY_FAR
    w = {b: an.CLOCK * float(np.linalg.norm(m[3].astype(np.float64))) for b, m in motions.items()}
    assert w[0] == 0 and not motions[0][2].any() and w[1] == 0 and motions[1][2].any() and 0.5 < w[2] < 2 and 0 < w[3] < 1e-8
    # the five kinds, at every state: L = 0, springs stretched and compressed, cords slack and taut; the exact zero
    for st in an.STATES:
        x, v = an.state(st, "mixed", X)
        _, _, y32, vq32 = an.points(anchors, motions, an.CLOCK)
        _, _, l, on = an.anchor_forces64(anchors, x, v, y32, vq32)
        L, cord = anchors["rest_length"].astype(np.float64), (anchors["flags"] & an.TENSION) != 0
        assert (L == 0).any() and ((L > 0) & ~cord & (l > L)).any() and ((L > 0) & ~cord & (l < L) & on).any()
        assert (cord & ~on).any() and (cord & on).any()
        assert l[-1] ** 2 < 1e-30 and L[-1] > 0 and not on[-1]


# ---- 5 -------------------------------------------------------------------------------------------------------------
PROGRAM = r"""
#include <cinttypes>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "mpm_anchors.h"

using namespace mpm;

static float bits_float(uint32_t u) {
    float f;
    memcpy(&f, &u, sizeof f);
    return f;
}
template <class T>
static void ints(const char* name, const std::vector<T>& v) {
    printf("%s", name);
    for (const T& x : v) printf(" %" PRId64, (int64_t)x);
    printf("\n");
}
template <class T>
static void words(const char* name, const std::vector<T>& v) {
    static_assert(sizeof(T) % 4 == 0, "records are made of 32-bit words");
    std::vector<uint32_t> w(v.size() * (sizeof(T) / 4));
    if (!w.empty()) memcpy(w.data(), v.data(), w.size() * 4);
    printf("%s", name);
    for (uint32_t x : w) printf(" %08" PRIx32, x);
    printf("\n");
}
static void doubles(const char* name, const std::vector<double>& v) {
    printf("%s", name);
    for (double x : v) printf(" %a", x);
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    static_assert(sizeof(Anchor) == 36 && sizeof(AnchorRecord) == 32 && sizeof(AnchorOne) == 32, "layouts");
    std::ifstream in(argv[1]);
    std::string name, why;
    while (in >> name) {
        printf("case %s\n", name.c_str());
        size_t nf, n_verts, slice, n, n_slots;
        in >> nf >> n_verts >> slice >> n >> n_slots;
        std::vector<uint32_t> slots(n_slots);
        for (uint32_t& b : slots) in >> b;
        std::vector<Anchor> anchors(n);
        std::vector<float> mass(n_verts);
        for (Anchor& q : anchors) {
            uint32_t w[6];
            in >> q.vertex >> q.body >> w[0] >> w[1] >> w[2] >> w[3] >> w[4] >> w[5] >> q.flags;
            for (int j = 0; j < 3; ++j) q.p_BQ[j] = bits_float(w[j]);
            q.stiffness = bits_float(w[3]);
            q.rest_length = bits_float(w[4]);
            q.damping = bits_float(w[5]);
        }
        for (float& x : mass) {
            uint32_t u;
            in >> u;
            x = bits_float(u);
        }
        if (!in) return 3;
        const std::string refusal = anchor_table_refusal(anchors.data(), n, n_verts);
        if (!refusal.empty()) {
            printf("refused %s\n", refusal.c_str());
            continue;
        }
        auto slot_of = [&](uint32_t body) {
            for (size_t k = 0; k < slots.size(); ++k)
                if (slots[k] == body) return (uint32_t)k;
            return ANCHOR_NO_SLOT;
        };
        AnchorTable t;
        if (!anchor_table(anchors.data(), n, nf, n_verts, slice, slot_of, t, why)) {
            printf("refused %s\n", why.c_str());
            continue;
        }
        ints("row_pid", t.row_pid);
        ints("slice_off", t.slice_off);
        words("ent", t.ent);
        words("one", t.one);
        doubles("k_sum", t.k_sum);
        doubles("c_sum", t.c_sum);
        ints("unresolved", std::vector<int>{t.unresolved ? 1 : 0});
        double W, G;
        anchor_rates(t, mass.data(), nf, &W, &G);
        doubles("rates", {W, G});
        words("limit", std::vector<float>{link_limit(W, G)});
    }
    return 0;
}
"""


def _case(anchors, nf, n_verts, slots, slice_=64, massless=()):
    mass = np.random.default_rng(3).uniform(1e-6, 3e-6, n_verts).astype(np.float32)
    mass[list(massless)] = 0.0
    return dict(nf=nf, n_verts=n_verts, slice=slice_, anchors=anchors, slots=list(slots), mass=mass)


def _cases():
    cloths, mixed, motions, X = an.scene("mixed")
    nf = sum(len(T) for _, T in cloths)
    hung = an.scene("hung")
    spring, cord = (50.0, 0.5 * lk.H0, 0.03, 0), (70.0, 0.5 * lk.H0, 0.05, an.TENSION)
    p = (0.25, -0.5, 0.125)
    return {
        "mixed": _case(mixed, nf, len(X), [3, 2, an.BODY_NONE, 1, 0, an.BODY_FAR]),      # slots in another order than the bodies
        "hung": _case(hung[1], sum(len(T) for _, T in hung[0]), len(hung[3]), [0]),
        "none": _case(an.make_anchors([]), nf, len(X), [0]),
        "unresolved": _case(an.make_anchors([(3, 5, p) + spring, (3, 9, p) + cord]), 7, 12, [9]),
        "same_pair_twice": _case(an.make_anchors([(3, 1, p) + spring, (3, 1, p) + cord]), 7, 12, [0, 1]),
        "rows64": _case(an.make_anchors([(v, v % 3, p) + (spring if v % 3 else cord) for v in range(64)]), nf, len(X), [0, 1, 2]),
        "massless": _case(an.make_anchors([(0, 0, p) + spring, (1, 0, p) + spring]), 2, 3, [0], massless=(1,)),
        "too_large": _case(an.make_anchors([(0, 0, p) + spring]), 2, 3, [0], slice_=1 << 31),
        "bad_vertex": _case(an.make_anchors([(2, 0, p) + spring, (12, 0, p) + spring]), 7, 12, [0]),
        "bad_flags": _case(an.make_anchors([(2, 0, p) + spring, (3, 0, p) + (1.0, 0.0, 0.0, 2)]), 7, 12, [0]),
        "bad_k": _case(an.make_anchors([(2, 0, p) + spring, (3, 0, p) + (-1.0, 0.0, 0.0, 0)]), 7, 12, [0]),
        "bad_point": _case(an.make_anchors([(2, 0, p) + spring, (3, 0, (0.0, np.inf, 0.0)) + spring]), 7, 12, [0]),
    }


def _bits(a):
    return " ".join(str(int(u)) for u in np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32))


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    cc = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cc is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("anchor_tables")
    src, exe, path = str(d / "dump.cc"), str(d / "dump"), str(d / "cases.txt")
    open(src, "w").write(PROGRAM)
    cases = _cases()
    with open(path, "w") as f:
        for name, c in cases.items():
            f.write(f"{name} {c['nf']} {c['n_verts']} {c['slice']} {len(c['anchors'])} {len(c['slots'])}\n")
            f.write(" ".join(str(b) for b in c["slots"]) + "\n")
            for q in c["anchors"]:
                f.write(f"{q['vertex']} {q['body']} {_bits(q['p_BQ'])} {_bits(q['stiffness'])} {_bits(q['rest_length'])} "
                        f"{_bits(q['damping'])} {q['flags']}\n")
            f.write(_bits(c["mass"]) + "\n")
    subprocess.check_call([cc, *rt.FLAGS, "-I", CSRC, src, "-o", exe])
    # (a sanitizer report ends the program with a non-zero status: check_output raises)
    got = rt.parse(subprocess.check_output([exe, path]).decode())
    assert set(got) == set(cases)
    return cases, got


GOOD = ["mixed", "hung", "none", "unresolved", "same_pair_twice", "rows64", "massless"]


@pytest.mark.parametrize("name", GOOD)
def test_anchor_table(tables, name):
    c, got = tables[0][name], tables[1][name]
    nf, A = c["nf"], c["anchors"]
    f32 = lambda a: np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32)   # noqa: E731
    flag = np.where(A["flags"] & an.TENSION, 0x80000000, 0).astype(np.uint32)
    slot = np.array([c["slots"].index(b) if b in c["slots"] else 0x7FFFFFFF for b in A["body"].tolist()], np.uint32)
    rec = np.zeros((len(A), 8), np.uint32)
    if len(A):
        rec[:, 0] = slot | flag
        rec[:, 1], rec[:, 2], rec[:, 3] = f32(A["stiffness"]), f32(A["rest_length"]), f32(A["damping"])
        rec[:, 4:7] = f32(A["p_BQ"]).reshape(-1, 3)
        rec[:, 7] = A["body"]
    verts = sorted(set(A["vertex"].tolist()))
    mine = {v: [i for i in range(len(A)) if A["vertex"][i] == v] for v in verts}      # anchor order inside a row
    rows = [rec[mine[v]] for v in verts]
    pads = [np.array([0, 0, 0, 0, 0, 0, 0, 0xFFFFFFFF], np.uint32) for _ in verts]
    rt._check_table(got, [nf + v for v in verts], rows, pads, c["slice"], 8)
    one = rec.copy()
    if len(A):
        one[:, 0], one[:, 1], one[:, 2], one[:, 3], one[:, 7] = nf + A["vertex"], rec[:, 0], rec[:, 1], rec[:, 2], 0
    assert np.array_equal(np.array([int(w, 16) for w in got["one"]], np.uint32).reshape(-1, 8), one)
    rt._check_sums(got["k_sum"], [A["stiffness"][mine[v]].astype(np.float64) for v in verts])
    rt._check_sums(got["c_sum"], [A["damping"][mine[v]].astype(np.float64) for v in verts])
    assert got["unresolved"] == ["1" if (slot == 0x7FFFFFFF).any() else "0"]
    # the guard's rates from the program's own sums: max over rows of sum / m in double (the factor is 1), infinite on a
    # massless row; the limit is the float not above the positive root of W dt^2 + 2 G dt = 4
    m = c["mass"].astype(np.float64)[verts]
    rates = []
    for key in ("k_sum", "c_sum"):
        s = np.array([float.fromhex(x) for x in got[key]])
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(s > 0, np.where(m > 0, s / m, np.inf), 0.0)
        rates.append(float(r.max()) if len(r) else 0.0)
    assert [float.fromhex(x) for x in got["rates"]] == rates
    limit = np.array([int(got["limit"][0], 16)], np.uint32).view(np.float32)[0]
    if name == "none":
        assert got["slice_off"] == ["0"] and got["ent"] == [] and got["row_pid"] == [] and limit == np.inf
    elif name == "massless":
        assert rates[0] == np.inf and limit == 0
    else:
        W, G = rates
        root = 4.0 / (G + np.sqrt(G * G + 4 * W))
        assert limit <= root and np.nextafter(limit, np.float32(np.inf)) > root * (1 - 2.0 ** -50)
        assert abs(limit / an.max_stable_dt(A, c["mass"].astype(np.float64)) - 1) < 1e-6
    if name == "mixed":
        n = [len(r) for r in rows]
        assert len(rows) > 128 and len(rows) % 64 and max(n) == 17 and len(got["slice_off"]) == 4
        assert int(got["slice_off"][1]) == 17 * 64
    if name == "rows64":
        assert len(rows) == 64 and len(got["slice_off"]) == 2
    if name == "unresolved":
        assert rows[0][0, 0] == 0x7FFFFFFF and rows[0][1, 0] == 0x80000000


def test_refusals_of_the_table(tables):
    got = tables[1]
    assert got["too_large"] == {"refused": "anchors: the table is too large"}
    assert "anchor 1 names a vertex" in got["bad_vertex"]["refused"]
    assert "anchor 1: unknown flags" in got["bad_flags"]["refused"]
    assert "anchor 1: stiffness" in got["bad_k"]["refused"]
    assert "anchor 1: p_BQ" in got["bad_point"]["refused"]
