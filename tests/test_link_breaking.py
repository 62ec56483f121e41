"""Breakable links on the CPU (drake_amd/csrc/mpm_links.h; the model, scenes and bounds are in tests/link_breaking.py).

1. mpm_link_breaks, the host build of the function k_link_break calls, against the float64 verdict on every decided link
   of every scene x state with limits derived from the state; its l2 is, to the bit, the l2 of the force law as
   tests/links.py restates it in float32.
2. The knife edge, exact: d = (3 h, 4 h, 0) with h a power of two has l2 = 25 h^2; break_length = 5 h gives B2 == l2 and
   the link holds, the float below 5 h breaks it.  A NaN breaks nothing.
3. The conditions the derived limits must meet, on the reference alone: no link undecided, at least three quarters of a
   scene's links with a limit, both verdicts among seams, springs and tension-only links; and what the rows scenes are
   for: vertices with 7, 8 and 9 links, 63 / 64 / 65 linked vertices, 255 / 256 / 257 links, two slices of different
   width, a duplicate pair with two limits of which one breaks, a vertex all of whose links break, links within a cloth
   and across two.
4. entry_of_link word for word: link_table compiled into a stand-alone program (its own main, the host compiler, address
   and undefined-behaviour sanitizers; nothing is preloaded) against the restatement of the sliced-ELL positions."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import link_breaking as lb
from tests import links as lk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "drake_amd", "csrc")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _host(links, x, b):
    from drake_amd import capi
    B2 = capi.link_break_squared(b)
    assert np.array_equal(B2, lb.squared(b))
    l2, breaks = capi.link_breaks(x[links["a"]], x[links["b"]], B2)
    return l2, breaks & (B2 > 0)


# ---- 1 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,st", lb.CASES)
def test_host_function_against_float64(name, st):
    _, links, X = lb.scene(name)
    x, _ = lb.state(st, X)
    b = lb.limits(name, links, x)
    l2, breaks = _host(links, x, b)
    ref, decided, l2_64 = lb.verdicts64(links, x, b)
    assert np.array_equal(breaks[decided], ref[decided])
    err = np.abs(l2.astype(np.float64) - l2_64)
    assert np.all(err <= lb.R_BREAK * lb.U * l2_64), float((err / np.maximum(lb.U * l2_64, 1e-300)).max())
    # the l2 of the force law, in float32
    assert np.array_equal(l2.view(np.uint32), lk._l32(x[links["b"]] - x[links["a"]])[0].view(np.uint32))
    # even in d
    from drake_amd import capi
    l2r, br = capi.link_breaks(x[links["b"]], x[links["a"]], lb.squared(b))
    assert np.array_equal(l2r.view(np.uint32), l2.view(np.uint32)) and np.array_equal(br & (b > 0), breaks)


# ---- 2 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e", [-20, -7, 0, 5])
def test_knife_edge(e):
    from drake_amd import capi
    h = np.float32(2.0 ** e)
    xa = np.array([[0.25, 0.5, 0.75]], np.float32) * h
    xb = xa + np.array([[3, 4, 0]], np.float32) * h
    hold, cut = np.float32(5) * h, np.nextafter(np.float32(5) * h, np.float32(0))
    B2 = capi.link_break_squared([hold, cut])
    assert B2[0] == np.float32(25) * h * h and B2[1] < B2[0]
    l2, breaks = capi.link_breaks(np.repeat(xa, 2, 0), np.repeat(xb, 2, 0), B2)
    assert l2[0] == l2[1] == B2[0]
    assert not breaks[0] and breaks[1]


def test_nan_breaks_nothing():
    from drake_amd import capi
    xa = np.zeros((4, 3), np.float32)
    xb = np.array([[np.nan, 0, 0], [0, np.nan, 1], [1, 2, np.nan], [np.inf, 0, 0]], np.float32)
    l2, breaks = capi.link_breaks(xa, xb, np.float32(1e-6))
    assert np.isnan(l2[:3]).all() and not breaks[:3].any()
    assert breaks[3]                                      # (an infinite length is past every limit)


# ---- 3 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(lb.SCENES))
def test_conditions_of_the_derived_limits(name):
    _, links, X = lb.scene(name)
    kinds = lb.kind_of(links)
    for st in lb.STATES:
        x, _ = lb.state(st, X)
        b = lb.limits(name, links, x)
        breaks, decided, l2 = lb.verdicts64(links, x, b)
        assert l2.min() > 0 and decided.all(), (st, int((~decided).sum()))
        assert (b > 0).mean() >= 0.75, (st, float((b > 0).mean()))
        assert np.all((b == 0) | (b > links["rest_length"])) and np.isfinite(b).all()
        for k in range(3):
            sel = (kinds == k) & (b > 0)
            assert breaks[sel].any() and (~breaks[sel]).any(), (st, k)
        if name in lb.ROWS:
            n = len(links)
            assert {int(links["a"][n - 1]), int(links["b"][n - 1])} == {int(links["a"][n - 2]), int(links["b"][n - 2])}
            assert b[n - 2] > 0 and b[n - 1] > 0 and b[n - 2] != b[n - 1] and breaks[n - 1] and not breaks[n - 2]
            v = lb.doomed(links)
            mine = (links["a"] == v) | (links["b"] == v)
            assert mine.sum() >= 2 and breaks[mine].all()


@pytest.mark.parametrize("name", list(lb.ROWS))
def test_shapes_of_the_rows_scenes(name):
    _, links, X = lb.scene(name)
    n_linked, n_links = lb.ROWS[name]
    deg = np.bincount(np.concatenate([links["a"], links["b"]]), minlength=len(X))
    assert len(links) == n_links and (deg > 0).sum() == n_linked
    assert [int(deg[links["a"][i]]) for i in (0, 7, 15)] == [7, 8, 9]
    cloth = lambda v: v >= lb.NV                                                 # noqa: E731
    same = cloth(links["a"]) == cloth(links["b"])
    assert same.any() and (~same).any()
    _, off, rows = lb.entry_of_link(links, len(X), 64)
    assert len(off) - 1 == (n_linked + 63) // 64
    if name == "rows65":
        widths = np.diff(off) // 64
        assert len(widths) == 2 and widths[0] != widths[1] and widths.min() > 0


# ---- 4 -------------------------------------------------------------------------------------------------------------------
PROGRAM = r"""
#include <cinttypes>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "mpm_links.h"

using namespace mpm;

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::string name, why;
    size_t nf, n_verts, slice, n;
    while (in >> name >> nf >> n_verts >> slice >> n) {
        printf("case %s\n", name.c_str());
        std::vector<Link> links(n);
        for (Link& q : links) {
            in >> q.a >> q.b >> q.flags;
            q.stiffness = 1.f;
            q.rest_length = 0.f;
            q.damping = 0.f;
        }
        if (!in) return 3;
        LinkTable t;
        if (!link_table(links.data(), n, nf, n_verts, slice, t, why)) return 4;
        if (t.entry_of_link.size() != 2 * n) return 5;
        printf("slice_off");
        for (unsigned x : t.slice_off) printf(" %u", x);
        printf("\nentry");
        for (unsigned x : t.entry_of_link) {
            if (x >= t.ent.size()) return 6;
            printf(" %u", x);
        }
        // (the record each entry names: the other end's id with the flag, read through the position)
        printf("\nid");
        for (unsigned x : t.entry_of_link) printf(" %u", t.ent[x].id);
        printf("\n");
    }
    return 0;
}
"""


def _table_cases():
    out = {}
    for name in lb.SCENES:
        _, links, X = lb.scene(name)
        for slice_ in (4, 64):
            out[f"{name}:{slice_}"] = (200, len(X), slice_, links)
    out["none:64"] = (3, 8, 64, lk.make_links([]))
    out["same_pair_three_times:4"] = (7, 12, 4, lk.make_links([(3, 9, 1, 0, 0, 0), (9, 3, 1, 0, 0, 1), (3, 9, 1, 0, 0, 0)]))
    return out


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    cc = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cc is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("link_breaking")
    src, exe, path = str(d / "dump.cc"), str(d / "dump"), str(d / "cases.txt")
    open(src, "w").write(PROGRAM)
    cases = _table_cases()
    with open(path, "w") as f:
        for name, (nf, nv, slice_, links) in cases.items():
            f.write(f"{name} {nf} {nv} {slice_} {len(links)}\n")
            for q in links:
                f.write(f"{int(q['a'])} {int(q['b'])} {int(q['flags'])}\n")
    subprocess.check_call([cc, *FLAGS, "-I", CSRC, src, "-o", exe])
    # (a sanitizer report ends the program with a non-zero status: check_output raises)
    got, cur = {}, None
    for ln in subprocess.check_output([exe, path]).decode().split("\n"):
        key, _, rest = ln.partition(" ")
        if key == "case":
            cur = got.setdefault(rest.strip(), {})
        elif key:
            cur[key] = np.array([int(w) for w in rest.split()], np.int64)
    assert set(got) == set(cases)
    return cases, got


@pytest.mark.parametrize("name", list(_table_cases()))
def test_entry_of_link(tables, name):
    nf, nv, slice_, links = tables[0][name]
    got = tables[1][name]
    entry, off, _ = lb.entry_of_link(links, nv, slice_)
    assert np.array_equal(got["slice_off"], off if len(links) else [0])
    assert np.array_equal(got["entry"].reshape(-1, 2), entry)
    # distinct places, duplicate pairs included, each holding the other end's id and the link's flag
    assert len(np.unique(got["entry"])) == 2 * len(links)
    flag = (links["flags"].astype(np.int64) & 1) << 31
    ids = got["id"].reshape(-1, 2)
    assert np.array_equal(ids[:, 0], (nf + links["b"].astype(np.int64)) | flag)
    assert np.array_equal(ids[:, 1], (nf + links["a"].astype(np.int64)) | flag)
