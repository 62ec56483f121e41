"""The host tables of shell bending (drake_amd/csrc/mpm_shell.h) on the CPU, word for word: the hinge list of mesh_hinges
and the gather table of shell_rows, against the numpy restatement of tests/shell_bending.py.

The tables are host code that compiles without HIP, so a small stand-alone program (its own main, the host compiler,
address and undefined-behaviour sanitizers) includes mpm_shell.h, reads the cases below from a file and prints every
table: the hinges' four vertex ids, row_pid, slice_off and every record of the gather table (padding included).  Nothing
is preloaded and no GPU is touched.

Expected, stated in tests/shell_bending.py independently of the product: a hinge per edge with exactly two faces, in
ascending (min, max), x0 -> x1 as the face with the lower id runs the edge; one row per vertex, its records
hinge << 2 | corner in ascending hinge id, slices of `slice` rows as wide as their longest row, column-major, padded
with 0xFFFFFFFF; slice_off[-1] == len(ent)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import shell_bending as sb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "drake_amd", "csrc")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]

PROGRAM = r"""
#include <cinttypes>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "mpm_shell.h"

using namespace mpm;

template <class T>
static void ints(const char* name, const std::vector<T>& v) {
    printf("%s", name);
    for (const T& x : v) printf(" %" PRId64, (int64_t)x);
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1]);
    std::string name, why;
    size_t n_verts, n_faces, slice;
    while (in >> name >> n_verts >> n_faces >> slice) {
        printf("case %s\n", name.c_str());
        std::vector<int32_t> idx(3 * n_faces);
        for (int32_t& i : idx) in >> i;
        if (!in) return 3;
        std::vector<ShellHinge> H;
        mesh_hinges(idx.data(), n_faces, H);
        std::vector<int32_t> ids4;
        for (const ShellHinge& h : H)
            for (int j = 0; j < 4; ++j) ids4.push_back(h.v[j]);
        ints("hinges", ids4);
        std::vector<int> row_vertex(n_verts);
        for (size_t v = 0; v < n_verts; ++v) row_vertex[v] = (int)v;
        RowTable<uint32_t> t;
        if (!shell_rows(ids4.data(), H.size(), row_vertex, n_faces, slice, t, why)) {
            printf("refused %s\n", why.c_str());
            continue;
        }
        ints("row_pid", t.row_pid);
        ints("slice_off", t.slice_off);
        ints("ent", t.ent);
    }
    return 0;
}
"""


def _non_manifold():
    """two fans around the edge (0, 1): three faces share it (no hinge there), the others pair up; vertex 7 is in no face"""
    return 8, np.array([(0, 1, 2), (1, 0, 3), (0, 1, 4), (2, 1, 5), (0, 2, 6), (4, 0, 3)], np.int32)


def _cases():
    out = {}
    for slice_ in (4, 64):
        for name in ("fan", "icosphere2"):
            X, T, _ = sb.mesh(name)
            out[f"{name}:{slice_}"] = (len(X), T, slice_)
        out[f"non_manifold:{slice_}"] = _non_manifold() + (slice_,)
    out["too_large"] = (len(sb.mesh("strip")[0]), sb.mesh("strip")[1], 1 << 31)
    return out


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    cc = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cc is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("shell_tables")
    src, exe, path = str(d / "dump.cc"), str(d / "dump"), str(d / "cases.txt")
    open(src, "w").write(PROGRAM)
    cases = _cases()
    with open(path, "w") as f:
        for name, (nv, T, slice_) in cases.items():
            f.write(f"{name} {nv} {len(T)} {slice_}\n" + " ".join(str(int(i)) for i in T.reshape(-1)) + "\n")
    subprocess.check_call([cc, *FLAGS, "-I", CSRC, src, "-o", exe])
    # (a sanitizer report ends the program with a non-zero status: check_output raises)
    got, cur = {}, None
    for ln in subprocess.check_output([exe, path]).decode().split("\n"):
        key, _, rest = ln.partition(" ")
        if key == "case":
            cur = got.setdefault(rest.strip(), {})
        elif key == "refused":
            cur[key] = rest
        elif key:
            cur[key] = np.array([int(w) for w in rest.split()], np.int64)
    assert set(got) == set(cases)
    return cases, got


@pytest.mark.parametrize("name", [n for n in _cases() if n != "too_large"])
def test_hinge_list_and_gather_table(tables, name):
    nv, T, slice_ = tables[0][name]
    got = tables[1][name]
    H = sb.hinges(T)
    assert np.array_equal(got["hinges"].reshape(-1, 4), H)
    row_pid, off, ent = sb.table_layout(H, range(nv), len(T), slice_)
    assert np.array_equal(got["row_pid"], row_pid)
    assert np.array_equal(got["slice_off"], off) and off[-1] == len(got["ent"])
    assert np.array_equal(got["ent"], ent)
    live = ent[ent != sb.PAD]
    assert len(live) == 4 * len(H) and (ent == sb.PAD).sum() == len(ent) - 4 * len(H)
    if name.startswith("fan"):                                  # the hub's row: 12 spokes and the 12 edges opposite
        rows = [[] for _ in range(nv)]
        for h in range(len(H)):
            for j in range(4):
                rows[H[h, j]].append(h)
        assert len(rows[0]) == 24 and max(len(r) for r in rows[1:]) < 24 and off[1] == 24 * slice_
    if name.startswith("icosphere2"):
        assert len(off) == {4: 42, 64: 4}[slice_]               # 162 rows: 41 slices of 4, three of 64
    if name.startswith("non_manifold"):
        assert len(H) == 4 and not any((min(h[0], h[1]), max(h[0], h[1])) == (0, 1) for h in H)
        assert 7 not in H                                       # an empty row: padding alone, where its slice has a width


def test_a_table_past_2_31_records_is_refused(tables):
    assert tables[1]["too_large"]["refused"] == "shell bending: the table is too large"
