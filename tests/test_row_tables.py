"""Vertex row tables (drake_amd/csrc/mpm_row_table.h) on the CPU, byte for byte: the tables that bending_table and
link_table lay out for k_bend / k_bend_damp / k_link, against a restatement of the layout in numpy.

The tables are host code that compiles without HIP, so a small stand-alone program (its own main, the host compiler,
address and undefined-behaviour sanitizers) includes mpm_bending.h and mpm_links.h, reads the cases below from a file and
prints every table: row_pid, slice_off, every record's raw 32-bit words (padding included), the links' pair records, the
guard's row sums as hex doubles, and for links the guard's rates and limit.  Nothing is preloaded and no GPU is touched.

Expected, stated here independently of the product:
  layout   one row per vertex in ascending id; slices of `slice` rows; a slice as wide as its longest row; record e of
           the slice's lane l at slice_off[s] + slice e + l; short rows padded with the row's padding record; the lanes
           past the last row hold the last row's padding; slice_off[-1] == len(ent); no rows: slice_off == [0].
  bending  from the CSR of drake_amd.bending_matrix (host only): a row per vertex of the cloths with k > 0, its records
           (float32(float64(k32) * val), nf + first_vertex + column) in ascending column order without the diagonal,
           padding (0, own id); abs_sum = sum |k val| with the diagonal.
  links    from the link list: two rows' entries per link, in link order inside a row, (nf + other end | flag in bit
           31, k, L, c), padding (own id, 0, 0, 0); pair records (nf + a, nf + b | flag, k, L); k_sum, c_sum per row.
Integers and record words must be equal.  The double sums are compared within n 2^-52 of the sum, n the row's term
count: the worst case of two summation orders of n non-negative terms (each of the n - 1 additions rounds a partial sum
that is at most the sum, by at most 2^-53 of it, in either order).
"too large" (a slice that would end at or past 2^31 records) is reached through the refusal alone: one slice of 2^31
rows, which is refused before anything is allocated."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import bending as bd
from tests import links as lk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "drake_amd", "csrc")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]

PROGRAM = r"""
#include <cinttypes>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "mpm_bending.h"
#include "mpm_links.h"

using namespace mpm;

struct Cloth {
    size_t first_vertex, n_verts, first_face, n_faces;
};
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
    std::ifstream in(argv[1]);
    std::string kind, name, why;
    while (in >> kind >> name) {
        printf("case %s\n", name.c_str());
        if (kind == "B") {
            size_t nf, slice, n_cloths, n_verts, n_faces;
            in >> nf >> slice >> n_cloths >> n_verts >> n_faces;
            std::vector<Cloth> cloths(n_cloths);
            std::vector<float> k(n_cloths), pos(3 * n_verts);
            std::vector<int> idx(3 * n_faces);
            for (size_t c = 0; c < n_cloths; ++c) {
                uint32_t u;
                in >> cloths[c].first_vertex >> cloths[c].n_verts >> cloths[c].first_face >> cloths[c].n_faces >> u;
                k[c] = bits_float(u);
            }
            for (float& x : pos) {
                uint32_t u;
                in >> u;
                x = bits_float(u);
            }
            for (int& i : idx) in >> i;
            if (!in) return 3;
            BendTable t;
            if (!bending_table(cloths, pos.data(), idx.data(), nf, n_cloths, k.data(), slice, t, why)) {
                printf("refused %s\n", why.c_str());
                continue;
            }
            ints("row_pid", t.row_pid);
            ints("slice_off", t.slice_off);
            words("ent", t.ent);
            doubles("abs_sum", t.abs_sum);
        } else if (kind == "L") {
            size_t nf, n_verts, slice, n;
            in >> nf >> n_verts >> slice >> n;
            std::vector<Link> links(n);
            std::vector<float> mass(n_verts);
            for (Link& q : links) {
                uint32_t k, L, c;
                in >> q.a >> q.b >> k >> L >> c >> q.flags;
                q.stiffness = bits_float(k);
                q.rest_length = bits_float(L);
                q.damping = bits_float(c);
            }
            for (float& x : mass) {
                uint32_t u;
                in >> u;
                x = bits_float(u);
            }
            if (!in) return 3;
            LinkTable t;
            if (!link_table(links.data(), n, nf, n_verts, slice, t, why)) {
                printf("refused %s\n", why.c_str());
                continue;
            }
            ints("row_pid", t.row_pid);
            ints("slice_off", t.slice_off);
            words("ent", t.ent);
            words("pair", t.pair);
            doubles("k_sum", t.k_sum);
            doubles("c_sum", t.c_sum);
            double W, G;
            link_rates(t, mass.data(), nf, &W, &G);
            doubles("rates", {W, G});
            words("limit", std::vector<float>{link_limit(W, G)});
        } else {
            return 4;
        }
    }
    return 0;
}
"""


# ---- the cases ------------------------------------------------------------------------------------------------------------
def _bending_case(meshes, ks, slice_=64):
    """cloths one behind the other, as the engine numbers them: (nf, slice, [(first_vertex, n_verts, first_face, n_faces,
    k)], X of all vertices, T of all faces in global vertex ids)"""
    cloths, X, T, v0, f0 = [], [], [], 0, 0
    for (x, t), k in zip(meshes, ks):
        cloths.append((v0, len(x), f0, len(t), np.float32(k)))
        X.append(x)
        T.append(t + v0)
        v0, f0 = v0 + len(x), f0 + len(t)
    return dict(nf=f0, slice=slice_, cloths=cloths, X=np.concatenate(X).astype(np.float32), T=np.concatenate(T).astype(np.int32))


def _bending_cases():
    out = {name: _bending_case([bd.mesh(name)], [0.75e-6]) for name in bd.MESHES}
    # rows absent in the middle: the ids jump over the k = 0 cloth; two hubs of 24, each in a slice of short rows
    out["fan_off_fan"] = _bending_case([bd.mesh("fan"), bd.mesh("regular"), bd.mesh("fan")], [0.5e-6, 0.0, 1.25e-6])
    out["rows64"] = _bending_case([bd.sheet(8, 8)], [1e-6])       # exactly one slice
    out["rows65"] = _bending_case([bd.sheet(5, 13)], [1e-6])      # one row in the second slice
    out["too_large"] = _bending_case([bd.mesh("strip")], [1e-6], slice_=1 << 31)
    return out


def _link_case(links, nf, n_verts, slice_=64, massless=()):
    mass = np.random.default_rng(3).uniform(1e-6, 3e-6, n_verts).astype(np.float32)
    mass[list(massless)] = 0.0
    return dict(nf=nf, n_verts=n_verts, slice=slice_, links=links, mass=mass)


def _link_cases():
    cloths, mixed, X = lk.scene("mixed")
    nf = sum(len(T) for _, T in cloths)
    spring, cord = (50.0, 0.5 * lk.H0, 0.03, 0), (70.0, 0.5 * lk.H0, 0.05, lk.TENSION)
    return {
        "mixed": _link_case(mixed, nf, len(X)),                 # > 64 rows, a partial last slice, a hub of 19
        "none": _link_case(lk.make_links([]), nf, len(X)),
        "same_pair_twice": _link_case(lk.make_links([(3, 9) + spring, (9, 3) + cord]), 7, 12),
        "rows64": _link_case(lk.make_links([(v, 100 + v) + (spring if v % 3 else cord) for v in range(32)]), nf, len(X)),
        "cord": _link_case(lk.make_links([(2, 5) + cord]), 4, 6),
        "massless": _link_case(lk.make_links([(0, 1) + spring, (1, 2) + spring]), 2, 3, massless=(1,)),
        "too_large": _link_case(lk.make_links([(0, 1) + spring]), 2, 3, slice_=1 << 31),
    }


def _bits(a):
    return " ".join(str(int(u)) for u in np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32))


def write_cases(path, bending, links):
    with open(path, "w") as f:
        for name, c in bending.items():
            f.write(f"B bend:{name} {c['nf']} {c['slice']} {len(c['cloths'])} {len(c['X'])} {len(c['T'])}\n")
            for v0, nv, f0, nfc, k in c["cloths"]:
                f.write(f"{v0} {nv} {f0} {nfc} {_bits(k)}\n")
            f.write(_bits(c["X"]) + "\n" + " ".join(str(int(i)) for i in c["T"].reshape(-1)) + "\n")
        for name, c in links.items():
            f.write(f"L link:{name} {c['nf']} {c['n_verts']} {c['slice']} {len(c['links'])}\n")
            for q in c["links"]:
                f.write(f"{q['a']} {q['b']} {_bits(q['stiffness'])} {_bits(q['rest_length'])} {_bits(q['damping'])} {q['flags']}\n")
            f.write(_bits(c["mass"]) + "\n")


def parse(text):
    """{case: {key: [tokens]}} of the program's output"""
    out, cur = {}, None
    for ln in text.split("\n"):
        if not ln.strip():
            continue
        key, _, rest = ln.partition(" ")
        if key == "case":
            cur = out.setdefault(rest.strip(), {})
        elif key == "refused":
            cur[key] = rest
        else:
            cur[key] = rest.split()
    return out


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    cc = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cc is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("row_tables")
    src, exe, cases = str(d / "dump.cc"), str(d / "dump"), str(d / "cases.txt")
    open(src, "w").write(PROGRAM)
    bending, links = _bending_cases(), _link_cases()
    write_cases(cases, bending, links)
    subprocess.check_call([cc, *FLAGS, "-I", CSRC, src, "-o", exe])
    # (a sanitizer report ends the program with a non-zero status: check_output raises)
    got = parse(subprocess.check_output([exe, cases]).decode())
    assert set(got) == {"bend:" + n for n in bending} | {"link:" + n for n in links}
    return bending, links, got


# ---- the layout, restated ---------------------------------------------------------------------------------------------
def layout(rows, pads, slice_, W):
    """rows: [row] (n_r, W) uint32 records; pads: [row] (W,) uint32 -> (slice_off (slices + 1,), ent (records, W))"""
    off, blocks = [0], []
    for s in range(0, len(rows), slice_):
        width = max(len(r) for r in rows[s:s + slice_])
        block = np.empty((width, slice_, W), np.uint32)          # column-major: [entry][lane]
        for lane in range(slice_):
            r = min(s + lane, len(rows) - 1)
            block[:, lane] = pads[r]
            if s + lane < len(rows):
                block[:len(rows[r]), lane] = rows[r]
        blocks.append(block.reshape(-1, W))
        off.append(off[-1] + width * slice_)
    return np.array(off, np.int64), np.concatenate(blocks) if blocks else np.zeros((0, W), np.uint32)


def _check_table(got, row_pid, rows, pads, slice_, W):
    off, ent = layout(rows, pads, slice_, W)
    assert np.array_equal(np.array(got["row_pid"], np.int64), np.array(row_pid, np.int64))
    assert np.array_equal(np.array(got["slice_off"], np.int64), off)
    words = np.array([int(w, 16) for w in got["ent"]], np.uint32).reshape(-1, W)
    assert off[-1] == len(words)
    assert np.array_equal(words, ent)


def _check_sums(got, terms):
    """terms: [row] the row's non-negative float64 terms"""
    got = np.array([float.fromhex(x) for x in got])
    assert len(got) == len(terms)
    for g, t in zip(got, terms):
        s = float(np.sum(t)) if len(t) else 0.0
        assert abs(g - s) <= len(t) * 2.0 ** -52 * s, (g, s, len(t))


@pytest.mark.parametrize("name", [n for n in _bending_cases() if n != "too_large"])
def test_bending_table(tables, name):
    from drake_amd import bending_matrix
    c, got = tables[0][name], tables[2]["bend:" + name]
    nf, row_pid, rows, pads, sums = c["nf"], [], [], [], []
    for v0, nv, f0, nfc, k in c["cloths"]:
        if not k > 0:
            continue
        off, cols, vals = bending_matrix(c["X"][v0:v0 + nv], c["T"][f0:f0 + nfc] - v0)
        kv = np.float64(k) * vals
        for v in range(nv):
            q = slice(off[v], off[v + 1])
            assert np.all(np.diff(cols[q]) > 0)
            keep = cols[q] != v
            pid = (nf + v0 + cols[q][keep]).astype(np.uint32)
            rows.append(np.stack([kv[q][keep].astype(np.float32).view(np.uint32), pid], 1).reshape(-1, 2))
            row_pid.append(nf + v0 + v)
            pads.append(np.array([0, nf + v0 + v], np.uint32))
            sums.append(np.abs(kv[q]))
    assert nf > 0 and len(rows)
    _check_table(got, row_pid, rows, pads, c["slice"], 2)
    _check_sums(got["abs_sum"], sums)
    if name == "triangle":                                   # rows of width 0: offsets, no record
        assert got["slice_off"] == ["0", "0"] and got["ent"] == []
    if name == "fan":                                        # one row of 24 in a slice of short rows, and a second slice
        n = [len(r) for r in rows]
        assert n[0] == 24 and max(n[1:64]) < 24 and got["slice_off"][1] == str(24 * 64) and len(got["slice_off"]) == 3
    if name == "fan_off_fan":
        assert np.diff(row_pid).max() > 1
    if name in ("rows64", "rows65"):
        assert len(got["slice_off"]) == {"rows64": 2, "rows65": 3}[name]


@pytest.mark.parametrize("name", [n for n in _link_cases() if n != "too_large"])
def test_link_table(tables, name):
    c, got = tables[1][name], tables[2]["link:" + name]
    nf, L = c["nf"], c["links"]
    flag = np.where(L["flags"] & lk.TENSION, 0x80000000, 0).astype(np.uint32)
    f32 = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)   # noqa: E731
    ent = {}
    for i in range(len(L)):                                  # link order inside a row: the links are visited in order
        for own, other in ((L["a"][i], L["b"][i]), (L["b"][i], L["a"][i])):
            ent.setdefault(int(own), []).append((np.uint32(nf + other) | flag[i], f32(L["stiffness"][i:i + 1])[0],
                                                 f32(L["rest_length"][i:i + 1])[0], f32(L["damping"][i:i + 1])[0], i))
    verts = sorted(ent)
    rows = [np.array([e[:4] for e in ent[v]], np.uint32) for v in verts]
    pads = [np.array([nf + v, 0, 0, 0], np.uint32) for v in verts]
    _check_table(got, [nf + v for v in verts], rows, pads, c["slice"], 4)
    pair = np.stack([(nf + L["a"]).astype(np.uint32), (nf + L["b"]).astype(np.uint32) | flag, f32(L["stiffness"]),
                     f32(L["rest_length"])], 1).reshape(-1, 4)
    assert np.array_equal(np.array([int(w, 16) for w in got["pair"]], np.uint32).reshape(-1, 4), pair)
    _check_sums(got["k_sum"], [L["stiffness"][[e[4] for e in ent[v]]].astype(np.float64) for v in verts])
    _check_sums(got["c_sum"], [L["damping"][[e[4] for e in ent[v]]].astype(np.float64) for v in verts])
    # the guard's rates from the program's own sums: max over rows of 2 sum / m in double, infinite on a massless row
    m = c["mass"].astype(np.float64)[verts]
    rates = []
    for key in ("k_sum", "c_sum"):
        s = np.array([float.fromhex(x) for x in got[key]])
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(s > 0, np.where(m > 0, 2.0 * s / m, np.inf), 0.0)
        rates.append(float(r.max()) if len(r) else 0.0)
    assert [float.fromhex(x) for x in got["rates"]] == rates
    if name == "none":
        assert got["slice_off"] == ["0"] and got["ent"] == [] and got["row_pid"] == [] and got["limit"] == ["7f800000"]
    if name == "mixed":
        n = [len(r) for r in rows]
        assert len(rows) > 128 and len(rows) % 64 and max(n) > 16
    if name == "rows64":
        assert len(rows) == 64 and len(got["slice_off"]) == 2
    if name == "cord":                                       # the flag on both records and on the pair
        assert rows[0][0, 0] >> 31 == 1 and rows[1][0, 0] >> 31 == 1 and pair[0, 1] >> 31 == 1 and pair[0, 0] >> 31 == 0
    if name == "massless":
        assert rates[0] == np.inf and got["limit"] == ["00000000"]


def test_a_table_past_2_31_records_is_refused(tables):
    assert tables[2]["bend:too_large"] == {"refused": "bending: the table is too large"}
    assert tables[2]["link:too_large"] == {"refused": "links: the table is too large"}
