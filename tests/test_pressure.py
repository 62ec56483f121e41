"""Enclosed-volume pressure on the CPU: mpm_pressure_vertex_force -- the inline row function the pressure kernel calls,
compiled for the host -- against the float64 restatement of tests/pressure.py inside the row bound on random rows; its
translation invariance to the bit; the exact zero of a padding-only row; on the closed meshes the restated force against
g grad V to the last bit and against central differences of the restated energy; mpm_mesh_is_closed on closed, open,
punctured, mis-wound, doubled and non-manifold meshes; and the row table word for word, printed by a stand-alone program
built under the address and undefined-behaviour sanitizers (nothing is preloaded, no GPU is touched)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import pressure as pr

U = pr.U
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "drake_amd", "csrc")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_exports():
    from drake_amd import capi
    lib = capi.load_library()
    for name in ("mpm_set_pressure", "mpm_get_pressure", "mpm_pressure_forces", "mpm_pressure_state", "mpm_mesh_is_closed",
                 "mpm_pressure_vertex_force"):
        assert name in capi.SYMBOLS and hasattr(lib, name), name
    assert capi.PRESSURE_DTYPE == pr.PRESSURE_DTYPE
    assert (capi.PRESSURE_OFF, capi.PRESSURE_CONSTANT, capi.PRESSURE_GAS) == (pr.OFF, pr.CONSTANT, pr.GAS)


# ---- the row function ----------------------------------------------------------------------------------------------------
def _random_rows(n, seed):
    """rows of 1 .. 24 entries around a vertex near the middle of the domain, corners 0.3 .. 3 H0 away"""
    r = np.random.default_rng(seed)
    rows = []
    for _ in range(n):
        m = int(r.integers(1, 25))
        xi = (0.5 + 0.2 * r.normal(size=3)).astype(np.float32)
        xb = (xi + pr.H0 * r.uniform(0.3, 3.0, (m, 1)) * r.normal(size=(m, 3))).astype(np.float32)
        xc = (xi + pr.H0 * r.uniform(0.3, 3.0, (m, 1)) * r.normal(size=(m, 3))).astype(np.float32)
        rows.append((np.float32(r.normal() * 100.0), xi, xb, xc))
    return rows


def _row64(g, xi, xb, xc):
    db, dc = xb.astype(np.float64) - xi.astype(np.float64), xc.astype(np.float64) - xi.astype(np.float64)
    f = float(g) / 6.0 * np.cross(db, dc).sum(axis=0)
    T = abs(float(g)) / 6.0 * float((np.linalg.norm(db, axis=1) * np.linalg.norm(dc, axis=1)).sum())
    return f, (pr.R_PRESSURE + len(xb)) * U * T


def test_host_function_against_float64():
    from drake_amd import pressure_vertex_force
    worst = 0.0
    for g, xi, xb, xc in _random_rows(3000, 1):
        f = pressure_vertex_force(g, xi, xb, xc)
        ref, bound = _row64(g, xi, xb, xc)
        assert np.isfinite(f).all()
        worst = max(worst, float(np.abs(f - ref).max() / bound))
    print(f"mpm_pressure_vertex_force: {worst:.3g} of the row bound")
    assert 0.0 < worst <= 1.0, worst


def test_translation_invariance_to_the_bit():
    """positions on a lattice of 2^-20 below 1/2: a shift by a lattice vector that keeps them below 1 changes no float
    difference, so the force must not change in any bit"""
    from drake_amd import pressure_vertex_force
    r = np.random.default_rng(2)
    q = 2.0 ** -20
    for _ in range(300):
        m = int(r.integers(1, 12))
        xi, xb, xc = (np.float32(q) * r.integers(1 << 17, 1 << 19, s).astype(np.float32) for s in ((3,), (m, 3), (m, 3)))
        t = np.float32(q) * r.integers(-(1 << 16), 1 << 18, 3).astype(np.float32)
        for a in (xi, xb, xc):
            assert np.array_equal((a + t).astype(np.float64), a.astype(np.float64) + t.astype(np.float64))
        f = pressure_vertex_force(77.5, xi, xb, xc)
        assert f.any()
        assert np.array_equal(_bits(pressure_vertex_force(77.5, xi + t, xb + t, xc + t)), _bits(f))


def test_padding_only_row_is_an_exact_zero():
    from drake_amd import pressure_vertex_force
    for xi in (np.array([0.3, 0.7, 0.5], np.float32), np.array([1e30, -3e-30, 7.0], np.float32)):
        pad = np.tile(xi, (5, 1))
        for g in (123.0, -1e30, 0.0):
            f = pressure_vertex_force(g, xi, pad, pad)
            # a zero of either sign (a negative g gives -0): f + (-0) is f in every bit, and +0 where f is +0
            assert not f.any() and np.isfinite(f).all(), (xi, g, f)
    assert not pressure_vertex_force(5.0, np.zeros(3, np.float32), np.zeros((0, 3)), np.zeros((0, 3))).any()
    # padding behind real entries changes nothing
    g, xi, xb, xc = _random_rows(1, 3)[0]
    f = pressure_vertex_force(g, xi, xb, xc)
    assert np.array_equal(_bits(pressure_vertex_force(g, xi, np.concatenate([xb, [xi, xi]]), np.concatenate([xc, [xi, xi]]))), _bits(f))


# ---- the restatement on the closed meshes -------------------------------------------------------------------------------
def _closed_state(name, st):
    X, T = pr.mesh(name)
    x = pr.state(st, X, np.zeros(len(X), int))
    return x, T


@pytest.mark.parametrize("name", pr.CLOSED)
@pytest.mark.parametrize("st", ["rest", "random"])
def test_restated_force_is_g_grad_v_to_the_last_bit(name, st):
    """grad V_i = 1/6 sum x_b x x_c over the faces (i, b, c); the restated force uses differences.  On float32
    positions in [1/4, 1) every coordinate and every difference is a multiple of 2^-25, every product one of 2^-50, and
    the partial sums stay far below 8 (a cross product's component is the difference of two nearly equal products):
    float64 forms both without a single rounding, so a closed fan must give the same bits."""
    x, T = _closed_state(name, st)
    assert x.min() >= 0.25 and x.max() < 1.0
    S, _, N = pr.cross_sums64(x, T, len(x))
    x64 = x.astype(np.float64)
    G = np.zeros_like(S)
    for k in range(3):
        np.add.at(G, T[:, k], np.cross(x64[T[:, (k + 1) % 3]], x64[T[:, (k + 2) % 3]]))
    assert np.array_equal(S, G), float(np.abs(S - G).max())
    g = 61.25
    assert np.array_equal((g / 6.0) * S, (g / 6.0) * G)
    assert N.min() >= 3 and np.abs(S).max() > 0


@pytest.mark.parametrize("name", pr.CLOSED)
@pytest.mark.parametrize("mode", ["constant", "gas"])
def test_restated_force_is_the_gradient_of_the_restated_energy(name, mode):
    """-dE/dx by central differences in float64.  V is linear in each single coordinate, so the difference quotient of
    -p V is exact up to rounding (about 2^-53 |E| / h, nine orders below the force at h = 1e-6); the gas energy adds
    a truncation term of order h^2 pv |dV/dx|^3 / V^3, smaller still.  Tolerance: 1e-7 of the largest force component."""
    X, T = pr.mesh(name)
    x = pr.state("random", X, np.zeros(len(X), int)).astype(np.float64)
    row = pr.make_table([(pr.CONSTANT, 60.0, 0, 0, 0) if mode == "constant" else pr.gas_row(name)])[0]

    def vol(xx):
        return float((xx[T[:, 0]] * np.cross(xx[T[:, 1]], xx[T[:, 2]])).sum()) / 6.0

    def energy(xx):
        V = vol(xx)
        if mode == "constant":
            return -float(row["p"]) * V
        return -float(row["pv"]) * np.log(V) + float(row["p_ambient"]) * V

    V0 = vol(x)
    g = float(row["p"]) if mode == "constant" else float(row["pv"]) / V0 - float(row["p_ambient"])
    assert mode == "constant" or float(row["pv"]) / V0 < float(row["p_max"])
    S, _, _ = pr.cross_sums64(x.astype(np.float32), T, len(x))
    F = g / 6.0 * S
    scale, h = float(np.abs(F).max()), 1e-6
    assert scale > 0
    r = np.random.default_rng(4)
    for i in r.choice(len(x), min(len(x), 30), replace=False):
        for j in range(3):
            xp, xm = x.copy(), x.copy()
            xp[i, j] += h
            xm[i, j] -= h
            d = -(energy(xp) - energy(xm)) / (2 * h)
            assert abs(d - F[i, j]) <= 1e-7 * scale, (i, j, d, F[i, j])


def test_meshes_are_what_the_issue_names():
    X, T = pr.mesh("tetrahedron")
    assert len(X) == 4 and len(T) == 4
    X, T = pr.mesh("icosphere")
    assert len(X) == 162 and len(T) == 320
    assert sorted(set(np.bincount(T.reshape(-1)))) == [5, 6]
    X, T = pr.mesh("bipyramid")
    assert len(X) == 22 and len(T) == 40 and np.bincount(T.reshape(-1)).max() == 20
    X, T = pr.mesh("sheet")
    assert len(X) == 144
    for name in pr.CLOSED:
        assert pr.volume64(*pr.mesh(name)) > 0
    cloths, table, X, T, cv, cf = pr.scene("mixed")
    assert list(table["mode"]) == [pr.GAS, pr.CONSTANT, pr.OFF, pr.CONSTANT] and table["p"][1] < 0
    st = pr.cloth_states(table, pr.state("collapsed", X, cv), T, cf)
    assert st[0][0] < 0 and st[0][2] and st[0][3] == 0.0
    assert not pr.cloth_states(table, X, T, cf)[0][2]


# ---- mpm_mesh_is_closed -----------------------------------------------------------------------------------------------------
def _open_cases():
    X, T = pr.mesh("icosphere")
    out = {"sheet": pr.mesh("sheet")[1], "face_removed": np.delete(T, 17, axis=0)}
    rev = T.copy()
    rev[40] = rev[40, [0, 2, 1]]
    out["face_reversed"] = rev
    out["face_duplicated"] = np.concatenate([T[:100], T[33:34], T[100:]])
    # an edge shared by three faces: a fin on the edge (a, b) of face 7, to a vertex of neither neighbour
    a, b = int(T[7, 0]), int(T[7, 1])
    around = {int(v) for f in T if a in f and b in f for v in f}
    c = next(v for v in range(len(X)) if v not in around)
    out["edge_of_three_faces"] = np.concatenate([T, [[a, b, c]]]).astype(np.int32)
    return out


def test_mesh_is_closed():
    from drake_amd import mesh_is_closed
    for name in pr.CLOSED:
        X, T = pr.mesh(name)
        assert pr.first_open_edge(T) is None
        assert mesh_is_closed(T, len(X)) == (True, None), name
    nv = {"sheet": 144}
    for name, T in _open_cases().items():
        want = pr.first_open_edge(T)
        assert want is not None, name
        closed, edge = mesh_is_closed(T, nv.get(name, 162))
        assert not closed and edge == want, (name, edge, want)
    assert mesh_is_closed(np.zeros((0, 3), np.int32), 0) == (True, None)
    assert mesh_is_closed([[0, 0, 1], [1, 0, 0]], 2)[0] is False           # a degenerate edge 0 -> 0
    from drake_amd import MpmError
    with pytest.raises(MpmError):
        mesh_is_closed([[0, 1, 5]], 3)


# ---- the table, word for word ---------------------------------------------------------------------------------------------
PROGRAM = r"""
#include <cinttypes>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "mpm_pressure.h"

using namespace mpm;

struct Cloth {
    size_t first_vertex, n_verts, first_face, n_faces;
};
struct I4 {
    int x, y, z, w;
};
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
    while (in >> name) {
        printf("case %s\n", name.c_str());
        size_t nf, slice, n_cloths;
        in >> nf >> slice >> n_cloths;
        std::vector<Cloth> cloths(n_cloths);
        std::vector<ClothPressure> modes(n_cloths);
        for (size_t c = 0; c < n_cloths; ++c) {
            in >> cloths[c].first_vertex >> cloths[c].n_verts >> cloths[c].first_face >> cloths[c].n_faces >> modes[c].mode;
            modes[c].p = modes[c].pv = modes[c].p_ambient = modes[c].p_max = 1.f;
        }
        std::vector<int> idx(3 * nf);
        for (int& i : idx) in >> i;
        if (!in) return 3;
        PressureTable t;
        if (!pressure_table(cloths, idx.data(), nf, modes.data(), slice, t, why)) {
            printf("refused %s\n", why.c_str());
            continue;
        }
        ints("row_pid", t.row_pid);
        ints("row_cloth", t.row_cloth);
        ints("slice_off", t.slice_off);
        std::vector<uint32_t> w;
        for (const PressureRecord& q : t.ent) {
            w.push_back(q.b);
            w.push_back(q.c);
        }
        ints("ent", w);
        std::vector<I4> chunks, ranges;
        pressure_chunks(cloths, [&](size_t c) { return modes[c].mode == PRESSURE_GAS; }, chunks, ranges);
        std::vector<int> flat;
        for (const I4& q : chunks) {
            flat.push_back(q.x);
            flat.push_back(q.y);
            flat.push_back(q.z);
        }
        ints("chunks", flat);
        flat.clear();
        for (const I4& q : ranges) {
            flat.push_back(q.x);
            flat.push_back(q.y);
        }
        ints("ranges", flat);
        int32_t edge[2] = {-1, -1};
        const bool closed = mesh_is_closed(idx.data(), nf, edge);
        printf("closed %d %d %d\n", closed ? 1 : 0, edge[0], edge[1]);
    }
    return 0;
}
"""


def _case(names, modes, slice_=64):
    cloths = [pr.mesh(n) if isinstance(n, str) else n for n in names]
    return dict(cloths=cloths, modes=list(modes), slice=slice_)


def _cases():
    names, table = pr.SCENES["mixed"]()
    big = pr.sheet(40, 40, (0.2, 0.2, 0.5))                      # 3042 faces: three chunks, the last one partial
    return {
        "mixed": _case(names, table["mode"]),                       # 310 rows: four full slices and a partial one
        "all_off": _case(names, [pr.OFF] * 4),
        "bipyramid": _case(["bipyramid"], [pr.GAS]),                # two rows of 20 in a slice of rows of 4
        "rows64": _case([pr.sheet(8, 8, (0.3, 0.3, 0.5))], [pr.CONSTANT]),
        "rows65": _case([pr.sheet(5, 13, (0.3, 0.3, 0.5))], [pr.CONSTANT]),
        "small_slices": _case(["tetrahedron", "bipyramid"], [pr.CONSTANT, pr.GAS], slice_=4),
        "chunks": _case(["icosphere", big, "tetrahedron", big], [pr.GAS, pr.GAS, pr.OFF, pr.GAS]),
        "too_large": _case(["tetrahedron"], [pr.CONSTANT], slice_=1 << 31),
    }


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    cc = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cc is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("pressure_table")
    src, exe, path = str(d / "dump.cc"), str(d / "dump"), str(d / "cases.txt")
    open(src, "w").write(PROGRAM)
    cases = _cases()
    with open(path, "w") as f:
        for name, c in cases.items():
            nf = sum(len(T) for _, T in c["cloths"])
            f.write(f"{name} {nf} {c['slice']} {len(c['cloths'])}\n")
            v0 = f0 = 0
            idx = []
            for (X, T), mode in zip(c["cloths"], c["modes"]):
                f.write(f"{v0} {len(X)} {f0} {len(T)} {int(mode)}\n")
                idx.append(T + v0)
                v0, f0 = v0 + len(X), f0 + len(T)
            f.write(" ".join(str(int(i)) for i in np.concatenate(idx).reshape(-1)) + "\n")
    subprocess.check_call([cc, *FLAGS, "-I", CSRC, src, "-o", exe])
    # (a sanitizer report ends the program with a non-zero status: check_output raises)
    out, cur = {}, None
    for ln in subprocess.check_output([exe, path]).decode().split("\n"):
        key, _, rest = ln.partition(" ")
        if key == "case":
            cur = out.setdefault(rest.strip(), {})
        elif key == "refused":
            cur[key] = rest
        elif key:
            cur[key] = [int(t) for t in rest.split()]
    assert set(out) == set(cases)
    return cases, out


@pytest.mark.parametrize("name", [n for n in _cases() if n != "too_large"])
def test_pressure_table(tables, name):
    c, got = tables[0][name], tables[1][name]
    row_pid, row_cloth, slice_off, ent = pr.table_layout(c["cloths"], c["modes"], c["slice"])
    assert np.array_equal(np.array(got["row_pid"], np.int64), row_pid)
    assert np.array_equal(np.array(got["row_cloth"], np.int64), row_cloth)
    assert np.array_equal(np.array(got["slice_off"], np.int64), slice_off)
    assert np.array_equal(np.array(got["ent"], np.int64).reshape(-1, 2), ent) and slice_off[-1] == len(ent)
    # the chunk list of the gas cloths: runs of at most 1024 consecutive face ids inside one cloth
    chunks, ranges, f0 = [], [], 0
    for k, ((X, T), mode) in enumerate(zip(c["cloths"], c["modes"])):
        first = len(chunks)
        if mode == pr.GAS:
            chunks += [(k, b, min(f0 + len(T), b + 1024)) for b in range(f0, f0 + len(T), 1024)]
        ranges.append((first, len(chunks)))
        f0 += len(T)
    assert np.array_equal(np.array(got["chunks"], np.int64).reshape(-1, 3), np.array(chunks, np.int64).reshape(-1, 3))
    assert np.array_equal(np.array(got["ranges"], np.int64).reshape(-1, 2), np.array(ranges, np.int64))
    nf = sum(len(T) for _, T in c["cloths"])
    if name == "mixed":
        assert len(row_pid) == 310 and len(slice_off) == 6 and 2 not in row_cloth
        assert got["closed"][0] == 0                                # (the sheet's boundary)
    if name == "all_off":
        assert got["row_pid"] == [] and got["slice_off"] == [0] and got["ent"] == [] and got["chunks"] == []
    if name == "bipyramid":
        assert slice_off[1] == 20 * 64 and got["closed"] == [1, -1, -1]
        assert (ent[0 * 64 + 21] != nf + 21).all() and (ent[19 * 64 + 0] == nf + 0).all()   # the apex's row is full, the ring's padded
    if name in ("rows64", "rows65"):
        assert len(slice_off) == {"rows64": 2, "rows65": 3}[name]
    if name == "chunks":
        assert [r[1] - r[0] for r in ranges] == [1, 3, 0, 3]


def test_a_table_past_2_31_records_is_refused(tables):
    assert tables[1]["too_large"] == {"refused": "pressure: the table is too large"}
