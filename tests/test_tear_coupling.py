"""Tearing composed with shell bending and gas on the CPU (tests/tear_coupling.py holds the rule and the cut patterns).

1. What every cut pattern promises, asserted from numpy alone on the meshes the GPU tests use.
2. mpm_mesh_hinge_faces (host only) against tear_coupling.hinge_faces on every mesh of tests/shell_bending.py.
3. The hinge-to-face table of the host builder (shell_table of mpm_shell.h), word for word, on two-cloth scenes in which
   cloth 1's first_face is not 0: the ids must be GLOBAL face ids (the cloth's first face + the cloth-local id).  The
   table comes from a stand-alone host program with its own main, built with the address and undefined-behaviour
   sanitizers, in the manner of tests/test_shell_tables.py: nothing is loaded into Python and no GPU is touched.
4. The vent rule on top of pressure.gauge."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import pressure as pr
from tests import shell_bending as sb
from tests import tear_coupling as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "drake_amd", "csrc")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
MESHES = ("tube", "book", "icosphere1", "icosphere2", "jittered")


# ---- 1 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MESHES)
def test_patterns_promise_what_they_say(name):
    X, T, _ = sb.mesh(name)
    nv, nf = len(X), len(T)
    H, FAB = sb.hinges(T), tc.hinge_faces(T)
    assert len(H) == len(FAB) > 8 and (FAB[:, 0] < FAB[:, 1]).all()
    # a hinge's faces hold its edge; face A holds x2 and not x3, face B the other way round
    for h in range(len(H)):
        fa, fb = set(int(i) for i in T[FAB[h, 0]]), set(int(i) for i in T[FAB[h, 1]])
        assert {int(H[h, 0]), int(H[h, 1])} <= fa & fb and int(H[h, 2]) in fa - fb and int(H[h, 3]) in fb - fa
    per_vertex = tc._hinges_of_vertex(H, nv)

    torn, _ = tc.pattern("none", T, nv)
    assert not torn.any() and not tc.cut(torn, FAB).any() and tc.act(torn, FAB).all()
    torn, _ = tc.pattern("all", T, nv)
    assert torn.all() and tc.cut(torn, FAB).all()

    torn, what = tc.pattern("single", T, nv)
    assert torn.sum() == 1 and torn[what["face"]]
    c = tc.cut(torn, FAB)
    assert 1 <= c.sum() <= 3 and np.array_equal(c, (FAB == what["face"]).any(axis=1)) and not c.all()

    torn, what = tc.pattern("a_b_both", T, nv)
    a, b, both = what["only_a"], what["only_b"], what["both"]
    assert a is not None and b is not None and len({a, b, both}) == 3
    assert torn[FAB[a, 0]] and not torn[FAB[a, 1]]
    assert torn[FAB[b, 1]] and not torn[FAB[b, 0]]
    assert torn[FAB[both, 0]] and torn[FAB[both, 1]]
    c = tc.cut(torn, FAB)
    assert c[a] and c[b] and c[both] and not c.all()

    torn, what = tc.pattern("vertex_all", T, nv)
    v = what["vertex"]
    c = tc.cut(torn, FAB)
    assert len(per_vertex[v]) >= 4 and c[per_vertex[v]].all() and not c.all()

    torn, what = tc.pattern("vertex_mix", T, nv)
    c = tc.cut(torn, FAB)
    assert what["vertex"] == v and c[per_vertex[v]].any() and not c[per_vertex[v]].all()
    assert set(tc.PATTERNS) == {"single", "a_b_both", "vertex_all", "vertex_mix", "none", "all"} and nf > 0


# ---- 2 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sb.MESHES))
def test_mesh_hinge_faces_is_the_restatement(name):
    from drake_amd import mesh_hinge_faces, mesh_hinges
    X, T, _ = sb.mesh(name)
    got = mesh_hinge_faces(T, len(X))
    assert got.dtype == np.int32 and got.shape == (len(sb.hinges(T)), 2)
    assert np.array_equal(got, tc.hinge_faces(T))
    assert np.array_equal(mesh_hinges(T, len(X)), sb.hinges(T))


def test_mesh_hinge_faces_refuses_a_bad_id():
    from drake_amd import MpmError, mesh_hinge_faces
    with pytest.raises(MpmError) as e:
        mesh_hinge_faces(np.array([(0, 1, 5)], np.int32), 3)
    assert e.value.code == -1 and "out of range" in str(e.value)


# ---- 3 -------------------------------------------------------------------------------------------------------------------
PROGRAM = r"""
#include <cinttypes>
#include <cstdio>
#include <fstream>
#include <string>
#include <vector>

#include "mpm_shell.h"

using namespace mpm;

struct Cloth {
    size_t first_vertex, n_verts, first_face, n_faces;
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
    size_t n_cloths;
    while (in >> name >> n_cloths) {
        printf("case %s\n", name.c_str());
        std::vector<Cloth> cloths(n_cloths);
        std::vector<ClothShell> par(n_cloths);
        size_t nv = 0, nf = 0;
        for (size_t c = 0; c < n_cloths; ++c) {
            in >> cloths[c].n_verts >> cloths[c].n_faces >> par[c].stiffness;
            par[c].rest = SHELL_REST_SHAPE;
            cloths[c].first_vertex = nv;
            cloths[c].first_face = nf;
            nv += cloths[c].n_verts;
            nf += cloths[c].n_faces;
        }
        std::vector<int> idx(3 * nf);
        for (int& i : idx) in >> i;
        std::vector<float> shape(3 * nv);
        for (float& x : shape) in >> x;
        if (!in) return 3;
        ShellTable t;
        if (!shell_table(cloths, idx.data(), nf, par.data(), shape.data(), (size_t)SHELL_SLICE, t, why)) {
            printf("refused %s\n", why.c_str());
            continue;
        }
        ints("ids4", t.ids4);
        ints("faces2", t.faces2);
        ints("hinge_cloth", t.hinge_cloth);
    }
    return 0;
}
"""


def _two_cloths():
    """cloth 0 the book (32 faces), cloth 1 the icosphere (80 faces): first_face of cloth 1 is 32, first_vertex 25"""
    out = []
    for name in ("book", "icosphere1"):
        X, T, _ = sb.mesh(name)
        out.append((sb.rest_shape(name), T))
    return out


def _cases():
    cl = _two_cloths()
    return {"both": (cl, (1e-6, 1e-6)), "second_only": (cl, (0.0, 1e-6)), "first_only": (cl, (1e-6, 0.0)),
            "swapped": (cl[::-1], (1e-6, 2e-6))}


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    cc = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cc is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("tear_coupling_tables")
    src, exe, path = str(d / "dump.cc"), str(d / "dump"), str(d / "cases.txt")
    open(src, "w").write(PROGRAM)
    cases = _cases()
    with open(path, "w") as f:
        for name, (cloths, ks) in cases.items():
            f.write(f"{name} {len(cloths)}\n")
            off = 0
            tri, pos = [], []
            for (X, T), k in zip(cloths, ks):
                f.write(f"{len(X)} {len(T)} {k!r}\n")
                tri.append(T + off)
                pos.append(X)
                off += len(X)
            f.write(" ".join(str(int(i)) for i in np.concatenate(tri).reshape(-1)) + "\n")
            f.write(" ".join(repr(float(x)) for x in np.concatenate(pos).reshape(-1)) + "\n")
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


@pytest.mark.parametrize("name", list(_cases()))
def test_the_host_table_holds_global_face_ids(tables, name):
    cloths, ks = tables[0][name]
    got = tables[1][name]
    assert "refused" not in got, got
    want_ids, want_faces, want_cloth = [], [], []
    v0 = f0 = 0
    for c, ((X, T), k) in enumerate(zip(cloths, ks)):
        if k > 0:
            H, FAB = sb.hinges(T), tc.hinge_faces(T)
            want_ids.append(H + v0)
            want_faces.append(FAB + f0)                       # GLOBAL: the cloth's first face + the cloth-local id
            want_cloth.append(np.full(len(H), c))
        v0 += len(X)
        f0 += len(T)
    want_ids, want_faces, want_cloth = (np.concatenate(a) for a in (want_ids, want_faces, want_cloth))
    assert np.array_equal(got["ids4"].reshape(-1, 4), want_ids)
    assert np.array_equal(got["hinge_cloth"], want_cloth)
    faces = got["faces2"].reshape(-1, 2)
    assert np.array_equal(faces, want_faces)
    # the bug to catch: local ids.  Where the second cloth has hinges they lie at or above its first face
    n0 = len(cloths[0][1])
    if ks[1] > 0:
        second = got["hinge_cloth"] == 1
        assert second.any() and faces[second].min() >= n0 and faces[second].max() < n0 + len(cloths[1][1])
        local = want_faces.copy()
        local[second] -= n0
        assert not np.array_equal(faces, local)
    # every hinge's faces hold its edge, in the global numbering
    Tg = np.concatenate([T + o for (X, T), o in zip(cloths, np.cumsum([0] + [len(X) for X, _ in cloths[:-1]]))])
    for h in range(len(faces)):
        e = {int(want_ids[h, 0]), int(want_ids[h, 1])}
        assert e <= set(int(i) for i in Tg[faces[h, 0]]) and e <= set(int(i) for i in Tg[faces[h, 1]])


# ---- 4 -------------------------------------------------------------------------------------------------------------------
def test_the_vent_rule():
    table = pr.make_table([pr.gas_row("icosphere"), (pr.CONSTANT, 80.0, 0, 0, 0), (pr.OFF, 0, 0, 0, 0)])
    X, T = pr.mesh("icosphere")
    V = pr.volume64(X, T)
    g, capped, E = tc.gauge(table[0], V, vented=False)
    assert (g, capped, E) == pr.gauge(table[0], V) and g > 0
    g, capped, E = tc.gauge(table[0], V, vented=True)
    assert g == 0 and not np.signbit(g) and g.dtype == np.float32 and capped is False and E == 0.0
    # constant pressure and off are not gas: the flag changes nothing
    for c in (1, 2):
        assert tc.gauge(table[c], V, vented=True) == pr.gauge(table[c], V)
    cof = np.repeat([0, 1, 2], 4)
    torn = np.zeros(12, bool)
    assert not tc.vented(table, torn, cof).any()
    torn[[3, 5, 9]] = True
    assert tc.vented(table, torn, cof).tolist() == [True, False, False]
    assert not tc.vented(table, torn, cof, mask=tc.CUTS_HINGES).any()
