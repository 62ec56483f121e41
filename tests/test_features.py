"""The feature table (drake_amd/csrc/mpm_features.h) on the CPU: every list function on every state.

The header is host code that compiles without HIP, so a small stand-alone program (its own main, the host compiler,
address and undefined-behaviour sanitizers) includes it alone, reads states from a file -- one per line: max_valence, dt,
the 13 on/off flags, the 13 max_dt, floats as their 32-bit words -- and prints the outcome of every list function with the
row's phrases.  Nothing is preloaded and no GPU is touched.

Expected, stated here independently of the table:
  single   each feature alone: the phrases and guard words below are literals copied from the host lists as they stood
           before the table (extensions_refused, fields_stable's dt_above_limit calls, rest_shape_conflict,
           single_engine_only's callers), not rebuilt from the rows.
  empty    nothing refused, the hint survives, the forces fuse at valence <= 8 and not at 9.
  all      all 2^13 on/off states against the earlier && chains, transcribed as boolean expressions; for the guards every
           subset of violated guards (2^6) on the engine with every guarded feature in force, and random subsets of
           features in force: the violated guard named is the first of anchors, shell, links, weave, damping, bending."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "drake_amd", "csrc")
FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]

PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>

#include "mpm_features.h"

using namespace mpm;

static const char* str(const char* s) { return s ? s : "-"; }
static float bits_float(uint32_t u) {
    float f;
    memcpy(&f, &u, sizeof f);
    return f;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    std::printf("count %d\n", (int)F_COUNT);
    for (int f = 0; f < F_COUNT; ++f) std::printf("what_is %d|%s\n", f, str(FEATURES[f].what_is));
    std::ifstream in(argv[1]);
    int valence;
    uint32_t u;
    while (in >> valence >> u) {
        const float dt = bits_float(u);
        FeatureState s;
        for (int f = 0; f < F_COUNT; ++f) {
            int on;
            in >> on;
            s.on[f] = on != 0;
        }
        for (int f = 0; f < F_COUNT; ++f) {
            in >> u;
            s.max_dt[f] = bits_float(u);
        }
        if (!in) return 3;
        const Feature halo = partition_blocker(s, false), set_up = partition_blocker(s, true), guard = violated_guard(s, dt),
                      rest = rest_shape_blocker(s);
        // (F_NONE indexes nothing: the phrases are read only behind the test)
        std::printf("state halo %d|%s|%s\n", (int)halo, halo == F_NONE ? "-" : str(FEATURES[halo].on_tail),
                    halo == F_NONE ? "-" : FEATURES[halo].phrase);
        std::printf("set_up %d|%s|%s\n", (int)set_up, set_up == F_NONE ? "-" : str(FEATURES[set_up].on_tail),
                    set_up == F_NONE ? "-" : FEATURES[set_up].phrase);
        std::printf("guard %d|%s|%s|%s|%a\n", (int)guard, guard == F_NONE ? "-" : FEATURES[guard].guard,
                    guard == F_NONE ? "-" : FEATURES[guard].force, guard == F_NONE ? "-" : FEATURES[guard].reduce,
                    guard == F_NONE ? 0.0 : (double)s.max_dt[guard]);
        std::printf("rest %d|%s\n", (int)rest, rest == F_NONE ? "-" : FEATURES[rest].phrase);
        std::printf("quiet %d\n", quiet_hint_holds(s) ? 1 : 0);
        std::printf("fused %d\n", forces_fusable(s, valence) ? 1 : 0);
        std::printf("max_dt");
        for (int f = 0; f < F_COUNT; ++f) std::printf(" %a", (double)max_stable_dt(s, (Feature)f));
        std::printf("\n");
    }
    return in.eof() ? 0 : 3;
}
"""

# the features in the order of extensions_refused
NAMES = ("pins", "materials", "grid_bodies", "force_fields", "bending", "damping", "weave", "tearing", "links", "pressure", "shell",
         "anchors", "rest_shape")
F = {n: k for k, n in enumerate(NAMES)}
NONE = len(NAMES)

# ---- literals of the host lists as they stood before the table --------------------------------------------------------------
# extensions_refused: "<what>: not available on " + ...
NOT_AVAILABLE_ON = {
    "pins": "an engine with pins (mpm_set_pins)",
    "materials": "a multi-material engine (mpm_add_qr_cloth_with_material)",
    "grid_bodies": "an engine with grid bodies (mpm_set_grid_bodies)",
    "force_fields": "an engine with force fields (mpm_set_force_fields)",
    "bending": "an engine with bending stiffness (mpm_set_bending)",
    "damping": "an engine with damping (mpm_set_damping)",
    "weave": "an engine with a weave (mpm_set_weave)",
    "tearing": "an engine with tearing (mpm_set_tearing, mpm_set_torn_faces)",
    "links": "an engine with links (mpm_set_links)",
    "pressure": "an engine with pressure (mpm_set_pressure)",
    "shell": "an engine with shell bending (mpm_set_shell_bending)",
    "anchors": "an engine with anchors (mpm_set_anchors)",
    "rest_shape": "an engine with a rest shape of its own (mpm_set_rest_shape; null restores the positions as added)",
}
# fields_stable: dt_above_limit(dt, max_dt, feature, force, reduce)
GUARD_WORDS = {
    "anchors": ("anchors", "anchor", "dt, the stiffness or the damping"),
    "shell": ("shell", "shell bending", "dt or the stiffness"),
    "links": ("links", "link", "dt, the stiffness or the damping"),
    "weave": ("weave", "weave", "dt or the moduli"),
    "damping": ("damping", "damping", "dt or the coefficients"),
    "bending": ("bending", "bending", "dt or the stiffness"),
}
GUARD_ORDER = ("anchors", "shell", "links", "weave", "damping", "bending")     # the order of fields_stable's tests
# rest_shape_conflict: "mpm_set_rest_shape: the engine has " + ...; tear_conflict takes three of the same
REST_PHRASE = {
    "bending": "bending stiffness (mpm_set_bending)",
    "shell": "shell bending (mpm_set_shell_bending)",
    "weave": "a weave (mpm_set_weave)",
    "damping": "damping (mpm_set_damping)",
    "pressure": "pressure (mpm_set_pressure)",
    "links": "links (mpm_set_links)",
    "anchors": "anchors (mpm_set_anchors)",
    "pins": "pins (mpm_set_pins)",
}
# single_engine_only's callers: "<what_is> not available on a partitioned or multi-rank engine"
WHAT_IS = {
    "pins": "pins are", "materials": "-", "grid_bodies": "grid bodies are", "force_fields": "force fields are",
    "bending": "bending stiffness is", "damping": "damping is", "weave": "the weave is", "tearing": "tearing is", "links": "links are",
    "pressure": "pressure is", "shell": "shell bending is", "anchors": "anchors are", "rest_shape": "a rest shape of its own is",
}


# ---- the lists as they stood, as boolean expressions ----------------------------------------------------------------------------
def quiet_hint(on):
    return (not on["force_fields"] and not on["bending"] and not on["damping"] and not on["weave"] and not on["tearing"]
            and not on["links"] and not on["pressure"] and not on["shell"] and not on["anchors"])


def fused_forces(on, max_valence):
    return (max_valence <= 8 and not on["bending"] and not on["links"] and not on["pressure"] and not on["shell"]
            and not on["anchors"])


def partition_refused(on, set_up):
    return (on["pins"] or on["materials"] or on["grid_bodies"] or on["force_fields"] or on["bending"] or on["damping"] or on["weave"]
            or on["tearing"] or on["links"] or on["pressure"] or on["shell"] or on["anchors"] or (set_up and on["rest_shape"]))


def rest_shape_blocked(on):
    return (on["bending"] or on["shell"] or on["weave"] or on["damping"] or on["pressure"] or on["links"] or on["anchors"]
            or on["pins"])


def first_violated(on, max_dt, dt):
    for k in GUARD_ORDER:
        if on[k] and not dt <= max_dt[k]:
            return k
    return None


# ---- running the program ------------------------------------------------------------------------------------------------------------
def _line(valence, dt, on, max_dt):
    bits = lambda x: str(int(np.float32(x).view(np.uint32)))   # noqa: E731
    return " ".join([str(valence), bits(dt)] + [str(int(on[n])) for n in NAMES] + [bits(max_dt.get(n, np.inf)) for n in NAMES])


def _parse(text):
    lines = text.strip().split("\n")
    assert lines[0] == f"count {len(NAMES)}"
    what_is = [ln.partition("|")[2] for ln in lines[1:1 + len(NAMES)]]
    out = []
    for ln in lines[1 + len(NAMES):]:
        key, _, rest = ln.partition(" ")
        if key == "state":
            out.append({})
            key, _, rest = rest.partition(" ")
        out[-1][key] = rest.split("|") if key in ("halo", "set_up", "guard", "rest") else rest.split()
    return what_is, out


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cc = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cc is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("features")
    src, exe = str(d / "lists.cc"), str(d / "lists")
    open(src, "w").write(PROGRAM)
    subprocess.check_call([cc, *FLAGS, "-I", CSRC, src, "-o", exe])

    def run(states):
        path = str(d / "states.txt")
        open(path, "w").write("\n".join(_line(*s) for s in states) + "\n")
        # (a sanitizer report ends the program with a non-zero status: check_output raises)
        what_is, got = _parse(subprocess.check_output([exe, path]).decode())
        assert len(got) == len(states)
        return what_is, got
    return run


def _on(*names):
    return {n: n in names for n in NAMES}


def _not_available_on(row):
    """the tail extensions_refused composes from a row: its own where it has one, else "an engine with <phrase>" """
    return row[1] if row[1] != "-" else "an engine with " + row[2]


def test_each_feature_alone(program):
    guard_dt = {n: 0.001 * (k + 2) for k, n in enumerate(GUARD_ORDER)}
    states = []
    for n in NAMES:   # per feature: dt above its guard, dt at it, and at valence 9
        states += [(8, 1.0, _on(n), guard_dt), (8, guard_dt.get(n, 1.0), _on(n), guard_dt), (9, 0.0, _on(n), guard_dt)]
    what_is, got = program(states)
    assert what_is == [WHAT_IS[n] for n in NAMES]
    for k, n in enumerate(NAMES):
        above, at, nine = got[3 * k:3 * k + 3]
        # the partitioned paths: every feature, the rest shape only at set-up
        assert int(above["set_up"][0]) == F[n] and _not_available_on(above["set_up"]) == NOT_AVAILABLE_ON[n], n
        if n == "rest_shape":
            assert above["halo"] == [str(NONE), "-", "-"]
        else:
            assert int(above["halo"][0]) == F[n] and _not_available_on(above["halo"]) == NOT_AVAILABLE_ON[n], n
        # the guard: refused above, accepted at the limit (dt <= max_dt), the words and the limit reported
        if n in GUARD_WORDS:
            assert above["guard"][:4] == [str(F[n]), *GUARD_WORDS[n]] and float.fromhex(above["guard"][4]) == np.float32(guard_dt[n]), n
        else:
            assert above["guard"][:4] == [str(NONE), "-", "-", "-"], n
        assert at["guard"][0] == str(NONE), n
        # mpm_<feature>_max_stable_dt: the limit of the feature in force, inf for every other
        want = [float(np.float32(guard_dt[m])) if m == n and m in GUARD_WORDS else np.inf for m in NAMES]
        assert [float.fromhex(x) for x in above["max_dt"]] == want, n
        # the rest shape
        assert above["rest"] == ([str(F[n]), REST_PHRASE[n]] if n in REST_PHRASE else [str(NONE), "-"]), n
        assert above["quiet"] == [str(int(quiet_hint(_on(n))))] and above["fused"] == [str(int(fused_forces(_on(n), 8)))], n
        assert nine["fused"] == ["0"], n
    assert sum(g["quiet"] == ["1"] for g in got[::3]) == 4 and sum(g["fused"] == ["1"] for g in got[::3]) == 8


def test_the_empty_state(program):
    _, got = program([(v, dt, _on(), {}) for v in (0, 6, 8, 9, 24) for dt in (0.0, 1.0, np.inf, np.nan)])
    for k, v in enumerate((0, 6, 8, 9, 24)):
        for g in got[4 * k:4 * k + 4]:
            assert g["halo"] == g["set_up"] == [str(NONE), "-", "-"] and g["guard"][0] == str(NONE) and g["rest"] == [str(NONE), "-"]
            assert g["quiet"] == ["1"] and g["fused"] == [str(int(v <= 8))]
            assert all(float.fromhex(x) == np.inf for x in g["max_dt"])


def test_all_on_off_states_against_the_chains(program):
    ons = [dict(zip(NAMES, bits)) for bits in itertools.product((False, True), repeat=len(NAMES))]
    assert len(ons) == 2 ** 13
    _, got = program([(8 + (k % 2), 0.0, on, {}) for k, on in enumerate(ons)])
    for k, (on, g) in enumerate(zip(ons, got)):
        assert (g["halo"][0] != str(NONE)) == partition_refused(on, False), on
        assert (g["set_up"][0] != str(NONE)) == partition_refused(on, True), on
        assert (g["rest"][0] != str(NONE)) == rest_shape_blocked(on), on
        assert g["quiet"] == [str(int(quiet_hint(on)))], on
        assert g["fused"] == [str(int(fused_forces(on, 8 + (k % 2))))], on
        # the first in the order of extensions_refused, i.e. the lowest index in force
        first = [n for n in NAMES if on[n] and n != "rest_shape"]
        assert int(g["halo"][0]) == (F[first[0]] if first else NONE), on
        assert int(g["set_up"][0]) == (F[first[0]] if first else F["rest_shape"] if on["rest_shape"] else NONE), on
        # (of several tables that block a new rest shape, the first in the same order is named)
        blockers = [n for n in NAMES if on[n] and n in REST_PHRASE]
        assert g["rest"] == ([str(F[blockers[0]]), REST_PHRASE[blockers[0]]] if blockers else [str(NONE), "-"]), on
        assert g["guard"][0] == str(NONE), on            # (dt = 0 violates no guard)


def test_guard_precedence(program):
    """dt = 1: a guard with max_dt 0.5 is violated, one with 2 is not.  Every subset of violated guards with all six
    features in force; then 512 random (in force, violated) pairs, among them guards violated on features that are off;
    and a NaN dt, which violates every guard in force."""
    rng = np.random.default_rng(13)
    cases = [(_on(*GUARD_ORDER), {n: 0.5 if v else 2.0 for n, v in zip(GUARD_ORDER, bits)}, 1.0)
             for bits in itertools.product((False, True), repeat=6)]
    for _ in range(512):
        on = {n: bool(rng.integers(2)) for n in NAMES}
        cases.append((on, {n: float(rng.choice([0.5, 1.0, 2.0, np.inf])) for n in GUARD_ORDER}, 1.0))
    cases += [(_on("damping", "links"), {n: np.inf for n in GUARD_ORDER}, np.nan), (_on("tearing"), {}, np.nan)]
    _, got = program([(8, dt, on, max_dt) for on, max_dt, dt in cases])
    seen = set()
    for (on, max_dt, dt), g in zip(cases, got):
        want = first_violated(on, {n: max_dt.get(n, np.inf) for n in GUARD_ORDER}, dt)
        seen.add(want)
        assert int(g["guard"][0]) == (F[want] if want else NONE), (on, max_dt, dt)
        if want:
            assert g["guard"][1:4] == list(GUARD_WORDS[want]) and float.fromhex(g["guard"][4]) == max_dt[want]
    assert seen == set(GUARD_ORDER) | {None}
    assert int(got[-2]["guard"][0]) == F["links"] and int(got[-1]["guard"][0]) == NONE
