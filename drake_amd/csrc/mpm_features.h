// The optional cloth features, each stated once: what the host has to know about a feature that is in force, and the
// lists that follow from it -- who refuses it, which dt guard it brings, whether the re-sort's quiet-time hint and the
// force fusion of ParticleToGrid survive it, whether a new rest shape has to wait for it.
// Plain C++17, no HIP and nothing of the engine: the rows are constants and the lists are pure functions of a
// FeatureState, which feature_state (mpm_host.h) fills from the engine.  tests/test_features.py compiles this header
// alone.  A new feature adds an enum entry and a row here, a line to feature_state, its launch and its entry points
// ("Adding a cloth feature").  The launches themselves stay explicit code in launch_fem_faces and
// launch_fem_vertices: each kernel has its own arguments and the order is part of the result.
#pragma once
#include <cmath>

namespace mpm {

// in the order in which a partitioned path names the feature it refuses (partition_blocker)
enum Feature {
    F_PINS, F_MATERIALS, F_GRID_BODIES, F_FORCE_FIELDS, F_BENDING, F_DAMPING, F_WEAVE, F_TEARING, F_LINKS, F_PRESSURE,
    F_SHELL, F_ANCHORS, F_REST_SHAPE,
    F_COUNT,
    F_NONE = F_COUNT   // what a list returns when no feature qualifies
};

// the halo, chain, dist and team paths (out of scope for every feature so far)
enum class Partitioned {
    Runs,             // the paths take an engine with the feature
    Refused,          // every one of them refuses it
    RefusedAtSetUp    // the calls that partition an engine or join it to other ranks refuse it; the halo substeps of a
                      // single engine run with it (the rest shape: they run on whatever rest state the engine holds)
};

struct FeatureRow {
    Feature id;
    const char* phrase;        // the feature as a refusal names it: "the engine has <phrase>", "an engine with <phrase>"
    const char* on_tail;       // "<call>: not available on <on_tail>" where that is not "an engine with <phrase>"; or null
    const char* what_is;       // "<what_is> not available on a partitioned or multi-rank engine"; null: nothing to set
    // the dt guard mpm_<guard>_max_stable_dt, as fields_stable words it: "the explicit <force> force is unstable --
    // reduce <reduce>"; all null: the feature has no max_dt guard
    const char *guard, *force, *reduce;
    bool adds_to_f;            // a kernel of its own adds to DP::f behind k_vforce: k_p2g cannot sum the forces itself
    bool ends_quiet_hint;      // the re-sort's quiet-time estimate assumes gravity alone
    // its host side caches something derived from the rest positions, Dm^-1, the volumes or the masses (what: the comment
    // on the row): mpm_set_rest_shape is refused while the table is in force
    bool caches_rest;
    Partitioned partitioned;
};

constexpr bool ADDS_TO_F = true, ENDS_HINT = true, CACHES_REST = true;
constexpr FeatureRow FEATURES[F_COUNT] = {
    // (caches nothing of its own: the bodies' impulse sums accumulate in the scale set_fixed_point_scales derives from
    // the total mass)
    {F_PINS, "pins (mpm_set_pins)", nullptr, "pins are", nullptr, nullptr, nullptr,
     !ADDS_TO_F, !ENDS_HINT, CACHES_REST, Partitioned::Refused},
    {F_MATERIALS, "per-cloth materials (mpm_add_qr_cloth_with_material)", "a multi-material engine (mpm_add_qr_cloth_with_material)", nullptr,
     nullptr, nullptr, nullptr, !ADDS_TO_F, !ENDS_HINT, !CACHES_REST, Partitioned::Refused},
    {F_GRID_BODIES, "grid bodies (mpm_set_grid_bodies)", nullptr, "grid bodies are", nullptr, nullptr, nullptr,
     !ADDS_TO_F, !ENDS_HINT, !CACHES_REST, Partitioned::Refused},
    {F_FORCE_FIELDS, "force fields (mpm_set_force_fields)", nullptr, "force fields are", nullptr, nullptr, nullptr,
     !ADDS_TO_F, ENDS_HINT, !CACHES_REST, Partitioned::Refused},
    // (k_bend, k_bend_damp; caches the cotangent weights of h_rest and the limit from the masses)
    {F_BENDING, "bending stiffness (mpm_set_bending)", nullptr, "bending stiffness is", "bending", "bending", "dt or the stiffness",
     ADDS_TO_F, ENDS_HINT, CACHES_REST, Partitioned::Refused},
    // (caches Dm^-1, volumes and masses of its Gershgorin sums)
    {F_DAMPING, "damping (mpm_set_damping)", nullptr, "damping is", "damping", "damping", "dt or the coefficients",
     !ADDS_TO_F, ENDS_HINT, CACHES_REST, Partitioned::Refused},
    // (caches the axes from h_rest; Dm^-1, volumes, masses)
    {F_WEAVE, "a weave (mpm_set_weave)", nullptr, "the weave is", "weave", "weave", "dt or the moduli",
     !ADDS_TO_F, ENDS_HINT, CACHES_REST, Partitioned::Refused},
    {F_TEARING, "tearing (mpm_set_tearing, mpm_set_torn_faces)", nullptr, "tearing is", nullptr, nullptr, nullptr,
     !ADDS_TO_F, ENDS_HINT, !CACHES_REST, Partitioned::Refused},
    // (k_link; caches the limit from the masses)
    {F_LINKS, "links (mpm_set_links)", nullptr, "links are", "links", "link", "dt, the stiffness or the damping",
     ADDS_TO_F, ENDS_HINT, CACHES_REST, Partitioned::Refused},
    // (k_pressure; the winding was checked against the rest volume)
    {F_PRESSURE, "pressure (mpm_set_pressure)", nullptr, "pressure is", nullptr, nullptr, nullptr,
     ADDS_TO_F, ENDS_HINT, CACHES_REST, Partitioned::Refused},
    // (k_hinge_gather; caches cbar, psibar and the guard's masses)
    {F_SHELL, "shell bending (mpm_set_shell_bending)", nullptr, "shell bending is", "shell", "shell bending", "dt or the stiffness",
     ADDS_TO_F, ENDS_HINT, CACHES_REST, Partitioned::Refused},
    // (k_anchor; caches the limit from the masses)
    {F_ANCHORS, "anchors (mpm_set_anchors)", nullptr, "anchors are", "anchors", "anchor", "dt, the stiffness or the damping",
     ADDS_TO_F, ENDS_HINT, CACHES_REST, Partitioned::Refused},
    {F_REST_SHAPE, "a rest shape of its own (mpm_set_rest_shape)",
     "an engine with a rest shape of its own (mpm_set_rest_shape; null restores the positions as added)", "a rest shape of its own is",
     nullptr, nullptr, nullptr, !ADDS_TO_F, !ENDS_HINT, !CACHES_REST, Partitioned::RefusedAtSetUp},
};
// Materials, force fields, tear limits and flags, grid colliders and bodies and contact materials cache nothing derived
// from the rest shape.

constexpr bool features_in_enum_order() {
    for (int f = 0; f < F_COUNT; ++f)
        if (FEATURES[f].id != f) return false;
    return true;
}
static_assert(features_in_enum_order(), "FEATURES: a row per Feature, in the enum's order");

// which features are in force, and the limit of each one's dt guard (read only where the row has a guard)
struct FeatureState {
    bool on[F_COUNT] = {};
    float max_dt[F_COUNT];
    FeatureState() {
        for (float& m : max_dt) m = INFINITY;
    }
};

// the first feature in force that a partitioned path refuses; set_up: the call partitions the engine or joins it to
// other ranks (mpm_dist_init, chain, team, world)
inline Feature partition_blocker(const FeatureState& s, bool set_up) {
    for (int f = 0; f < F_COUNT; ++f)
        if (s.on[f] && (FEATURES[f].partitioned == Partitioned::Refused || (set_up && FEATURES[f].partitioned == Partitioned::RefusedAtSetUp)))
            return (Feature)f;
    return F_NONE;
}
// the guard that dt violates: the LAST such feature in table order (a NaN dt violates every guard in force).  Every feature
// is tested alone: the guards do not compose, and a dt below all of them is not thereby stable for the sum of the forces
// ("What the dt guards bound"; 1 / sum_f (1 / max_dt[f]) over the guards in force would be sufficient).
inline Feature violated_guard(const FeatureState& s, float dt) {
    for (int f = F_COUNT - 1; f >= 0; --f)
        if (FEATURES[f].guard && s.on[f] && !(dt <= s.max_dt[f])) return (Feature)f;
    return F_NONE;
}
// what mpm_<guard>_max_stable_dt reports
inline float max_stable_dt(const FeatureState& s, Feature f) { return s.on[f] ? s.max_dt[f] : INFINITY; }
inline bool quiet_hint_holds(const FeatureState& s) {
    for (int f = 0; f < F_COUNT; ++f)
        if (s.on[f] && FEATURES[f].ends_quiet_hint) return false;
    return true;
}
// k_p2g may sum the vertex forces from the vertices' entries of DP::VF itself: no vertex of more than eight faces, and
// no kernel that adds to the forces k_vforce has written
inline bool forces_fusable(const FeatureState& s, int max_valence) {
    if (max_valence > 8) return false;
    for (int f = 0; f < F_COUNT; ++f)
        if (s.on[f] && FEATURES[f].adds_to_f) return false;
    return true;
}
// the first table in force that blocks mpm_set_rest_shape
inline Feature rest_shape_blocker(const FeatureState& s) {
    for (int f = 0; f < F_COUNT; ++f)
        if (s.on[f] && FEATURES[f].caches_rest) return (Feature)f;
    return F_NONE;
}

}  // namespace mpm
