// Every method of include/gpu_mpm.hpp that allocates a buffer for the C ABI or forwards a caller's size, in front of the
// stub of tests/facade_stub.cc, under the address and undefined-behaviour sanitizers (tests/test_facade.py builds and runs
// it).  Checked per method: each returned vector has exactly the documented length and the stub's pattern from its first
// to its last byte (the stub writes the extent mpm_hip.h documents: a vector made too small is a sanitizer report, one
// made too large fails here); the stub's log shows the pointer or null, the count and the bytes mpm_hip.h calls for; a
// size argument other than the engine's count throws std::invalid_argument.  One "ok <Method>" line per method; arguments
// name the methods to run (none: all).  -DFACADE_PARENT leaves out what the header did not have before the size checks.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <set>
#include <string>

#include "facade_stub.h"
#include "mpm_driver.hpp"

using namespace drake::multibody::gmpm;
using stub::holds;
using stub::N;
using State = GpuMpmState<float>;
using Solver = GpuMpmSolver<float>;
using Args = std::vector<long long>;

static const char* current = "";
#define CHECK(cond)                                                                                   \
    do {                                                                                              \
        if (!(cond)) {                                                                                \
            std::fprintf(stderr, "FAILED %s: %s (line %d)\n", current, #cond, __LINE__);             \
            std::exit(1);                                                                             \
        }                                                                                             \
    } while (0)

// the k-th call of `fn` from the end of the log (0: the last)
static const stub::Call& call(const char* fn, size_t back = 0) {
    for (size_t k = stub::LOG.size(); k-- > 0;)
        if (stub::LOG[k].fn == fn && back-- == 0) return stub::LOG[k];
    std::fprintf(stderr, "FAILED %s: no call of %s in the log\n", current, fn);
    std::exit(1);
}
static size_t calls(const char* fn) {
    size_t n = 0;
    for (const auto& c : stub::LOG) n += c.fn == fn;
    return n;
}
// n items of an input table, every byte different from its neighbours'
template <class R>
static std::vector<R> items(size_t n, unsigned seed) {
    std::vector<R> v(n);
    unsigned char* b = reinterpret_cast<unsigned char*>(v.data());
    for (size_t k = 0; k < n * sizeof(R); ++k) b[k] = (unsigned char)(seed + 7u * k);
    return v;
}
// an empty vector whose data() is not null: "empty means null" must look at the size, not at the pointer
static std::vector<float> emptied() {
    std::vector<float> v(4, 1.f);
    v.clear();
    return v;
}
static std::vector<float> floats(size_t n, float first) {
    std::vector<float> v(n);
    for (size_t k = 0; k < n; ++k) v[k] = first + float(k);
    return v;
}
template <class R>
static void append(std::vector<unsigned char>* b, const std::vector<R>& v) {
    const unsigned char* p = reinterpret_cast<const unsigned char*>(v.data());
    b->insert(b->end(), p, p + v.size() * sizeof(R));
}
template <class F>
static bool invalid_argument(F f) {
    try {
        f();
    } catch (const std::invalid_argument&) {
        return true;
    }
    return false;
}
// a size argument must be the engine's count: every other number throws, before the C ABI is reached
template <class F>
static void wrong_sizes(const char* fn, size_t right, F f, bool zero_is_a_default = false) {
#ifndef FACADE_PARENT
    const size_t before = calls(fn);
    for (size_t n : {size_t(0), right - 1, right + 1, N.verts, N.faces, N.cloths, N.hinges, N.links, 3 * right})
        if (n != right && !(n == 0 && zero_is_a_default)) CHECK(invalid_argument([&] { f(n); }));
    CHECK(calls(fn) == before);
    f(right);   // and the object is as usable as before
#else
    (void)fn; (void)right; (void)f;
#endif
}

// ---- the sixteen evaluators that take their extent from the caller ---------------------------------------------------------
static void vertex_forces(State& s, const char* fn, std::vector<float> (State::*m)(size_t) const) {
    CHECK(holds((s.*m)(N.verts), 3 * N.verts, fn));
    CHECK(call(fn).args == Args{1});
    wrong_sizes(fn, N.verts, [&](size_t n) { (s.*m)(n); });
}
static void weave_forces(State& s, Solver&) {
    const char* fn = "mpm_weave_forces";
    CHECK(holds(s.WeaveForces(N.verts), 3 * N.verts, "mpm_weave_forces.f"));
    CHECK((call(fn).args == Args{1, 0}));
    {   // records that held something before: the facade sizes them, whatever n_faces says
        std::vector<float> rec(2, 1.f);
        CHECK(holds(s.WeaveForces(N.verts, &rec), 3 * N.verts, "mpm_weave_forces.f"));
        CHECK(holds(rec, 9 * N.faces, "mpm_weave_forces.rec"));
        CHECK((call(fn).args == Args{1, 1}));
    }
    {   // fresh records
        std::vector<float> rec;
        s.WeaveForces(N.verts, &rec);
        CHECK(holds(rec, 9 * N.faces, "mpm_weave_forces.rec"));
        CHECK((call(fn).args == Args{1, 1}));
    }
    {   // records larger than needed, n_faces given
        std::vector<float> rec(1000, 1.f);
        s.WeaveForces(N.verts, &rec, N.faces);
        CHECK(holds(rec, 9 * N.faces, "mpm_weave_forces.rec"));
    }
    wrong_sizes(fn, N.verts, [&](size_t n) { s.WeaveForces(n); });
    wrong_sizes(fn, N.faces, [&](size_t n) {
        std::vector<float> rec;
        s.WeaveForces(N.verts, &rec, n);
    }, true);
}
static void per_face(State& s, const char* fn, size_t per, std::vector<float> (State::*m)(size_t) const) {
    CHECK(holds((s.*m)(N.faces), per * N.faces, fn));
    CHECK(call(fn).args == Args{1});
    wrong_sizes(fn, N.faces, [&](size_t n) { (s.*m)(n); });
}
static void tear_state(State& s, Solver&) {
    const char* fn = "mpm_tear_state";
    CHECK(holds(s.TearState(N.faces), N.faces, "mpm_tear_state.torn"));
    std::vector<uint32_t> counts(1, 9u);
    CHECK(holds(s.TearState(N.faces, &counts), N.faces, "mpm_tear_state.torn"));
    CHECK(holds(counts, N.cloths, "mpm_tear_state.counts"));
    CHECK((call(fn).args == Args{1, 1, (long long)N.cloths, 1}));
    CHECK((call(fn, 1).args == Args{0, 0, 0, 1}));
    wrong_sizes(fn, N.faces, [&](size_t n) { s.TearState(n); });
}
static void tear_measure(State& s, Solver&) {
    const char* fn = "mpm_tear_measure";
    CHECK(holds(s.TearMeasure(N.faces), 2 * N.faces, "mpm_tear_measure.mq"));
    CHECK((call(fn).args == Args{1, 0}));
    std::vector<uint8_t> fail(40, 1);
    CHECK(holds(s.TearMeasure(N.faces, &fail), 2 * N.faces, "mpm_tear_measure.mq"));
    CHECK(holds(fail, N.faces, "mpm_tear_measure.would_fail"));
    CHECK((call(fn).args == Args{1, 1}));
    wrong_sizes(fn, N.faces, [&](size_t n) { s.TearMeasure(n, &fail); });
}
static void shell_cut_hinges(State& s, Solver&) {
    const char* fn = "mpm_shell_cut_hinges";
    CHECK(holds(s.ShellCutHinges(N.hinges), N.hinges, "mpm_shell_cut_hinges.cut"));
    std::vector<uint32_t> counts;
    CHECK(holds(s.ShellCutHinges(N.hinges, &counts), N.hinges, "mpm_shell_cut_hinges.cut"));
    CHECK(holds(counts, N.cloths, "mpm_shell_cut_hinges.counts"));
    CHECK((call(fn).args == Args{1, 1, (long long)N.cloths, 1}));
    wrong_sizes(fn, N.hinges, [&](size_t n) { s.ShellCutHinges(n); });
#ifndef FACADE_PARENT
    CHECK(s.ShellHingeCount() == N.hinges);
    CHECK((call("mpm_shell_hinges").args == Args{0, 0, 0, 0, 1}));
#endif
}
static void shell_damping_power(State& s, Solver&) {
    CHECK(holds(s.ShellDampingPower(N.cloths), N.cloths, "mpm_shell_damping_state.power"));
    CHECK((call("mpm_shell_damping_state").args == Args{1, 0}));
    wrong_sizes("mpm_shell_damping_state", N.cloths, [&](size_t n) { s.ShellDampingPower(n); });
}
static void shell_energy(State& s, Solver&) {
    CHECK(holds(s.ShellEnergy(N.cloths), N.cloths, "mpm_shell_state.energy"));
    CHECK((call("mpm_shell_state").args == Args{1, 0, 0}));
    wrong_sizes("mpm_shell_state", N.cloths, [&](size_t n) { s.ShellEnergy(n); });
}

// ---- the two-call getters ----------------------------------------------------------------------------------------------------
template <class R>
static void table(const char* fn, size_t count, const std::vector<R>& got) {
    CHECK(holds(got, count, fn));
    CHECK((call(fn).args == Args{1, (long long)count, 1}));
    CHECK((call(fn, 1).args == Args{0, 0, 1}));
}
// ---- setters: the count, the pointer (null for an empty optional table) and the bytes ----------------------------------------
template <class R, class F>
static void set_table(const char* fn, size_t n, F set) {
    const auto t = items<R>(n, 3);
    set(t);
    CHECK((call(fn).args == Args{(long long)n, 1}));
    std::vector<unsigned char> want;
    append(&want, t);
    CHECK(call(fn).bytes == want);
    set(std::vector<R>());
    CHECK(call(fn).args[0] == 0 && call(fn).bytes.empty());
}

static void tearing(State& s, Solver&) {
    const std::vector<float> limits{1.5f, 0.f, 2.25f};
    s.SetTearing(limits);
    const stub::Call& c = call("mpm_set_tearing");
    CHECK((c.args == Args{3, 1}));
    std::vector<mpm_cloth_tear_t> sent(3);
    CHECK(c.bytes.size() == sizeof(mpm_cloth_tear_t) * 3);
    std::memcpy(sent.data(), c.bytes.data(), c.bytes.size());
    for (size_t k = 0; k < 3; ++k) {
        CHECK(sent[k].stretch_limit == limits[k]);
        for (float r : sent[k].reserved) CHECK(r == 0.f);
    }
    const auto got = s.GetTearing();
    CHECK(got.size() == N.cloths);
    for (size_t k = 0; k < got.size(); ++k) CHECK(got[k] == stub::tear_limit(k));
    CHECK((call("mpm_get_tearing").args == Args{1, (long long)N.cloths, 1}));
    s.SetTearing({});
    CHECK(call("mpm_set_tearing").args[0] == 0);
}
static void link_energy(State& s, Solver&) {
    CHECK(s.LinkEnergy() == stub::LINK_ENERGY);
    CHECK((call("mpm_link_energy").args == Args{1, 0}));
    std::vector<float> len(3, 1.f);
    CHECK(s.LinkEnergy(&len) == stub::LINK_ENERGY);
    CHECK(holds(len, N.links, "mpm_link_energy.length"));
    CHECK((call("mpm_link_energy").args == Args{1, 1}));
    const size_t links = N.links;
    N.links = 0;   // no links: lengths come back empty and the C ABI is given null
    CHECK(s.LinkEnergy(&len) == stub::LINK_ENERGY && len.empty());
    CHECK((call("mpm_link_energy").args == Args{1, 0}));
    N.links = links;
}
static void link_break_state(State& s, Solver&) {
    CHECK(holds(s.LinkBreakState(), N.links, "mpm_link_break_state"));
    uint32_t count = 0;
    CHECK(holds(s.LinkBreakState(&count), N.links, "mpm_link_break_state"));
    CHECK(count == stub::BROKEN);
}
static void link_break_measure(State& s, Solver&) {
    CHECK(holds(s.LinkBreakMeasure(), N.links, "mpm_link_break_measure.l2"));
    CHECK((call("mpm_link_break_measure").args == Args{1, 0}));
    std::vector<uint8_t> would(1, 1);
    CHECK(holds(s.LinkBreakMeasure(&would), N.links, "mpm_link_break_measure.l2"));
    CHECK(holds(would, N.links, "mpm_link_break_measure.would_break"));
    CHECK((call("mpm_link_break_measure").args == Args{1, 1}));
}
static void anchor_state(State& s, Solver&) {
    for (int mask = 0; mask < 8; ++mask) {
        std::vector<float> len(2, 1.f), pts(50, 1.f);
        double q = 0;
        CHECK(s.AnchorState(mask & 1 ? &len : nullptr, mask & 2 ? &pts : nullptr, mask & 4 ? &q : nullptr) == stub::ANCHOR_ENERGY);
        CHECK((call("mpm_anchor_state").args == Args{1, mask & 1, (mask >> 1) & 1, (mask >> 2) & 1}));
        if (mask & 1) CHECK(holds(len, N.anchors, "mpm_anchor_state.length"));
        if (mask & 2) CHECK(holds(pts, 3 * N.anchors, "mpm_anchor_state.point"));
        if (mask & 4) CHECK(q == stub::ANCHOR_QUANTUM);
    }
    const size_t anchors = N.anchors;
    N.anchors = 0;
    std::vector<float> len(2, 1.f), pts(5, 1.f);
    s.AnchorState(&len, &pts);
    CHECK(len.empty() && pts.empty());
    CHECK((call("mpm_anchor_state").args == Args{1, 0, 0, 0}));
    N.anchors = anchors;
}
static void crease_state(State& s, Solver&) {
    CHECK(holds(s.CreaseState(), N.hinges, "mpm_crease_state.psibar"));
    std::vector<uint32_t> counts(9, 1u);
    CHECK(holds(s.CreaseState(&counts), N.hinges, "mpm_crease_state.psibar"));
    CHECK(holds(counts, N.cloths, "mpm_crease_state.counts"));
    CHECK((call("mpm_crease_state").args == Args{1, 1, (long long)N.cloths, 1}));
}
static void crease_measure(State& s, Solver&) {
    for (int mask = 0; mask < 4; ++mask) {
        std::vector<float> psi(1, 1.f), dpsi(30, 1.f);
        CHECK(holds(s.CreaseMeasure(mask & 1 ? &psi : nullptr, mask & 2 ? &dpsi : nullptr), N.hinges, "mpm_crease_measure.next"));
        CHECK((call("mpm_crease_measure").args == Args{mask & 1, (mask >> 1) & 1, 1}));
        if (mask & 1) CHECK(holds(psi, N.hinges, "mpm_crease_measure.psi"));
        if (mask & 2) CHECK(holds(dpsi, N.hinges, "mpm_crease_measure.dpsi"));
    }
}
static void weave_energy(State& s, Solver&) {
    CHECK(holds(s.WeaveEnergy(), N.cloths, "mpm_weave_energy"));
    CHECK((call("mpm_weave_energy").args == Args{1, (long long)N.cloths, 1, 0}));
    double total = 0;
    CHECK(holds(s.WeaveEnergy(&total), N.cloths, "mpm_weave_energy"));
    CHECK(total == stub::WEAVE_TOTAL);
    CHECK((call("mpm_weave_energy").args == Args{1, (long long)N.cloths, 1, 1}));
}
static void measure(State& s, Solver&) {
    CHECK(holds(s.Measure(), N.cloths, "mpm_measure.rows"));
    CHECK((call("mpm_measure").args == Args{1, (long long)N.cloths, 1, 0}));
    mpm_cloth_measure_t total{};
    CHECK(holds(s.Measure(&total), N.cloths, "mpm_measure.rows"));
    CHECK(total.kinetic == stub::KINETIC && total.bending == stub::BENDING);
    CHECK((call("mpm_measure").args == Args{1, (long long)N.cloths, 1, 1}));
}
static void kinetic(State& s, Solver&) {
    CHECK(s.CalcKineticEnergy() == stub::KINETIC + stub::KINETIC_AFFINE);
    CHECK((call("mpm_measure").args == Args{0, 0, 0, 1}));
}
static void potential(State& s, Solver&) {
    CHECK(s.CalcPotentialEnergy() == stub::GRAVITY + stub::IN_PLANE + stub::NORMAL + stub::SHEAR + stub::BENDING);
    CHECK((call("mpm_measure").args == Args{0, 0, 0, 1}));
}
static void rest_shape(State& s, Solver&) {
    CHECK(holds(s.GetRestShape(), 3 * N.verts, "mpm_get_rest_shape"));
    bool set = false;
    CHECK(holds(s.GetRestShape(&set), 3 * N.verts, "mpm_get_rest_shape") && set);
}
static void set_rest_shape(State& s, Solver&) {
    const auto rest = floats(3 * N.verts, 0.25f);
    s.SetRestShape(rest);
    std::vector<unsigned char> want;
    append(&want, rest);
    CHECK(call("mpm_set_rest_shape").args == Args{1} && call("mpm_set_rest_shape").bytes == want);
    s.ClearRestShape();
    CHECK(call("mpm_set_rest_shape").args == Args{0});
    CHECK(invalid_argument([&] { s.SetRestShape(floats(3 * N.verts - 1, 0.f)); }));
    CHECK(invalid_argument([&] { s.SetRestShape(floats(N.verts, 0.f)); }));
    CHECK(invalid_argument([&] { s.SetRestShape({}); }));
}
static void set_torn_faces(State& s, Solver&) {
    const auto torn = items<uint8_t>(N.faces, 5);
    s.SetTornFaces(torn);
    CHECK(call("mpm_set_torn_faces").args == Args{1} && call("mpm_set_torn_faces").bytes == torn);
    const size_t before = calls("mpm_set_torn_faces");
    CHECK(invalid_argument([&] { s.SetTornFaces(items<uint8_t>(N.faces - 1, 5)); }));
    CHECK(invalid_argument([&] { s.SetTornFaces(items<uint8_t>(N.verts, 5)); }));
    CHECK(calls("mpm_set_torn_faces") == before);
}
static void set_weave(State& s, Solver&) {
    const auto w = items<mpm_cloth_weave_t>(N.cloths, 9);
    const auto dirs = floats(3 * N.faces, 0.5f);
    std::vector<unsigned char> want;
    append(&want, w);
    s.SetWeave(w);
    CHECK((call("mpm_set_weave").args == Args{(long long)N.cloths, 1, 0}) && call("mpm_set_weave").bytes == want);
    s.SetWeave(w, {});
    CHECK((call("mpm_set_weave").args == Args{(long long)N.cloths, 1, 0}) && call("mpm_set_weave").bytes == want);
    const auto none = emptied();
    CHECK(none.empty() && none.data() != nullptr);
    s.SetWeave(w, none);
    CHECK((call("mpm_set_weave").args == Args{(long long)N.cloths, 1, 0}) && call("mpm_set_weave").bytes == want);
    s.SetWeave(w, dirs);
    append(&want, dirs);
    CHECK((call("mpm_set_weave").args == Args{(long long)N.cloths, 1, 1}) && call("mpm_set_weave").bytes == want);
    s.SetWeave({});
    CHECK(call("mpm_set_weave").args[0] == 0 && call("mpm_set_weave").args[2] == 0);
}
static void set_shell_bending(State& s, Solver&) {
    const auto k = items<mpm_cloth_shell_t>(N.cloths, 11);
    const auto rest = floats(3 * N.verts, 2.f);
    std::vector<unsigned char> want;
    append(&want, k);
    s.SetShellBending(k);
    CHECK((call("mpm_set_shell_bending").args == Args{(long long)N.cloths, 1, 0}) && call("mpm_set_shell_bending").bytes == want);
    s.SetShellBending(k, emptied());
    CHECK((call("mpm_set_shell_bending").args == Args{(long long)N.cloths, 1, 0}) && call("mpm_set_shell_bending").bytes == want);
    s.SetShellBending(k, rest);
    append(&want, rest);
    CHECK((call("mpm_set_shell_bending").args == Args{(long long)N.cloths, 1, 1}) && call("mpm_set_shell_bending").bytes == want);
    s.SetShellBending({});
    CHECK(call("mpm_set_shell_bending").args[0] == 0 && call("mpm_set_shell_bending").args[2] == 0);
}
static void set_crease_state(State& s, Solver&) {
    const auto psibar = floats(N.hinges, 0.125f);
    std::vector<unsigned char> want;
    append(&want, psibar);
    s.SetCreaseState(psibar);
    CHECK(call("mpm_set_crease_state").args == Args{1} && call("mpm_set_crease_state").bytes == want);
    s.SetCreaseState({});
    CHECK(call("mpm_set_crease_state").args == Args{0});
    s.SetCreaseState(psibar);
    s.SetCreaseState(emptied());
    CHECK(call("mpm_set_crease_state").args == Args{0});
}
static void set_broken_links(State& s, Solver&) {
    set_table<uint8_t>("mpm_set_broken_links", N.links, [&](const std::vector<uint8_t>& t) { s.SetBrokenLinks(t); });
}
static void dump_cpu_state(State& s, Solver&) {
    const auto d = s.DumpCpuState();
    CHECK(holds(std::get<0>(d), N.verts, "mpm_dump_cpu_state.pos"));
    CHECK(holds(std::get<1>(d), 3 * N.faces, "mpm_dump_cpu_state.indices"));
    CHECK((call("mpm_dump_cpu_state").args == Args{1, 1}));
}
static void sync_particles(State& s, Solver& solver) {
    s.positions_host().assign(2, Vec3<float>{1, 1, 1});
    solver.SyncParticleStateToCpu(&s);
    CHECK(holds(s.positions_host(), N.particles(), "mpm_sync_particle_state_to_cpu"));
}
static mpm_collider_t a_collider() { return items<mpm_collider_t>(1, 17)[0]; }
static void collider_distance(State& s, Solver& solver) {
    const mpm_collider_t c = a_collider();
    const auto x = floats(15, 0.1f);
    std::vector<float> phi(1, 1.f), grad(99, 1.f);
    solver.ColliderSignedDistance(s, c, x, &phi, &grad);
    CHECK(holds(phi, 5, "mpm_collider_signed_distance.phi") && holds(grad, 15, "mpm_collider_signed_distance.grad"));
    std::vector<unsigned char> want;
    append(&want, std::vector<mpm_collider_t>{c});
    append(&want, x);
    CHECK((call("mpm_collider_signed_distance").args == Args{1, 5}) && call("mpm_collider_signed_distance").bytes == want);
}
static void sdf_collider_distance(State& s, Solver& solver) {
    const mpm_sdf_collider_t c = items<mpm_sdf_collider_t>(1, 19)[0];
    const auto x = floats(12, 0.2f);
    std::vector<float> phi, grad;
    solver.SdfColliderSignedDistance(s, c, x, &phi, &grad);
    CHECK(holds(phi, 4, "mpm_sdf_collider_signed_distance.phi") && holds(grad, 12, "mpm_sdf_collider_signed_distance.grad"));
    std::vector<unsigned char> want;
    append(&want, std::vector<mpm_sdf_collider_t>{c});
    append(&want, x);
    CHECK((call("mpm_sdf_collider_signed_distance").args == Args{1, 4}) && call("mpm_sdf_collider_signed_distance").bytes == want);
}
static void check_pairs(const MpmParticleContactPairs<float>& p) {
    CHECK(holds(p.particle_in_contact_index, N.contacts, "mpm_download_contact_pairs.particle"));
    CHECK(holds(p.non_mpm_id, N.contacts, "mpm_download_contact_pairs.body"));
    CHECK(holds(p.penetration_distance, N.contacts, "mpm_download_contact_pairs.dist"));
    CHECK(holds(p.normal, N.contacts, "mpm_download_contact_pairs.normal"));
    CHECK(holds(p.particle_in_contact_position, N.contacts, "mpm_download_contact_pairs.position"));
    CHECK(holds(p.rigid_v, N.contacts, "mpm_download_contact_pairs.rigid_v"));
    CHECK(holds(p.rigid_p_WB, N.contacts, "mpm_download_contact_pairs.rigid_p_WB"));
}
static void download_pairs(State& s, Solver& solver) {
    const std::vector<mpm_collider_t> cols{a_collider()};
    MpmParticleContactPairs<float> p;
    // pairs counted on the device: the state object has not heard of a count
    solver.GenerateContactPairsOnDevice(&s, cols);
    CHECK((call("mpm_generate_contact_pairs").args == Args{1, 0}));
    solver.DownloadContactPairs(s, &p);
    check_pairs(p);
    // pairs counted on the host, and then more of them made through a copy of the state
    CHECK(solver.GenerateContactPairs(&s, cols) == N.contacts && s.num_contacts() == N.contacts);
    State alias = s;
    N.contacts += 3;
    solver.GenerateContactPairsOnDevice(&alias, cols);
    solver.DownloadContactPairs(s, &p);
    check_pairs(p);
    N.contacts -= 3;
}
static void run_coupled(State& s, Solver& solver) {
    const auto cols = items<mpm_collider_t>(3, 23);
    const int before = s.total_contact_iteration_count;
    const auto r = solver.RunCoupledSubsteps(&s, 4, 2.5e-4f, 5, 0.5f, 1e5f, 1e-3f, true, cols);
    CHECK(r.size() == 4);
    for (int k = 0; k < 4; ++k) CHECK(r[k].iterations == k + 1 && r[k].contacts == 100u + unsigned(k) && r[k].setup_reused == (k & 1));
    CHECK(s.total_contact_iteration_count == before + 10 && s.num_contacts() == 103);
    const stub::Call& c = call("mpm_run_coupled_substeps");
    CHECK((c.args == Args{4, 1, 3, 1}));
    mpm_coupled_params_t p;
    CHECK(c.bytes.size() == sizeof p + 3 * sizeof(mpm_collider_t));
    std::memcpy(&p, c.bytes.data(), sizeof p);
    CHECK(p.dt == 2.5e-4f && p.mpm_bc == 5 && p.friction_mu == 0.5f && p.stiffness == 1e5f && p.damping == 1e-3f &&
          p.exact_line_search == 1 && p.max_newton_iterations == 0);
    CHECK(std::memcmp(c.bytes.data() + sizeof p, cols.data(), 3 * sizeof(mpm_collider_t)) == 0);
    CHECK(solver.RunCoupledSubsteps(&s, 0, 2.5e-4f, -1, 0.f, 0.f, 0.f, false, {}).empty());
    CHECK(call("mpm_run_coupled_substeps").args[0] == 0 && call("mpm_run_coupled_substeps").args[2] == 0);
    CHECK(s.num_contacts() == 103);
}
static void body_force_to_host(State& s, Solver&) {
    s.ReallocateExternelBodies(5);
    CHECK(call("mpm_reallocate_external_bodies").args == Args{5} && s.num_external_bodies() == 5);
    s.ExternelBodyForceToHost();
    const auto& F = s.external_forces_host();
    CHECK(F.size() == 5 && holds(F.F_Bq_W_tau, 5, "mpm_external_body_force_to_host.tau") &&
          holds(F.F_Bq_W_f, 5, "mpm_external_body_force_to_host.f"));
}
static void finalize_forces(State& s, Solver&) {
    InitalizeExternalContactForces(&s, std::vector<Vec3<float>>{{1, 2, 3}, {4, 5, 6}});
    CHECK(call("mpm_reallocate_external_bodies").args == Args{2});
    s.external_forces_host().resize(1);   // (the call sizes the slots itself)
    FinalizeExternalContactForces(&s, 0.004f);
    const auto& F = s.external_forces_host();
    CHECK(holds(F.F_Bq_W_tau, 2, "mpm_finalize_external_contact_forces.tau") &&
          holds(F.F_Bq_W_f, 2, "mpm_finalize_external_contact_forces.f"));
    for (const auto& p : F.p_BoBq_B) CHECK(p[0] == 0 && p[1] == 0 && p[2] == 0);
    const float dt = 0.004f;
    const stub::Call& c = call("mpm_finalize_external_contact_forces");
    CHECK((c.args == Args{1, 1}) && c.bytes.size() == 4 && std::memcmp(c.bytes.data(), &dt, 4) == 0);
}
static void applied_forces(State& s, Solver&) {
    s.ReallocateExternelBodies(2);
    auto& F = s.external_forces_host();
    F.resize(2);
    for (size_t i = 0; i < 2; ++i)
        for (int d = 0; d < 3; ++d) {
            F.p_BoBq_B[i][d] = 1.f + float(3 * i + d);
            F.F_Bq_W_tau[i][d] = 10.f + float(3 * i + d);
            F.F_Bq_W_f[i][d] = 20.f + float(3 * i + d);
        }
    const auto R = items<std::array<float, 9>>(2, 29);
    std::vector<Vec3<float>> tau(2, Vec3<float>{1000.f, 1000.f, 1000.f}), f(2, Vec3<float>{2000.f, 2000.f, 2000.f});
    AddAppliedExternalSpatialForces(s, R, &tau, &f);
    for (size_t i = 0; i < 2; ++i)
        for (int d = 0; d < 3; ++d) {
            CHECK(tau[i][d] == 1000.f + (100.f + float(3 * i + d)));
            CHECK(f[i][d] == 2000.f + F.F_Bq_W_f[i][d]);
        }
    std::vector<unsigned char> want;
    append(&want, R);
    append(&want, F.p_BoBq_B);
    append(&want, F.F_Bq_W_tau);
    append(&want, F.F_Bq_W_f);
    CHECK(call("mpm_external_forces_at_body_origin").args == Args{2} && call("mpm_external_forces_at_body_origin").bytes == want);
    bool threw = false;
    try {
        tau.resize(1);
        AddAppliedExternalSpatialForces(s, R, &tau, &f);
    } catch (const std::logic_error&) {
        threw = true;
    }
    CHECK(threw);
}

struct Method {
    const char* name;
    std::function<void(State&, Solver&)> run;
};

#define FORCES(M, fn) {#M, [](State& s, Solver&) { vertex_forces(s, fn, &State::M); }}
#define TABLE(M, fn, count) {#M, [](State& s, Solver&) { table(fn, count, s.M()); }}
#define SETTER(M, R, fn, count) {#M, [](State& s, Solver&) { set_table<R>(fn, count, [&](const std::vector<R>& t) { s.M(t); }); }}

int main(int argc, char** argv) {
    const std::vector<Method> methods = {
        FORCES(BendingForces, "mpm_bending_forces"), FORCES(DampingForces, "mpm_damping_forces"),
        {"WeaveForces", weave_forces},
        FORCES(LinkForces, "mpm_link_forces"), FORCES(AnchorForces, "mpm_anchor_forces"),
        FORCES(PressureForces, "mpm_pressure_forces"), FORCES(ShellForces, "mpm_shell_forces"),
        FORCES(ShellDampingForces, "mpm_shell_damping_forces"),
        {"WeaveAxes", [](State& s, Solver&) { per_face(s, "mpm_weave_axes", 2, &State::WeaveAxes); }},
        {"WeaveStrain", [](State& s, Solver&) { per_face(s, "mpm_weave_strain", 3, &State::WeaveStrain); }},
        {"TearState", tear_state}, {"TearMeasure", tear_measure},
        {"FaceStrain", [](State& s, Solver&) { per_face(s, "mpm_face_strain", 4, &State::FaceStrain); }},
        {"ShellCutHinges", shell_cut_hinges}, {"ShellDampingPower", shell_damping_power}, {"ShellEnergy", shell_energy},
        TABLE(GetPins, "mpm_get_pins", N.pins), TABLE(GetGridBodies, "mpm_get_grid_bodies", N.grid_bodies),
        TABLE(GetForceFields, "mpm_get_force_fields", N.fields), TABLE(GetBending, "mpm_get_bending", N.cloths),
        TABLE(GetDamping, "mpm_get_damping", N.cloths), TABLE(GetWeave, "mpm_get_weave", N.cloths),
        TABLE(GetLinks, "mpm_get_links", N.links), TABLE(GetLinkLimits, "mpm_get_link_limits", N.links),
        TABLE(GetAnchors, "mpm_get_anchors", N.anchors), TABLE(GetPressure, "mpm_get_pressure", N.cloths),
        TABLE(PressureState, "mpm_pressure_state", N.cloths), TABLE(GetShellBending, "mpm_get_shell_bending", N.cloths),
        TABLE(GetShellDamping, "mpm_get_shell_damping", N.cloths), TABLE(GetCreases, "mpm_get_creases", N.cloths),
        TABLE(PressureVented, "mpm_pressure_vented", N.cloths),
        {"GetBodyContactMaterials", [](State& s, Solver& solver) {
             table("mpm_get_body_contact_materials", N.materials, solver.GetBodyContactMaterials(s));
         }},
        {"GetTearing", tearing}, {"LinkEnergy", link_energy}, {"LinkBreakState", link_break_state},
        {"LinkBreakMeasure", link_break_measure}, {"AnchorState", anchor_state}, {"CreaseState", crease_state},
        {"CreaseMeasure", crease_measure}, {"WeaveEnergy", weave_energy}, {"Measure", measure},
        {"CalcKineticEnergy", kinetic}, {"CalcPotentialEnergy", potential}, {"GetRestShape", rest_shape},
        {"DumpCpuState", dump_cpu_state}, {"SyncParticleStateToCpu", sync_particles},
        {"ColliderSignedDistance", collider_distance}, {"SdfColliderSignedDistance", sdf_collider_distance},
        {"DownloadContactPairs", download_pairs}, {"RunCoupledSubsteps", run_coupled},
        {"ExternelBodyForceToHost", body_force_to_host}, {"FinalizeExternalContactForces", finalize_forces},
        {"AddAppliedExternalSpatialForces", applied_forces},
        // the setters: null for an empty optional table, the count and the bytes
        {"SetWeave", set_weave}, {"SetShellBending", set_shell_bending}, {"SetCreaseState", set_crease_state},
        {"SetRestShape", set_rest_shape}, {"SetTornFaces", set_torn_faces}, {"SetBrokenLinks", set_broken_links},
        SETTER(SetBodyMotions, mpm_body_motion_t, "mpm_set_body_motions", N.bodies),
        SETTER(SetPins, mpm_pin_t, "mpm_set_pins", N.pins),
        SETTER(SetGridBodies, mpm_grid_body_t, "mpm_set_grid_bodies", N.grid_bodies),
        SETTER(SetForceFields, mpm_force_field_t, "mpm_set_force_fields", N.fields),
        SETTER(SetBending, float, "mpm_set_bending", N.cloths),
        SETTER(SetDamping, mpm_cloth_damping_t, "mpm_set_damping", N.cloths),
        SETTER(SetLinks, mpm_link_t, "mpm_set_links", N.links),
        SETTER(SetLinkLimits, float, "mpm_set_link_limits", N.links),
        SETTER(SetAnchors, mpm_anchor_t, "mpm_set_anchors", N.anchors),
        SETTER(SetPressure, mpm_cloth_pressure_t, "mpm_set_pressure", N.cloths),
        SETTER(SetShellDamping, mpm_cloth_shell_damping_t, "mpm_set_shell_damping", N.cloths),
        SETTER(SetCreases, mpm_cloth_crease_t, "mpm_set_creases", N.cloths),
        {"SetBodyContactMaterials", [](State& s, Solver& solver) {
             set_table<mpm_contact_material_t>("mpm_set_body_contact_materials", N.materials,
                                               [&](const std::vector<mpm_contact_material_t>& t) { solver.SetBodyContactMaterials(&s, t); });
         }},
        {"SetSdfColliders", [](State& s, Solver& solver) {
             set_table<mpm_sdf_collider_t>("mpm_set_sdf_colliders", 3,
                                           [&](const std::vector<mpm_sdf_collider_t>& t) { solver.SetSdfColliders(&s, t); });
         }},
    };
    std::set<std::string> only(argv + 1, argv + argc);
    State s(6);
    Solver solver;
    for (const Method& m : methods) {
        if (!only.empty() && !only.count(m.name)) continue;
        current = m.name;
        stub::N = stub::Counts();
        try {
            m.run(s, solver);
        } catch (const std::exception& e) {
            std::fprintf(stderr, "FAILED %s: threw %s\n", current, e.what());
            return 1;
        }
        std::printf("ok %s\n", m.name);
        std::fflush(stdout);
    }
    return 0;
}
