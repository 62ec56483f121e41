// Replays a script of calls through the C++ facade (include/gpu_mpm.hpp) and writes every returned value to a file, for
// tests/test_facade_gpu.py: tests/facade_scene.py runs the same script through the ctypes binding on a twin engine, and in
// deterministic mode the two must agree to the bit, since both marshal into one C ABI.
//
//   facade_replay replay|refusals|sizes|statics <scene file> <result file>
//
// Both files are sequences of named blocks: a 64-byte name, the item size and the count as uint64, the raw bytes.  Tables
// arrive as the raw bytes of the binding's ctypes structures and numpy records and are read into std::vector<mpm_link_t>
// and the like: an item size that differs from the header's struct stops the program.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <map>
#include <string>

#include "mpm_driver.hpp"

using namespace drake::multibody::gmpm;
using State = GpuMpmState<float>;
using Solver = GpuMpmSolver<float>;

namespace {

[[noreturn]] void die(const std::string& what) {
    std::fprintf(stderr, "facade_replay: %s\n", what.c_str());
    std::exit(1);
}

struct Block {
    uint64_t item = 0, count = 0;
    std::string bytes;
};
std::map<std::string, Block> scene;
std::ofstream result;
std::string result_path;

void read_scene(const char* path) {
    std::ifstream in(path, std::ios::binary);
    if (!in) die(std::string("cannot read ") + path);
    char name[64];
    while (in.read(name, 64)) {
        Block b;
        in.read(reinterpret_cast<char*>(&b.item), 8);
        in.read(reinterpret_cast<char*>(&b.count), 8);
        b.bytes.resize(b.item * b.count);
        in.read(&b.bytes[0], (std::streamsize)b.bytes.size());
        if (!in) die("truncated scene file");
        scene[std::string(name, strnlen(name, 64))] = b;
    }
}
template <class R>
std::vector<R> get(const std::string& name) {
    const auto it = scene.find(name);
    if (it == scene.end()) die("no block " + name);
    const Block& b = it->second;
    if (b.count && b.item != sizeof(R))
        die("block " + name + ": items of " + std::to_string(b.item) + " bytes, the header's type has " + std::to_string(sizeof(R)));
    std::vector<R> v(b.count);
    if (b.count) std::memcpy(v.data(), b.bytes.data(), b.bytes.size());
    return v;
}
void put_bytes(const std::string& name, uint64_t item, uint64_t count, const void* data) {
    char head[64] = {0};
    if (name.size() >= 64) die("name too long: " + name);
    std::memcpy(head, name.data(), name.size());
    result.write(head, 64);
    result.write(reinterpret_cast<const char*>(&item), 8);
    result.write(reinterpret_cast<const char*>(&count), 8);
    result.write(reinterpret_cast<const char*>(data), (std::streamsize)(item * count));
}
template <class R>
void put(const std::string& name, const std::vector<R>& v) { put_bytes(name, sizeof(R), v.size(), v.data()); }
template <class R>
void put1(const std::string& name, const R& value) { put_bytes(name, sizeof(R), 1, &value); }
void done(const std::string& name) { put1<uint32_t>(name, 1u); }
std::vector<Vec3<float>> vec3s(const std::vector<float>& f) {
    std::vector<Vec3<float>> v(f.size() / 3);
    if (!f.empty()) std::memcpy(v.data(), f.data(), v.size() * sizeof(Vec3<float>));
    return v;
}

constexpr int N_PHASES = 24, N_COUPLED = 16, BC = MPM_BC_BODIES;

State create() {
    const auto material = get<mpm_material_t>("material");
    State s(6, &material.at(0));
    // before the cloths: reproducible bits need the canonical order inside a cell from Finalize's own first sort on (a
    // later switch keeps sorting by the previous slot, which the arrival of that first sort's atomics decided)
    s.SetDeterministic(true);
    const uint32_t n = get<uint32_t>("n_cloths").at(0);
    for (uint32_t c = 0; c < n; ++c) {
        const std::string k = std::to_string(c);
        const auto pos = vec3s(get<float>("pos" + k)), vel = vec3s(get<float>("vel" + k));
        const auto idx = get<int>("idx" + k);
        const auto m = get<mpm_cloth_material_t>("cmat" + k);
        if (m.empty()) s.AddQRCloth(pos, vel, idx); else s.AddQRCloth(pos, vel, idx, m[0]);
    }
    return s;
}
State create_logged(Solver& solver) {
    State s = create();
    done("AddQRCloth");
    put1<uint64_t>("n_cloths", s.n_cloths());
    std::vector<mpm_cloth_material_t> mats;
    for (size_t c = 0; c < s.n_cloths(); ++c) mats.push_back(s.cloth_material(c));
    put("cloth_material", mats);
    done("SetDeterministic");
    s.Finalize(); done("Finalize");
    put("counts", std::vector<uint64_t>{s.n_verts(), s.n_faces(), s.n_particles()});
    solver.SetFastMath(&s, false); done("SetFastMath");
    s.ReallocateExternelBodies(3); done("ReallocateExternelBodies");
    return s;
}
// the same without a record, for the modes that start from a bare engine
State create_quiet(Solver& solver) {
    State s = create();
    s.Finalize();
    solver.SetFastMath(&s, false);
    s.ReallocateExternelBodies(3);
    return s;
}

void getters(State& s, Solver& solver, const std::string& tag) {
    put("GetPins" + tag, s.GetPins());
    put("GetGridBodies" + tag, s.GetGridBodies());
    put("GetForceFields" + tag, s.GetForceFields());
    put("GetBending" + tag, s.GetBending());
    put("GetDamping" + tag, s.GetDamping());
    put("GetWeave" + tag, s.GetWeave());
    put("GetTearing" + tag, s.GetTearing());
    put1<uint32_t>("GetTearCoupling" + tag, s.GetTearCoupling());
    bool is_set = false;
    put("GetRestShape" + tag, s.GetRestShape(&is_set));
    put1<uint32_t>("GetRestShape.is_set" + tag, is_set ? 1u : 0u);
    put("GetLinks" + tag, s.GetLinks());
    put("GetLinkLimits" + tag, s.GetLinkLimits());
    put("GetAnchors" + tag, s.GetAnchors());
    put("GetPressure" + tag, s.GetPressure());
    put("GetShellBending" + tag, s.GetShellBending());
    put1<uint64_t>("ShellHingeCount" + tag, s.ShellHingeCount());
    put("GetShellDamping" + tag, s.GetShellDamping());
    put("GetCreases" + tag, s.GetCreases());
    put("GetBodyContactMaterials" + tag, solver.GetBodyContactMaterials(s));
}
void guards(State& s, const std::string& tag) {
    put1("BendingMaxStableDt" + tag, s.BendingMaxStableDt());
    put1("DampingMaxStableDt" + tag, s.DampingMaxStableDt());
    put1("WeaveMaxStableDt" + tag, s.WeaveMaxStableDt());
    put1("LinksMaxStableDt" + tag, s.LinksMaxStableDt());
    put1("AnchorsMaxStableDt" + tag, s.AnchorsMaxStableDt());
    put1("ShellMaxStableDt" + tag, s.ShellMaxStableDt());
}
void states(State& s, const std::string& tag) {
    std::vector<uint32_t> counts;
    put("TearState" + tag, s.TearState(s.n_faces(), &counts));
    put("TearState.counts" + tag, counts);
    uint32_t count = 0;
    put("LinkBreakState" + tag, s.LinkBreakState(&count));
    put1("LinkBreakState.count" + tag, count);
    put("CreaseState" + tag, s.CreaseState(&counts));
    put("CreaseState.counts" + tag, counts);
    put("PressureVented" + tag, s.PressureVented());
    put("ShellCutHinges" + tag, s.ShellCutHinges(s.ShellHingeCount(), &counts));
    put("ShellCutHinges.counts" + tag, counts);
}
void evaluators(State& s, const std::string& tag) {
    const size_t nv = s.n_verts(), nf = s.n_faces(), nc = s.n_cloths();
    guards(s, tag);
    put("BendingForces" + tag, s.BendingForces(nv));
    put("DampingForces" + tag, s.DampingForces(nv));
    put("WeaveAxes" + tag, s.WeaveAxes(nf));
    std::vector<float> records;
    put("WeaveForces" + tag, s.WeaveForces(nv, &records));
    put("WeaveForces.records" + tag, records);
    put("WeaveStrain" + tag, s.WeaveStrain(nf));
    double total = 0;
    put("WeaveEnergy" + tag, s.WeaveEnergy(&total));
    put1("WeaveEnergy.total" + tag, total);
    std::vector<uint8_t> verdicts;
    put("TearMeasure" + tag, s.TearMeasure(nf, &verdicts));
    put("TearMeasure.would_fail" + tag, verdicts);
    put("LinkForces" + tag, s.LinkForces(nv));
    std::vector<float> lengths, points;
    put1("LinkEnergy" + tag, s.LinkEnergy(&lengths));
    put("LinkEnergy.lengths" + tag, lengths);
    put("LinkBreakMeasure" + tag, s.LinkBreakMeasure(&verdicts));
    put("LinkBreakMeasure.would_break" + tag, verdicts);
    put("AnchorForces" + tag, s.AnchorForces(nv));
    double quantum = 0;
    put1("AnchorState" + tag, s.AnchorState(&lengths, &points, &quantum));
    put("AnchorState.lengths" + tag, lengths);
    put("AnchorState.points" + tag, points);
    put1("AnchorState.impulse_quantum" + tag, quantum);
    put("PressureForces" + tag, s.PressureForces(nv));
    put("PressureState" + tag, s.PressureState());
    put("ShellForces" + tag, s.ShellForces(nv));
    put("ShellEnergy" + tag, s.ShellEnergy(nc));
    put("ShellDampingForces" + tag, s.ShellDampingForces(nv));
    put("ShellDampingPower" + tag, s.ShellDampingPower(nc));
    std::vector<float> psi, dpsi;
    put("CreaseMeasure" + tag, s.CreaseMeasure(&psi, &dpsi));
    put("CreaseMeasure.psi" + tag, psi);
    put("CreaseMeasure.dpsi" + tag, dpsi);
    mpm_cloth_measure_t sum;
    put("Measure" + tag, s.Measure(&sum));
    put1("Measure.total" + tag, sum);
    put1("CalcKineticEnergy" + tag, s.CalcKineticEnergy());
    put1("CalcPotentialEnergy" + tag, s.CalcPotentialEnergy());
    put("FaceStrain" + tag, s.FaceStrain(nf));
    states(s, tag);
}
void set_tables(State& s, Solver& solver) {
    s.SetRestShape(get<float>("rest_shape")); done("SetRestShape");
    s.SetBodyMotions(get<mpm_body_motion_t>("body_motions")); done("SetBodyMotions");
    s.SetTearCoupling(get<uint32_t>("tear_coupling").at(0)); done("SetTearCoupling");
    s.SetBending(get<float>("bending")); done("SetBending");
    s.SetDamping(get<mpm_cloth_damping_t>("damping")); done("SetDamping");
    s.SetWeave(get<mpm_cloth_weave_t>("weave"), get<float>("weave_dirs")); done("SetWeave");
    s.SetLinks(get<mpm_link_t>("links")); done("SetLinks");
    s.SetLinkLimits(get<float>("link_limits")); done("SetLinkLimits");
    s.SetTearing(get<float>("tearing")); done("SetTearing");
    s.SetPressure(get<mpm_cloth_pressure_t>("pressure")); done("SetPressure");
    s.SetShellBending(get<mpm_cloth_shell_t>("shell"), get<float>("shell_rest")); done("SetShellBending");
    s.SetShellDamping(get<mpm_cloth_shell_damping_t>("shell_damping")); done("SetShellDamping");
    s.SetCreases(get<mpm_cloth_crease_t>("creases")); done("SetCreases");
    s.SetAnchors(get<mpm_anchor_t>("anchors")); done("SetAnchors");
    s.SetPins(get<mpm_pin_t>("pins")); done("SetPins");
    s.SetForceFields(get<mpm_force_field_t>("force_fields")); done("SetForceFields");
    s.SetGridBodies(get<mpm_grid_body_t>("grid_bodies")); done("SetGridBodies");
    solver.SetBodyContactMaterials(&s, get<mpm_contact_material_t>("contact_materials")); done("SetBodyContactMaterials");
}
void clear_tables(State& s, Solver& solver) {
    s.SetCreases({}); done("SetCreases@clear");
    s.SetShellDamping({}); done("SetShellDamping@clear");
    s.SetShellBending({}); done("SetShellBending@clear");
    s.SetAnchors({}); done("SetAnchors@clear");
    s.SetPins({}); done("SetPins@clear");
    s.SetLinkLimits({}); done("SetLinkLimits@clear");
    s.SetLinks({}); done("SetLinks@clear");
    s.SetPressure({}); done("SetPressure@clear");
    s.SetWeave({}); done("SetWeave@clear");
    s.SetDamping({}); done("SetDamping@clear");
    s.SetBending({}); done("SetBending@clear");
    s.SetTearing(std::vector<float>(s.n_cloths(), 0.f)); done("SetTearing@clear");   // (mpm_set_tearing has no empty form)
    s.SetTornFaces(std::vector<uint8_t>(s.n_faces(), 0)); done("SetTornFaces@clear");
    s.SetTearCoupling(0); done("SetTearCoupling@clear");
    s.SetForceFields({}); done("SetForceFields@clear");
    s.SetGridBodies({}); done("SetGridBodies@clear");
    solver.SetBodyContactMaterials(&s, {}); done("SetBodyContactMaterials@clear");
    solver.SetSdfColliders(&s, {}); done("SetSdfColliders@clear");
    s.ClearRestShape(); done("ClearRestShape");
}

int replay() {
    Solver solver;
    State s = create_logged(solver);
    const float dt = get<float>("dt").at(0);
    const auto contact = get<float>("contact");
    const float mu = contact.at(0), k_ct = contact.at(1), d_ct = contact.at(2);
    const auto floor = get<mpm_collider_t>("floor");
    InitalizeExternalContactForces(&s, std::vector<Vec3<float>>(3, Vec3<float>{0, 0, 0})); done("InitalizeExternalContactForces");
    set_tables(s, solver);
    getters(s, solver, "@set");
    evaluators(s, "@0");
    // 24 substeps of the five solver calls
    s.SetBodyMotions(get<mpm_body_motion_t>("body_motions")); done("SetBodyMotions@run");
    for (int k = 0; k < N_PHASES; ++k) {
        solver.RebuildMapping(&s, false);
        solver.CalcFemStateAndForce(&s, dt);
        solver.ParticleToGrid(&s, dt);
        solver.UpdateGrid(&s, BC);
        solver.GridToParticle(&s, dt);
    }
    solver.GpuSync(&s); done("GpuSync");
    solver.GpuSync(); done("GpuSync.device");
    put1("grid_touched_cnt_host", s.grid_touched_cnt_host());
    states(s, "@phases");
    // a batch against the floor
    put("RunCoupledSubsteps", solver.RunCoupledSubsteps(&s, N_COUPLED, dt, BC, mu, k_ct, d_ct, false, floor));
    evaluators(s, "@1");
    const auto dumped = s.DumpCpuState();
    put("DumpCpuState.pos", std::get<0>(dumped));
    put("DumpCpuState.indices", std::get<1>(dumped));
    {
        const std::string obj = result_path + ".obj";
        solver.Dump(s, obj);
        std::ifstream in(obj, std::ios::binary);
        const std::string text((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        put_bytes("Dump", 1, text.size(), text.data());
        std::remove(obj.c_str());
    }
    solver.SyncParticleStateToCpu(&s);
    put("SyncParticleStateToCpu", s.positions_host());
    s.ExternelBodyForceToHost();
    put("ExternelBodyForceToHost.tau", s.external_forces_host().F_Bq_W_tau);
    put("ExternelBodyForceToHost.f", s.external_forces_host().F_Bq_W_f);
    // the seven calls, pairs on the device, then pairs through the host
    for (int host = 0; host < 2; ++host) {
        solver.RebuildMapping(&s, false);
        solver.CalcFemStateAndForce(&s, dt);
        solver.ParticleToGrid(&s, dt);
        solver.UpdateGrid(&s, BC);
        if (!host) {
            solver.GenerateContactPairsOnDevice(&s, floor);
            put1<uint64_t>("ContactPairCount", solver.ContactPairCount(&s));
        } else {
            put1<uint64_t>("GenerateContactPairs", solver.GenerateContactPairs(&s, floor));
            if (s.num_contacts() == 0) die("no contact pairs where the run ends: the host leg would test nothing");
            MpmParticleContactPairs<float> pairs;
            solver.DownloadContactPairs(s, &pairs);
            put("DownloadContactPairs.particle", pairs.particle_in_contact_index);
            put("DownloadContactPairs.body", pairs.non_mpm_id);
            put("DownloadContactPairs.dist", pairs.penetration_distance);
            put("DownloadContactPairs.normal", pairs.normal);
            put("DownloadContactPairs.position", pairs.particle_in_contact_position);
            put("DownloadContactPairs.rigid_v", pairs.rigid_v);
            put("DownloadContactPairs.rigid_p_WB", pairs.rigid_p_WB);
            s.ReallocateContacts(pairs.size());
            solver.CopyContactPairs(&s, pairs); done("CopyContactPairs");
        }
        solver.UpdateContact(&s, 0, host, dt, mu, k_ct, d_ct, false, false);
        solver.GridToParticle(&s, dt);
        done(host ? "UpdateContact.host" : "UpdateContact.device");
    }
    solver.GpuSync(&s);
    put1<int32_t>("total_contact_iteration_count", s.total_contact_iteration_count);
    const float plant_dt = float(double(dt) * (N_PHASES + N_COUPLED + 2));
    FinalizeExternalContactForces(&s, plant_dt);
    put("FinalizeExternalContactForces.tau", s.external_forces_host().F_Bq_W_tau);
    put("FinalizeExternalContactForces.f", s.external_forces_host().F_Bq_W_f);
    {
        const size_t nb = s.num_external_bodies();
        std::vector<std::array<float, 9>> R(nb, std::array<float, 9>{1, 0, 0, 0, 1, 0, 0, 0, 1});
        std::vector<Vec3<float>> tau(nb, Vec3<float>{1, 1, 1}), f(nb, Vec3<float>{2, 2, 2});
        AddAppliedExternalSpatialForces(s, R, &tau, &f);
        put("AddAppliedExternalSpatialForces.tau", tau);
        put("AddAppliedExternalSpatialForces.f", f);
    }
    // signed distances, a mesh collider, a fixed constraint
    auto points = get<float>("query_points");
    std::vector<float> phi, grad;
    solver.ColliderSignedDistance(s, get<mpm_collider_t>("query_collider").at(0), points, &phi, &grad);
    put("ColliderSignedDistance.phi", phi);
    put("ColliderSignedDistance.grad", grad);
    const uint32_t shape = solver.SdfShapeFromMesh(&s, get<float>("mesh_verts"), get<int32_t>("mesh_tris"), 0.01f);
    put1("SdfShapeFromMesh", shape);
    mpm_sdf_collider_t mesh{};
    mesh.shape = shape;
    mesh.body = 2;
    const auto pose = get<float>("mesh_pose");
    for (int d = 0; d < 3; ++d) {
        mesh.p_WB[d] = pose.at(d);
        mesh.R_WB[4 * d] = 1.f;
    }
    solver.SetSdfColliders(&s, {mesh}); done("SetSdfColliders");
    for (float& p : points) p += 0.3f;
    solver.SdfColliderSignedDistance(s, mesh, points, &phi, &grad);
    put("SdfColliderSignedDistance.phi", phi);
    put("SdfColliderSignedDistance.grad", grad);
    {
        const auto now = std::get<0>(s.DumpCpuState());
        mpm_collider_t ball{};
        ball.kind = MPM_COLLIDER_SPHERE;
        for (int d = 0; d < 3; ++d) {
            ball.p_WB[d] = now.at(5)[d];
            ball.R_WB[4 * d] = 1.f;
        }
        ball.dims[0] = 1e-3f;
        put1<uint64_t>("AddFixedConstraint", s.AddFixedConstraint(0, ball, Vec3<float>{0, 0, 0}, std::array<float, 9>{1, 0, 0, 0, 1, 0, 0, 0, 1}));
    }
    getters(s, solver, "@1");
    // scissors and restore, the state read after each
    auto torn = s.TearState(s.n_faces());
    torn.at(get<uint32_t>("ico_face").at(0)) = 1;
    s.SetTornFaces(torn); done("SetTornFaces");
    states(s, "@torn");
    auto broken = s.LinkBreakState();
    broken.back() = 1;
    for (int k = 0; k < 8; ++k) broken.at(k) = 0;
    s.SetBrokenLinks(broken); done("SetBrokenLinks");
    states(s, "@broken");
    const auto psibar = s.CreaseState();
    s.SetCreaseState({}); done("SetCreaseState@iron");
    states(s, "@ironed");
    s.SetCreaseState(psibar); done("SetCreaseState");
    states(s, "@creased");
    evaluators(s, "@2");
    clear_tables(s, solver);
    getters(s, solver, "@clear");
    guards(s, "@clear");
    s.Destroy(); done("Destroy");
    return 0;
}

// a call the C ABI refuses: std::runtime_error whose what() goes to the result
template <class F>
void refused(const std::string& name, F call) {
    try {
        call();
    } catch (const std::runtime_error& e) {
        const std::string what = e.what();
        put_bytes(name, 1, what.size(), what.data());
        return;
    }
    die(name + ": the call was not refused");
}
int refusals() {
    Solver solver;
    State s = create_quiet(solver);
    const float dt = get<float>("dt").at(0);
    refused("refused.SetCreases", [&] { s.SetCreases(get<mpm_cloth_crease_t>("creases")); });     // before SetShellBending
    put("GetCreases", s.GetCreases());
    s.SetBending(get<float>("bending"));
    const float guard = s.BendingMaxStableDt();
    solver.RebuildMapping(&s, false);
    solver.CalcFemStateAndForce(&s, dt);
    refused("refused.ParticleToGrid", [&] { solver.ParticleToGrid(&s, 4.f * guard); });           // dt above a guard
    solver.ParticleToGrid(&s, dt);
    solver.UpdateGrid(&s);
    solver.GridToParticle(&s, dt);
    solver.GpuSync(&s);
    put("DumpCpuState.pos", std::get<0>(s.DumpCpuState()));
    refused("refused.SetRestShape", [&] { s.SetRestShape(get<float>("rest_shape")); });           // bending caches the rest shape
    bool is_set = true;
    put("GetRestShape", s.GetRestShape(&is_set));
    put1<uint32_t>("GetRestShape.is_set", is_set ? 1u : 0u);
    s.Destroy();
    return 0;
}

// every evaluator with a size that is not the engine's: std::invalid_argument, and the engine as usable as before
int sizes() {
    Solver solver;
    State s = create_quiet(solver);
    s.SetBending(get<float>("bending"));
    const size_t nv = s.n_verts(), nf = s.n_faces(), nc = s.n_cloths(), nh = s.ShellHingeCount();
    uint32_t thrown = 0;
    auto wrong = [&](const char* name, auto call) {
        try {
            call();
        } catch (const std::invalid_argument&) {
            ++thrown;
            return;
        }
        die(std::string(name) + ": a wrong size was accepted");
    };
    std::vector<float> records;
    wrong("BendingForces", [&] { s.BendingForces(nv + 1); });
    wrong("DampingForces", [&] { s.DampingForces(nv - 1); });
    wrong("WeaveForces", [&] { s.WeaveForces(nf); });
    wrong("WeaveForces records", [&] { s.WeaveForces(nv, &records, nv); });
    wrong("LinkForces", [&] { s.LinkForces(0); });
    wrong("AnchorForces", [&] { s.AnchorForces(3 * nv); });
    wrong("PressureForces", [&] { s.PressureForces(nf); });
    wrong("ShellForces", [&] { s.ShellForces(nv + 7); });
    wrong("ShellDampingForces", [&] { s.ShellDampingForces(nc); });
    wrong("WeaveAxes", [&] { s.WeaveAxes(2 * nf); });
    wrong("WeaveStrain", [&] { s.WeaveStrain(nv); });
    wrong("TearState", [&] { s.TearState(nf - 1); });
    wrong("TearMeasure", [&] { s.TearMeasure(nf + 1); });
    wrong("FaceStrain", [&] { s.FaceStrain(nv); });
    wrong("ShellCutHinges", [&] { s.ShellCutHinges(nh + 1); });
    wrong("ShellDampingPower", [&] { s.ShellDampingPower(nc + 1); });
    wrong("ShellEnergy", [&] { s.ShellEnergy(nv); });
    put1("wrong_sizes", thrown);
    put("BendingForces", s.BendingForces(nv));
    put("FaceStrain", s.FaceStrain(nf));
    s.Destroy();
    return 0;
}

// the host-only statics: no engine
int statics() {
    const auto x9 = get<float>("st_x9");
    put("DampingFaceRecords", State::DampingFaceRecords(x9.size() / 9, get<float>("st_dminv3").data(), get<float>("st_vol").data(),
                                                        get<float>("st_mu").data(), get<float>("st_lambda").data(),
                                                        get<float>("st_beta").data(), x9.data(), get<float>("st_v9").data()));
    std::vector<float> f(3), y(3), v_Q(3);
    State::LinkForce(get<mpm_link_t>("st_link").at(0), get<float>("st_xa").data(), get<float>("st_xb").data(),
                     get<float>("st_va").data(), get<float>("st_vb").data(), f.data());
    put("LinkForce", f);
    State::AnchorPoint(get<mpm_body_motion_t>("st_motion").at(0), get<double>("st_t").at(0), get<float>("st_p_BQ").data(), y.data(),
                       v_Q.data());
    put("AnchorPoint.y", y);
    put("AnchorPoint.v_Q", v_Q);
    for (const char* k : {"closed", "open"}) {
        std::vector<int32_t> edge(2, 0);
        const bool ok = State::MeshIsClosed(get<int32_t>(std::string("st_") + k), 4, edge.data());
        put1<uint32_t>(std::string("MeshIsClosed.") + k, ok ? 1u : 0u);
        put(std::string("MeshIsClosed.") + k + ".edge", edge);
    }
    const auto x_b = get<float>("st_x_b");
    State::PressureVertexForce(get<float>("st_g").at(0), get<float>("st_x_own").data(), x_b.size() / 3, x_b.data(),
                               get<float>("st_x_c").data(), f.data());
    put("PressureVertexForce", f);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 4) die("usage: facade_replay replay|refusals|sizes|statics <scene file> <result file>");
    read_scene(argv[2]);
    result_path = argv[3];
    result.open(argv[3], std::ios::binary);
    if (!result) die(std::string("cannot write ") + argv[3]);
    const std::string mode = argv[1];
    int rc = 2;
    try {
        rc = mode == "replay" ? replay() : mode == "refusals" ? refusals() : mode == "sizes" ? sizes() : mode == "statics" ? statics() : 2;
    } catch (const std::exception& e) {
        die(std::string("exception: ") + e.what());
    }
    result.close();
    if (!result) die("the result file could not be written");
    if (rc == 0) std::printf("facade_replay %s ok\n", mode.c_str());
    return rc;
}
