// A stub of the C ABI (include/mpm_hip.h) for tests/facade_sizes.cc: only the entry points the facade methods under test
// reference, nothing of the engine.  The engine is its counts (facade_stub.h).  Every output pointer that is not null is
// written over exactly the extent mpm_hip.h documents for it, with a pattern that depends on (entry point, argument, byte
// offset); every input table is copied into the log over exactly the extent mpm_hip.h says the engine reads.  Under the
// address sanitizer a buffer the facade made too small is therefore a report, one made too large a failed pattern check.
#include <cstring>
#include <initializer_list>

#include "facade_stub.h"
#include "mpm_hip.h"

namespace stub {
Counts N;
std::vector<Call> LOG;
}  // namespace stub

using stub::N;

namespace {

int engine_word;   // what a handle points at

stub::Call& log(const char* fn, std::initializer_list<long long> args = {}) {
    stub::LOG.push_back(stub::Call{fn, std::vector<long long>(args), {}});
    return stub::LOG.back();
}
template <class R>
void reads(stub::Call& c, const R* p, size_t n) {
    if (!p) return;
    const unsigned char* b = reinterpret_cast<const unsigned char*>(p);
    c.bytes.insert(c.bytes.end(), b, b + n * sizeof(R));
}
template <class R>
void fill(R* p, size_t n, const char* what) {
    if (!p) return;
    unsigned char* b = reinterpret_cast<unsigned char*>(p);
    for (size_t k = 0; k < n * sizeof(R); ++k) b[k] = stub::pattern(what, k);
}
// the two-call getters: the count when capacity == 0, and no more than capacity records
template <class R>
int getter(const char* fn, size_t count, R* out, size_t capacity, size_t* n_out) {
    log(fn, {out != nullptr, (long long)capacity, n_out != nullptr});
    if (capacity && !out) return MPM_ERR_INVALID;
    if (capacity) fill(out, count < capacity ? count : capacity, fn);
    if (n_out) *n_out = count;
    return 0;
}
template <class R>
int setter(const char* fn, size_t n, const R* p) {
    reads(log(fn, {(long long)n, p != nullptr}), p, n);
    return 0;
}
int vertex_forces(const char* fn, float* f_out) {
    log(fn, {f_out != nullptr});
    fill(f_out, 3 * N.verts, fn);
    return 0;
}
int guard(const char* fn, float* dt_out) {
    log(fn);
    *dt_out = stub::GUARD_DT;
    return 0;
}

}  // namespace

extern "C" {

const char* mpm_last_error(void) { return "stub"; }
int mpm_create(int domain_bits, const mpm_material_t* material, int device, mpm_handle_t* out) {
    log("mpm_create", {domain_bits, material != nullptr, device});
    *out = reinterpret_cast<mpm_handle_t>(&engine_word);
    return 0;
}
int mpm_destroy(mpm_handle_t) { return 0; }
int mpm_counts(mpm_handle_t, size_t* n_verts, size_t* n_faces, size_t* n_particles) {
    if (n_verts) *n_verts = N.verts;
    if (n_faces) *n_faces = N.faces;
    if (n_particles) *n_particles = N.particles();
    return 0;
}
int mpm_cloth_count(mpm_handle_t, size_t* n_out) {
    *n_out = N.cloths;
    return 0;
}
int mpm_dump_cpu_state(mpm_handle_t, float* pos_out, int32_t* indices_out) {
    log("mpm_dump_cpu_state", {pos_out != nullptr, indices_out != nullptr});
    fill(pos_out, 3 * N.verts, "mpm_dump_cpu_state.pos");
    fill(indices_out, 3 * N.faces, "mpm_dump_cpu_state.indices");
    return 0;
}
int mpm_sync_particle_state_to_cpu(mpm_handle_t, float* pos_out) {
    log("mpm_sync_particle_state_to_cpu", {pos_out != nullptr});
    fill(pos_out, 3 * N.particles(), "mpm_sync_particle_state_to_cpu");
    return 0;
}
int mpm_reallocate_external_bodies(mpm_handle_t, size_t n_bodies) {
    log("mpm_reallocate_external_bodies", {(long long)n_bodies});
    N.bodies = n_bodies;
    return 0;
}
int mpm_external_body_force_to_host(mpm_handle_t, float* tau_out, float* f_out) {
    log("mpm_external_body_force_to_host", {tau_out != nullptr, f_out != nullptr});
    fill(tau_out, 3 * N.bodies, "mpm_external_body_force_to_host.tau");
    fill(f_out, 3 * N.bodies, "mpm_external_body_force_to_host.f");
    return 0;
}
int mpm_finalize_external_contact_forces(mpm_handle_t, float dt, float* tau_out, float* f_out) {
    reads(log("mpm_finalize_external_contact_forces", {tau_out != nullptr, f_out != nullptr}), &dt, 1);
    fill(tau_out, 3 * N.bodies, "mpm_finalize_external_contact_forces.tau");
    fill(f_out, 3 * N.bodies, "mpm_finalize_external_contact_forces.f");
    return 0;
}
int mpm_external_forces_at_body_origin(size_t n_bodies, const float* R_WB, const float* p_BoBq_B, const float* tau, const float* f,
                                       float* tau_Bo_out) {
    stub::Call& c = log("mpm_external_forces_at_body_origin", {(long long)n_bodies});
    reads(c, R_WB, 9 * n_bodies);
    reads(c, p_BoBq_B, 3 * n_bodies);
    reads(c, tau, 3 * n_bodies);
    reads(c, f, 3 * n_bodies);
    for (size_t k = 0; k < 3 * n_bodies; ++k) tau_Bo_out[k] = 100.f + float(k);   // (the facade adds these: numbers)
    return 0;
}

// ---- the tables: setters log (count, pointer, bytes), getters follow the two-call contract -------------------------------
int mpm_set_body_motions(mpm_handle_t, size_t n, const mpm_body_motion_t* p) { return setter("mpm_set_body_motions", n, p); }
int mpm_set_pins(mpm_handle_t, size_t n, const mpm_pin_t* p) { return setter("mpm_set_pins", n, p); }
int mpm_get_pins(mpm_handle_t, mpm_pin_t* out, size_t cap, size_t* n_out) { return getter("mpm_get_pins", N.pins, out, cap, n_out); }
int mpm_set_grid_bodies(mpm_handle_t, size_t n, const mpm_grid_body_t* p) { return setter("mpm_set_grid_bodies", n, p); }
int mpm_get_grid_bodies(mpm_handle_t, mpm_grid_body_t* out, size_t cap, size_t* n_out) {
    return getter("mpm_get_grid_bodies", N.grid_bodies, out, cap, n_out);
}
int mpm_set_force_fields(mpm_handle_t, size_t n, const mpm_force_field_t* p) { return setter("mpm_set_force_fields", n, p); }
int mpm_get_force_fields(mpm_handle_t, mpm_force_field_t* out, size_t cap, size_t* n_out) {
    return getter("mpm_get_force_fields", N.fields, out, cap, n_out);
}
int mpm_set_bending(mpm_handle_t, size_t n, const float* p) { return setter("mpm_set_bending", n, p); }
int mpm_get_bending(mpm_handle_t, float* out, size_t cap, size_t* n_out) { return getter("mpm_get_bending", N.cloths, out, cap, n_out); }
int mpm_set_damping(mpm_handle_t, size_t n, const mpm_cloth_damping_t* p) { return setter("mpm_set_damping", n, p); }
int mpm_get_damping(mpm_handle_t, mpm_cloth_damping_t* out, size_t cap, size_t* n_out) {
    return getter("mpm_get_damping", N.cloths, out, cap, n_out);
}
int mpm_set_weave(mpm_handle_t, size_t n, const mpm_cloth_weave_t* w, const float* face_dirs) {
    stub::Call& c = log("mpm_set_weave", {(long long)n, w != nullptr, face_dirs != nullptr});
    reads(c, w, n);
    reads(c, face_dirs, 3 * N.faces);
    return 0;
}
int mpm_get_weave(mpm_handle_t, mpm_cloth_weave_t* out, size_t cap, size_t* n_out) {
    return getter("mpm_get_weave", N.cloths, out, cap, n_out);
}
int mpm_set_tearing(mpm_handle_t, size_t n, const mpm_cloth_tear_t* p) { return setter("mpm_set_tearing", n, p); }
int mpm_get_tearing(mpm_handle_t, mpm_cloth_tear_t* out, size_t cap, size_t* n_out) {
    log("mpm_get_tearing", {out != nullptr, (long long)cap, n_out != nullptr});
    for (size_t c = 0; c < N.cloths && c < cap; ++c) {
        out[c].stretch_limit = stub::tear_limit(c);
        for (int k = 0; k < 3; ++k) out[c].reserved[k] = 1000.f + float(3 * c + k);   // what a wrong field would return
    }
    if (n_out) *n_out = N.cloths;
    return 0;
}
int mpm_set_links(mpm_handle_t, size_t n, const mpm_link_t* p) { return setter("mpm_set_links", n, p); }
int mpm_get_links(mpm_handle_t, mpm_link_t* out, size_t cap, size_t* n_out) { return getter("mpm_get_links", N.links, out, cap, n_out); }
int mpm_set_link_limits(mpm_handle_t, size_t n, const float* p) { return setter("mpm_set_link_limits", n, p); }
int mpm_get_link_limits(mpm_handle_t, float* out, size_t cap, size_t* n_out) {
    return getter("mpm_get_link_limits", N.links, out, cap, n_out);
}
int mpm_set_broken_links(mpm_handle_t, size_t n, const uint8_t* p) { return setter("mpm_set_broken_links", n, p); }
int mpm_set_anchors(mpm_handle_t, size_t n, const mpm_anchor_t* p) { return setter("mpm_set_anchors", n, p); }
int mpm_get_anchors(mpm_handle_t, mpm_anchor_t* out, size_t cap, size_t* n_out) {
    return getter("mpm_get_anchors", N.anchors, out, cap, n_out);
}
int mpm_set_pressure(mpm_handle_t, size_t n, const mpm_cloth_pressure_t* p) { return setter("mpm_set_pressure", n, p); }
int mpm_get_pressure(mpm_handle_t, mpm_cloth_pressure_t* out, size_t cap, size_t* n_out) {
    return getter("mpm_get_pressure", N.cloths, out, cap, n_out);
}
int mpm_pressure_state(mpm_handle_t, mpm_cloth_pressure_state_t* out, size_t cap, size_t* n_out) {
    return getter("mpm_pressure_state", N.cloths, out, cap, n_out);
}
int mpm_set_shell_bending(mpm_handle_t, size_t n, const mpm_cloth_shell_t* p, const float* rest_pos) {
    stub::Call& c = log("mpm_set_shell_bending", {(long long)n, p != nullptr, rest_pos != nullptr});
    reads(c, p, n);
    reads(c, rest_pos, 3 * N.verts);
    return 0;
}
int mpm_get_shell_bending(mpm_handle_t, mpm_cloth_shell_t* out, size_t cap, size_t* n_out) {
    return getter("mpm_get_shell_bending", N.cloths, out, cap, n_out);
}
int mpm_set_shell_damping(mpm_handle_t, size_t n, const mpm_cloth_shell_damping_t* p) { return setter("mpm_set_shell_damping", n, p); }
int mpm_get_shell_damping(mpm_handle_t, mpm_cloth_shell_damping_t* out, size_t cap, size_t* n_out) {
    return getter("mpm_get_shell_damping", N.cloths, out, cap, n_out);
}
int mpm_set_creases(mpm_handle_t, size_t n, const mpm_cloth_crease_t* p) { return setter("mpm_set_creases", n, p); }
int mpm_get_creases(mpm_handle_t, mpm_cloth_crease_t* out, size_t cap, size_t* n_out) {
    return getter("mpm_get_creases", N.cloths, out, cap, n_out);
}
int mpm_set_body_contact_materials(mpm_handle_t, size_t n, const mpm_contact_material_t* p) {
    return setter("mpm_set_body_contact_materials", n, p);
}
int mpm_get_body_contact_materials(mpm_handle_t, mpm_contact_material_t* out, size_t cap, size_t* n_out) {
    return getter("mpm_get_body_contact_materials", N.materials, out, cap, n_out);
}
int mpm_set_sdf_colliders(mpm_handle_t, size_t n, const mpm_sdf_collider_t* p) { return setter("mpm_set_sdf_colliders", n, p); }

// ---- per-vertex forces and the guards --------------------------------------------------------------------------------------
int mpm_bending_forces(mpm_handle_t, float* f) { return vertex_forces("mpm_bending_forces", f); }
int mpm_damping_forces(mpm_handle_t, float* f) { return vertex_forces("mpm_damping_forces", f); }
int mpm_link_forces(mpm_handle_t, float* f) { return vertex_forces("mpm_link_forces", f); }
int mpm_anchor_forces(mpm_handle_t, float* f) { return vertex_forces("mpm_anchor_forces", f); }
int mpm_pressure_forces(mpm_handle_t, float* f) { return vertex_forces("mpm_pressure_forces", f); }
int mpm_shell_forces(mpm_handle_t, float* f) { return vertex_forces("mpm_shell_forces", f); }
int mpm_shell_damping_forces(mpm_handle_t, float* f) { return vertex_forces("mpm_shell_damping_forces", f); }
int mpm_bending_max_stable_dt(mpm_handle_t, float* dt) { return guard("mpm_bending_max_stable_dt", dt); }
int mpm_damping_max_stable_dt(mpm_handle_t, float* dt) { return guard("mpm_damping_max_stable_dt", dt); }
int mpm_weave_max_stable_dt(mpm_handle_t, float* dt) { return guard("mpm_weave_max_stable_dt", dt); }
int mpm_links_max_stable_dt(mpm_handle_t, float* dt) { return guard("mpm_links_max_stable_dt", dt); }
int mpm_anchors_max_stable_dt(mpm_handle_t, float* dt) { return guard("mpm_anchors_max_stable_dt", dt); }
int mpm_shell_max_stable_dt(mpm_handle_t, float* dt) { return guard("mpm_shell_max_stable_dt", dt); }

// ---- the weave -------------------------------------------------------------------------------------------------------------
int mpm_weave_axes(mpm_handle_t, float* cs_out) {
    log("mpm_weave_axes", {cs_out != nullptr});
    fill(cs_out, 2 * N.faces, "mpm_weave_axes");
    return 0;
}
int mpm_weave_forces(mpm_handle_t, float* f_out, float* rec_out) {
    log("mpm_weave_forces", {f_out != nullptr, rec_out != nullptr});
    fill(f_out, 3 * N.verts, "mpm_weave_forces.f");
    fill(rec_out, 9 * N.faces, "mpm_weave_forces.rec");
    return 0;
}
int mpm_weave_strain(mpm_handle_t, float* out) {
    log("mpm_weave_strain", {out != nullptr});
    fill(out, 3 * N.faces, "mpm_weave_strain");
    return 0;
}
int mpm_weave_energy(mpm_handle_t, double* per_cloth, size_t cap, size_t* n_out, double* total) {
    log("mpm_weave_energy", {per_cloth != nullptr, (long long)cap, n_out != nullptr, total != nullptr});
    if (cap && !per_cloth) return MPM_ERR_INVALID;
    if (cap) fill(per_cloth, N.cloths < cap ? N.cloths : cap, "mpm_weave_energy");
    if (n_out) *n_out = N.cloths;
    if (total) *total = stub::WEAVE_TOTAL;
    return 0;
}

// ---- tearing and its coupling ----------------------------------------------------------------------------------------------
int mpm_set_torn_faces(mpm_handle_t, const uint8_t* torn) {
    reads(log("mpm_set_torn_faces", {torn != nullptr}), torn, N.faces);
    return 0;
}
int mpm_tear_state(mpm_handle_t, uint8_t* torn_out, uint32_t* count_per_cloth, size_t cap, size_t* n_out) {
    log("mpm_tear_state", {torn_out != nullptr, count_per_cloth != nullptr, (long long)cap, n_out != nullptr});
    if (cap && !count_per_cloth) return MPM_ERR_INVALID;
    fill(torn_out, N.faces, "mpm_tear_state.torn");
    if (cap) fill(count_per_cloth, N.cloths < cap ? N.cloths : cap, "mpm_tear_state.counts");
    if (n_out) *n_out = N.cloths;
    return 0;
}
int mpm_tear_measure(mpm_handle_t, float* mq_out, uint8_t* would_fail_out) {
    log("mpm_tear_measure", {mq_out != nullptr, would_fail_out != nullptr});
    fill(mq_out, 2 * N.faces, "mpm_tear_measure.mq");
    fill(would_fail_out, N.faces, "mpm_tear_measure.would_fail");
    return 0;
}
int mpm_set_tear_coupling(mpm_handle_t, uint32_t mask) {
    log("mpm_set_tear_coupling", {(long long)mask});
    return 0;
}
int mpm_get_tear_coupling(mpm_handle_t, uint32_t* mask_out) {
    *mask_out = stub::COUPLING;
    return 0;
}
int mpm_shell_cut_hinges(mpm_handle_t, uint8_t* cut_out, uint32_t* cut_per_cloth, size_t cap, size_t* n_out) {
    log("mpm_shell_cut_hinges", {cut_out != nullptr, cut_per_cloth != nullptr, (long long)cap, n_out != nullptr});
    if (cap && !cut_per_cloth) return MPM_ERR_INVALID;
    fill(cut_out, N.hinges, "mpm_shell_cut_hinges.cut");
    if (cap) fill(cut_per_cloth, N.cloths < cap ? N.cloths : cap, "mpm_shell_cut_hinges.counts");
    if (n_out) *n_out = N.cloths;
    return 0;
}
int mpm_pressure_vented(mpm_handle_t, uint8_t* vented, size_t cap, size_t* n_out) {
    return getter("mpm_pressure_vented", N.cloths, vented, cap, n_out);
}

// ---- the rest shape --------------------------------------------------------------------------------------------------------
int mpm_set_rest_shape(mpm_handle_t, const float* rest_pos) {
    reads(log("mpm_set_rest_shape", {rest_pos != nullptr}), rest_pos, 3 * N.verts);
    return 0;
}
int mpm_get_rest_shape(mpm_handle_t, float* rest_pos_out, int* is_set_out) {
    log("mpm_get_rest_shape", {rest_pos_out != nullptr, is_set_out != nullptr});
    fill(rest_pos_out, 3 * N.verts, "mpm_get_rest_shape");
    if (is_set_out) *is_set_out = 1;
    return 0;
}

// ---- links and anchors -----------------------------------------------------------------------------------------------------
int mpm_link_energy(mpm_handle_t, double* energy_out, float* length_out) {
    log("mpm_link_energy", {energy_out != nullptr, length_out != nullptr});
    if (energy_out) *energy_out = stub::LINK_ENERGY;
    fill(length_out, N.links, "mpm_link_energy.length");
    return 0;
}
int mpm_link_break_state(mpm_handle_t, uint8_t* broken_out, uint32_t* count_out) {
    log("mpm_link_break_state", {broken_out != nullptr, count_out != nullptr});
    fill(broken_out, N.links, "mpm_link_break_state");
    if (count_out) *count_out = stub::BROKEN;
    return 0;
}
int mpm_link_break_measure(mpm_handle_t, float* l2_out, uint8_t* would_break_out) {
    log("mpm_link_break_measure", {l2_out != nullptr, would_break_out != nullptr});
    fill(l2_out, N.links, "mpm_link_break_measure.l2");
    fill(would_break_out, N.links, "mpm_link_break_measure.would_break");
    return 0;
}
int mpm_anchor_state(mpm_handle_t, double* energy_out, float* length_out, float* point_out, double* impulse_quantum_out) {
    log("mpm_anchor_state", {energy_out != nullptr, length_out != nullptr, point_out != nullptr, impulse_quantum_out != nullptr});
    if (energy_out) *energy_out = stub::ANCHOR_ENERGY;
    fill(length_out, N.anchors, "mpm_anchor_state.length");
    fill(point_out, 3 * N.anchors, "mpm_anchor_state.point");
    if (impulse_quantum_out) *impulse_quantum_out = stub::ANCHOR_QUANTUM;
    return 0;
}

// ---- shell bending, its damper, creases --------------------------------------------------------------------------------------
int mpm_shell_hinges(mpm_handle_t, int32_t* ids4, float* kc, float* psibar, size_t cap, size_t* n_out) {
    log("mpm_shell_hinges", {ids4 != nullptr, kc != nullptr, psibar != nullptr, (long long)cap, n_out != nullptr});
    const size_t n = N.hinges < cap ? N.hinges : cap;
    fill(ids4, 4 * n, "mpm_shell_hinges.ids4");
    fill(kc, n, "mpm_shell_hinges.kc");
    fill(psibar, n, "mpm_shell_hinges.psibar");
    if (n_out) *n_out = N.hinges;
    return 0;
}
int mpm_shell_state(mpm_handle_t, double* energy_per_cloth, float* psi_out, uint32_t* inactive_out) {
    log("mpm_shell_state", {energy_per_cloth != nullptr, psi_out != nullptr, inactive_out != nullptr});
    fill(energy_per_cloth, N.cloths, "mpm_shell_state.energy");
    fill(psi_out, N.hinges, "mpm_shell_state.psi");
    if (inactive_out) *inactive_out = 0;
    return 0;
}
int mpm_shell_damping_state(mpm_handle_t, double* power_per_cloth, float* psidot_out) {
    log("mpm_shell_damping_state", {power_per_cloth != nullptr, psidot_out != nullptr});
    fill(power_per_cloth, N.cloths, "mpm_shell_damping_state.power");
    fill(psidot_out, N.hinges, "mpm_shell_damping_state.psidot");
    return 0;
}
int mpm_set_crease_state(mpm_handle_t, const float* psibar) {
    reads(log("mpm_set_crease_state", {psibar != nullptr}), psibar, N.hinges);
    return 0;
}
int mpm_crease_state(mpm_handle_t, float* psibar_out, uint32_t* creased_per_cloth, size_t cap, size_t* n_out) {
    log("mpm_crease_state", {psibar_out != nullptr, creased_per_cloth != nullptr, (long long)cap, n_out != nullptr});
    if (cap && !creased_per_cloth) return MPM_ERR_INVALID;
    fill(psibar_out, N.hinges, "mpm_crease_state.psibar");
    if (cap) fill(creased_per_cloth, N.cloths < cap ? N.cloths : cap, "mpm_crease_state.counts");
    if (n_out) *n_out = N.cloths;
    return 0;
}
int mpm_crease_measure(mpm_handle_t, float* psi_out, float* dpsi_out, float* psibar_next_out) {
    log("mpm_crease_measure", {psi_out != nullptr, dpsi_out != nullptr, psibar_next_out != nullptr});
    fill(psi_out, N.hinges, "mpm_crease_measure.psi");
    fill(dpsi_out, N.hinges, "mpm_crease_measure.dpsi");
    fill(psibar_next_out, N.hinges, "mpm_crease_measure.next");
    return 0;
}

// ---- the report ------------------------------------------------------------------------------------------------------------
int mpm_measure(mpm_handle_t, mpm_cloth_measure_t* per_cloth, size_t cap, size_t* n_cloths_out, mpm_cloth_measure_t* total) {
    log("mpm_measure", {per_cloth != nullptr, (long long)cap, n_cloths_out != nullptr, total != nullptr});
    if (cap && !per_cloth) return MPM_ERR_INVALID;
    if (cap) fill(per_cloth, N.cloths < cap ? N.cloths : cap, "mpm_measure.rows");
    if (n_cloths_out) *n_cloths_out = N.cloths;
    if (total) {
        std::memset(total, 0, sizeof *total);
        total->kinetic = stub::KINETIC;
        total->kinetic_affine = stub::KINETIC_AFFINE;
        total->gravity_potential = stub::GRAVITY;
        total->elastic_in_plane = stub::IN_PLANE;
        total->elastic_normal = stub::NORMAL;
        total->elastic_shear = stub::SHEAR;
        total->bending = stub::BENDING;
        total->mass = 1e6;   // (in no energy)
    }
    return 0;
}
int mpm_face_strain(mpm_handle_t, float* out) {
    log("mpm_face_strain", {out != nullptr});
    fill(out, 4 * N.faces, "mpm_face_strain");
    return 0;
}

// ---- contact ---------------------------------------------------------------------------------------------------------------
int mpm_collider_signed_distance(mpm_handle_t, const mpm_collider_t* c, size_t n, const float* x_W, float* phi_out, float* grad_W_out) {
    stub::Call& l = log("mpm_collider_signed_distance", {c != nullptr, (long long)n});
    reads(l, c, 1);
    reads(l, x_W, 3 * n);
    fill(phi_out, n, "mpm_collider_signed_distance.phi");
    fill(grad_W_out, 3 * n, "mpm_collider_signed_distance.grad");
    return 0;
}
int mpm_sdf_collider_signed_distance(mpm_handle_t, const mpm_sdf_collider_t* c, size_t n, const float* x_W, float* phi_out,
                                     float* grad_W_out) {
    stub::Call& l = log("mpm_sdf_collider_signed_distance", {c != nullptr, (long long)n});
    reads(l, c, 1);
    reads(l, x_W, 3 * n);
    fill(phi_out, n, "mpm_sdf_collider_signed_distance.phi");
    fill(grad_W_out, 3 * n, "mpm_sdf_collider_signed_distance.grad");
    return 0;
}
int mpm_generate_contact_pairs(mpm_handle_t, size_t n_colliders, const mpm_collider_t* colliders, size_t* n_contacts_out) {
    reads(log("mpm_generate_contact_pairs", {(long long)n_colliders, n_contacts_out != nullptr}), colliders, n_colliders);
    if (n_contacts_out) *n_contacts_out = N.contacts;
    return 0;
}
int mpm_get_contact_pair_count(mpm_handle_t, size_t* n_contacts_out) {
    *n_contacts_out = N.contacts;
    return 0;
}
int mpm_download_contact_pairs(mpm_handle_t, uint32_t* particle, uint32_t* body, float* dist, float* normal, float* position,
                               float* rigid_v, float* rigid_p_WB) {
    log("mpm_download_contact_pairs", {particle != nullptr, body != nullptr, dist != nullptr, normal != nullptr, position != nullptr,
                                       rigid_v != nullptr, rigid_p_WB != nullptr});
    fill(particle, N.contacts, "mpm_download_contact_pairs.particle");
    fill(body, N.contacts, "mpm_download_contact_pairs.body");
    fill(dist, N.contacts, "mpm_download_contact_pairs.dist");
    fill(normal, 3 * N.contacts, "mpm_download_contact_pairs.normal");
    fill(position, 3 * N.contacts, "mpm_download_contact_pairs.position");
    fill(rigid_v, 3 * N.contacts, "mpm_download_contact_pairs.rigid_v");
    fill(rigid_p_WB, 3 * N.contacts, "mpm_download_contact_pairs.rigid_p_WB");
    return 0;
}
int mpm_run_coupled_substeps(mpm_handle_t, int n, const mpm_coupled_params_t* params, size_t n_colliders,
                             const mpm_collider_t* colliders, mpm_coupled_result_t* results) {
    stub::Call& c = log("mpm_run_coupled_substeps", {n, params != nullptr, (long long)n_colliders, results != nullptr});
    reads(c, params, 1);
    reads(c, colliders, n_colliders);
    for (int k = 0; results && k < n; ++k) {   // (the facade adds the iterations and keeps the last count: numbers)
        results[k].iterations = k + 1;
        results[k].contacts = 100u + unsigned(k);
        results[k].nodes = 200u + unsigned(k);
        results[k].residual = 0.5f * float(k);
        results[k].setup_reused = k & 1;
    }
    return 0;
}

}  // extern "C"
