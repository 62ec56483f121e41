// gpu_mpm.hpp -- header-only C++ facade over the C ABI (mpm_hip.h) that re-creates the
// reference's class interface, so that a caller written against
//   multibody/gpu_mpm/cuda_mpm_model.cuh   (GpuMpmState<T>)
//   multibody/gpu_mpm/cuda_mpm_solver.cuh  (GpuMpmSolver<T>)
//   multibody/gpu_mpm/cpu_mpm_model.h      (MpmConfigParams, MpmParticleContactPairs, ...)
// compiles against this engine by swapping the include.  Method names, argument order and
// meaning are the reference's; only T = float exists (as in the reference, settings.h:37).
//
// Vec3<T> here is std::array<T,3>; Eigen::Vector3f has the same layout (three packed floats),
// so inside Drake the arrays can be passed through reinterpret_cast or Eigen::Map.
#pragma once
#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <tuple>
#include <vector>

#include "mpm_hip.h"

namespace drake {
namespace multibody {
namespace gmpm {

template <typename T> using Vec3 = std::array<T, 3>;
namespace config { using GpuT = float; }

inline void mpm_check(int rc) {
    if (rc != 0) throw std::runtime_error(std::string("mpm_hip: ") + mpm_last_error());
}

// cpu_mpm_model.h:16-26
template <typename T = config::GpuT>
struct MpmConfigParams {
    T substep_dt{static_cast<T>(1e-3)};
    bool write_files{false};
    T contact_stiffness{static_cast<T>(1e5)};
    T contact_damping{static_cast<T>(0.0)};
    T contact_friction_mu{static_cast<T>(0.0)};
    int contact_query_frequency{1};
    int mpm_bc{-1};
    bool exact_line_search{false};
    // extension: contact material per rigid body (mpm_set_body_contact_materials); entry b belongs to body b, a field < 0
    // and every body beyond the vector take the three scalars above.  Empty: the scalars for every body.
    std::vector<mpm_contact_material_t> body_contact_materials;
};

// cpu_mpm_model.h:32-40
template <typename T>
struct CpuMpmModel {
    std::vector<Vec3<T>> cloth_pos;
    std::vector<Vec3<T>> cloth_vel;
    std::vector<int> cloth_indices;
    MpmConfigParams<T> config;
};

// cpu_mpm_model.h:45-49
template <typename T>
struct MpmPortData {
    std::vector<Vec3<T>> pos;
    std::vector<int> indices;
};

// cpu_mpm_model.h:73-114
template <typename T>
struct MpmParticleContactPairs {
    std::vector<uint32_t> particle_in_contact_index;
    std::vector<uint32_t> non_mpm_id;
    std::vector<T> penetration_distance;
    std::vector<Vec3<T>> normal;
    std::vector<Vec3<T>> particle_in_contact_position;
    std::vector<Vec3<T>> rigid_v;
    std::vector<Vec3<T>> rigid_p_WB;
    void clear() {
        particle_in_contact_index.clear(); non_mpm_id.clear(); penetration_distance.clear(); normal.clear();
        particle_in_contact_position.clear(); rigid_v.clear(); rigid_p_WB.clear();
    }
    void push_back(uint32_t particle, uint32_t body, T dist, Vec3<T> n, Vec3<T> pos, Vec3<T> v, Vec3<T> p_WB) {
        particle_in_contact_index.push_back(particle); non_mpm_id.push_back(body);
        penetration_distance.push_back(dist); normal.push_back(n); particle_in_contact_position.push_back(pos);
        rigid_v.push_back(v); rigid_p_WB.push_back(p_WB);
    }
    size_t size() const { return non_mpm_id.size(); }
};

// cuda_mpm_model.cuh:19-35
template <typename T>
struct ExternalSpatialForce {
    std::vector<Vec3<T>> p_BoBq_B;
    std::vector<Vec3<T>> F_Bq_W_tau;
    std::vector<Vec3<T>> F_Bq_W_f;
    size_t size() const { return p_BoBq_B.size(); }
    void resize(size_t n) { p_BoBq_B.resize(n); F_Bq_W_tau.resize(n); F_Bq_W_f.resize(n); }
};

// cuda_mpm_model.cuh:37-260.  Copies alias the same engine handle, like the reference's
// shallow-copied device pointers (deformable_model.cc:428); Destroy() is explicit.
template <typename T>
struct GpuMpmState {
    static_assert(sizeof(T) == sizeof(float), "only float is instantiated, as in the reference");
    explicit GpuMpmState(int domain_bits = 7, const mpm_material_t* material = nullptr, int device = 0) {
        mpm_check(mpm_create(domain_bits, material, device, &h_));
    }
    mpm_handle_t handle() const { return h_; }

    size_t n_verts() const { size_t a, b, c; mpm_check(mpm_counts(h_, &a, &b, &c)); return a; }
    size_t n_faces() const { size_t a, b, c; mpm_check(mpm_counts(h_, &a, &b, &c)); return b; }
    size_t n_particles() const { size_t a, b, c; mpm_check(mpm_counts(h_, &a, &b, &c)); return c; }

    void AddQRCloth(const std::vector<Vec3<T>>& pos, const std::vector<Vec3<T>>& vel, const std::vector<int>& indices) {
        mpm_check(mpm_add_qr_cloth(h_, reinterpret_cast<const float*>(pos.data()),
                                   reinterpret_cast<const float*>(vel.data()), pos.size(), indices.data(),
                                   indices.size() / 3));
    }
    // Extension: a cloth with a material of its own (DeformableBodyConfig per body, deformable_model.h:161-163): E, nu,
    // rho, gamma, K and c_F; the rest stays the engine's.  See mpm_add_qr_cloth_with_material.
    void AddQRCloth(const std::vector<Vec3<T>>& pos, const std::vector<Vec3<T>>& vel, const std::vector<int>& indices,
                    const mpm_cloth_material_t& material) {
        mpm_check(mpm_add_qr_cloth_with_material(h_, reinterpret_cast<const float*>(pos.data()),
                                                 reinterpret_cast<const float*>(vel.data()), pos.size(), indices.data(),
                                                 indices.size() / 3, &material));
    }
    size_t n_cloths() const { size_t n = 0; mpm_check(mpm_cloth_count(h_, &n)); return n; }
    mpm_cloth_material_t cloth_material(size_t cloth) const {
        mpm_cloth_material_t m{};
        mpm_check(mpm_get_cloth_info(h_, cloth, nullptr, nullptr, nullptr, nullptr, &m));
        return m;
    }
    void Finalize() { mpm_check(mpm_finalize(h_)); }
    void Destroy() { mpm_check(mpm_destroy(h_)); h_ = nullptr; }

    using DumpT = std::tuple<std::vector<Vec3<T>>, std::vector<int>>;
    DumpT DumpCpuState() const {
        std::vector<Vec3<T>> pos(n_verts());
        std::vector<int> idx(n_faces() * 3);
        mpm_check(mpm_dump_cpu_state(h_, reinterpret_cast<float*>(pos.data()), idx.data()));
        return std::make_tuple(pos, idx);
    }
    void ReallocateContacts(size_t) {}  // implicit in CopyContactPairs
    // extension: bitwise run-to-run reproducibility (see mpm_set_deterministic).  Call it before Finalize: the order inside
    // a cell is canonical from Finalize's own first sort on; switched on later, every re-sort keeps the order that sort left
    void SetDeterministic(bool on) { mpm_check(mpm_set_deterministic(h_, on ? 1 : 0)); }
    void ReallocateExternelBodies(size_t n) { mpm_check(mpm_reallocate_external_bodies(h_, n)); n_bodies_ = n; }
    void ExternelBodyForceToHost() {
        h_external_forces_.resize(n_bodies_);
        mpm_check(mpm_external_body_force_to_host(h_, reinterpret_cast<float*>(h_external_forces_.F_Bq_W_tau.data()),
                                                  reinterpret_cast<float*>(h_external_forces_.F_Bq_W_f.data())));
    }
    uint32_t grid_touched_cnt_host() const { uint32_t c = 0; mpm_check(mpm_grid_touched_cnt(h_, &c)); return c; }
    // Extension: DeformableModel::AddFixedConstraint (deformable_model.h:227-230) for the cloth.  Pins every vertex inside
    // shape G (an analytic collider posed in the world) to body `body`, whose pose is X_WB = (p_WB, R_WB row-major);
    // returns the number of pins added (none: throws, as Drake does).  See mpm_pins_inside_collider.
    size_t AddFixedConstraint(uint32_t body, const mpm_collider_t& shape_G, const Vec3<T>& p_WB, const std::array<T, 9>& R_WB) {
        size_t n = 0;
        mpm_check(mpm_pins_inside_collider(h_, &shape_G, body, p_WB.data(), R_WB.data(), &n));
        return n;
    }
    // the poses of the pinned bodies at the start of the plant step and their spatial velocities (CalcAbstractStates):
    // once per step, before its substeps.  See mpm_set_body_motions.
    void SetBodyMotions(const std::vector<mpm_body_motion_t>& motions) {
        mpm_check(mpm_set_body_motions(h_, motions.size(), motions.data()));
    }
    void SetPins(const std::vector<mpm_pin_t>& pins) { mpm_check(mpm_set_pins(h_, pins.size(), pins.data())); }
    std::vector<mpm_pin_t> GetPins() const { return table<mpm_pin_t>(mpm_get_pins); }
    // Extension: rigid bodies in UpdateGrid's boundary condition (mpm_set_grid_bodies).  The table that
    // UpdateGrid(state, MPM_BC_BODIES) and the substep calls with that mpm_bc use: once per plant step, from the body
    // poses and spatial velocities of CalcAbstractStates, before its substeps.  The bodies' reactions arrive in
    // external_forces_host() with the contact impulses (ExternelBodyForceToHost).
    void SetGridBodies(const std::vector<mpm_grid_body_t>& bodies) {
        mpm_check(mpm_set_grid_bodies(h_, bodies.size(), bodies.data()));
    }
    std::vector<mpm_grid_body_t> GetGridBodies() const { return table<mpm_grid_body_t>(mpm_get_grid_bodies); }
    // Extension: external force fields evaluated inside ParticleToGrid (mpm_set_force_fields): off-axis gravity,
    // springs, drag towards a wind, drag along the cloth's normal.  Coefficients are per unit mass: a Drake force
    // density with coefficient c per unit volume maps to gamma = c / rho.  Once per plant step, before its substeps.
    void SetForceFields(const std::vector<mpm_force_field_t>& fields) {
        mpm_check(mpm_set_force_fields(h_, fields.size(), fields.data()));
    }
    std::vector<mpm_force_field_t> GetForceFields() const { return table<mpm_force_field_t>(mpm_get_force_fields); }
    // Extension: bending stiffness per cloth (mpm_set_bending), the quadratic hinge energy on a flat rest shape; all
    // zeros or an empty vector switches it off.  A synchronisation point, like SetForceFields.
    void SetBending(const std::vector<float>& stiffness) { mpm_check(mpm_set_bending(h_, stiffness.size(), stiffness.data())); }
    std::vector<float> GetBending() const { return table<float>(mpm_get_bending); }
    // -k Q x on the current positions, 3 floats per vertex in the numbering of DumpCpuState (a diagnostic)
    std::vector<float> BendingForces(size_t n_verts) const { return vertex_forces(mpm_bending_forces, n_verts, "BendingForces"); }
    // the dt above which the substep entry points refuse an engine with bending (+inf while it is off)
    float BendingMaxStableDt() const { return max_stable_dt(mpm_bending_max_stable_dt); }
    // Extension: stiffness-proportional damping per cloth (mpm_set_damping), the counterpart of Drake's
    // DeformableBodyConfig::stiffness_damping_coefficient: {membrane, bending} in seconds; all zeros or an empty vector
    // switches it off.  A synchronisation point, like SetBending.
    void SetDamping(const std::vector<mpm_cloth_damping_t>& d) { mpm_check(mpm_set_damping(h_, d.size(), d.data())); }
    std::vector<mpm_cloth_damping_t> GetDamping() const { return table<mpm_cloth_damping_t>(mpm_get_damping); }
    // the damping force on the current positions and velocities, 3 floats per vertex in the numbering of DumpCpuState
    std::vector<float> DampingForces(size_t n_verts) const { return vertex_forces(mpm_damping_forces, n_verts, "DampingForces"); }
    // the dt above which the substep entry points refuse an engine with damping (+inf while it is off)
    float DampingMaxStableDt() const { return max_stable_dt(mpm_damping_max_stable_dt); }
    // the membrane damping kernel's face function on the host: n faces, see mpm_damping_face_records
    static std::vector<float> DampingFaceRecords(size_t n, const float* dminv3, const float* vol, const float* mu,
                                                 const float* lambda, const float* beta, const float* x9, const float* v9) {
        std::vector<float> rec(9 * n);
        mpm_check(mpm_damping_face_records(n, dminv3, vol, mu, lambda, beta, x9, v9, rec.data()));
        return rec;
    }
    // Extension: woven cloth (mpm_set_weave) -- orthotropic warp / weft / shear stiffness per cloth, added to the isotropic
    // membrane; face_dirs: empty, or 3 floats per face (a zero entry falls back to the cloth's warp_dir).  All-zero moduli
    // or an empty vector switches it off.  A synchronisation point, like SetBending.
    void SetWeave(const std::vector<mpm_cloth_weave_t>& w, const std::vector<float>& face_dirs = {}) {
        mpm_check(mpm_set_weave(h_, w.size(), w.data(), face_dirs.empty() ? nullptr : face_dirs.data()));
    }
    std::vector<mpm_cloth_weave_t> GetWeave() const { return table<mpm_cloth_weave_t>(mpm_get_weave); }
    // (c, s) of the warp per face in the face's rest frame, 2 floats per face in the numbering of DumpCpuState
    std::vector<float> WeaveAxes(size_t n_faces) const {
        expect("WeaveAxes", "n_faces", n_faces, this->n_faces());
        std::vector<float> cs(2 * n_faces);
        mpm_check(mpm_weave_axes(h_, cs.data()));
        return cs;
    }
    // the weave's force on the current positions, 3 floats per vertex; records: null, or receives 9 floats per face of the
    // engine (n_faces: 0, or the engine's face count)
    std::vector<float> WeaveForces(size_t n_verts, std::vector<float>* records = nullptr, size_t n_faces = 0) const {
        expect("WeaveForces", "n_verts", n_verts, this->n_verts());
        std::vector<float> f(3 * n_verts);
        if (records) {
            const size_t nf = this->n_faces();
            if (n_faces != 0) expect("WeaveForces", "n_faces", n_faces, nf);
            records->assign(9 * nf, 0.f);
        }
        mpm_check(mpm_weave_forces(h_, f.data(), records ? records->data() : nullptr));
        return f;
    }
    // Eaa, Ebb, Eab per face
    std::vector<float> WeaveStrain(size_t n_faces) const {
        expect("WeaveStrain", "n_faces", n_faces, this->n_faces());
        std::vector<float> out(3 * n_faces);
        mpm_check(mpm_weave_strain(h_, out.data()));
        return out;
    }
    // the weave's elastic energy per cloth; total: null, or the sum of the rows
    std::vector<double> WeaveEnergy(double* total = nullptr) const {
        size_t n = 0;
        mpm_check(mpm_weave_energy(h_, nullptr, 0, &n, nullptr));
        std::vector<double> out(n);
        mpm_check(mpm_weave_energy(h_, out.data(), n, &n, total));
        return out;
    }
    // the dt above which the substep entry points refuse an engine with a weave (+inf while it is off)
    float WeaveMaxStableDt() const { return max_stable_dt(mpm_weave_max_stable_dt); }
    // Extension: tearing cloth (mpm_set_tearing) -- one stretch limit per cloth (0: never tears; else finite and > 1); a
    // face whose largest in-plane stretch exceeds it fails for good and exerts no force from then on.  A synchronisation
    // point, like SetBending.
    void SetTearing(const std::vector<float>& stretch_limits) {
        std::vector<mpm_cloth_tear_t> t(stretch_limits.size(), mpm_cloth_tear_t{0.f, {0.f, 0.f, 0.f}});
        for (size_t c = 0; c < t.size(); ++c) t[c].stretch_limit = stretch_limits[c];
        mpm_check(mpm_set_tearing(h_, t.size(), t.data()));
    }
    std::vector<float> GetTearing() const {
        size_t n = 0;
        mpm_check(mpm_get_tearing(h_, nullptr, 0, &n));
        std::vector<mpm_cloth_tear_t> t(n);
        mpm_check(mpm_get_tearing(h_, t.data(), n, &n));
        std::vector<float> out(n);
        for (size_t c = 0; c < n; ++c) out[c] = t[c].stretch_limit;
        return out;
    }
    // scissors / restore: one byte per face in the numbering of DumpCpuState, non-zero = torn; replaces every flag
    void SetTornFaces(const std::vector<uint8_t>& torn) {
        if (torn.size() != n_faces()) throw std::invalid_argument("SetTornFaces: one byte per face");
        mpm_check(mpm_set_torn_faces(h_, torn.data()));
    }
    // the flags per face; counts: null, or the torn faces per cloth
    std::vector<uint8_t> TearState(size_t n_faces, std::vector<uint32_t>* counts = nullptr) const {
        expect("TearState", "n_faces", n_faces, this->n_faces());
        size_t n = 0;
        mpm_check(mpm_tear_state(h_, nullptr, nullptr, 0, &n));
        std::vector<uint8_t> torn(n_faces);
        std::vector<uint32_t> c(n);
        mpm_check(mpm_tear_state(h_, torn.data(), c.data(), n, &n));
        if (counts) counts->swap(c);
        return torn;
    }
    // (m, q) per face on the current positions, 2 floats per face; would_fail: null, or the verdict per face
    std::vector<float> TearMeasure(size_t n_faces, std::vector<uint8_t>* would_fail = nullptr) const {
        expect("TearMeasure", "n_faces", n_faces, this->n_faces());
        std::vector<float> mq(2 * n_faces);
        if (would_fail) would_fail->assign(n_faces, 0);
        mpm_check(mpm_tear_measure(h_, mq.data(), would_fail ? would_fail->data() : nullptr));
        return mq;
    }
    // Extension: tearing composed with shell bending and gas (mpm_set_tear_coupling) -- MPM_TEAR_CUTS_HINGES: a hinge with
    // a torn face carries no moment; MPM_TEAR_VENTS_GAS: a gas cloth with a torn face has gauge 0.  0, the default, keeps
    // both combinations refused.
    void SetTearCoupling(uint32_t mask) { mpm_check(mpm_set_tear_coupling(h_, mask)); }
    uint32_t GetTearCoupling() const {
        uint32_t mask = 0;
        mpm_check(mpm_get_tear_coupling(h_, &mask));
        return mask;
    }
    // one byte per hinge of the table in force (n_hinges: mpm_shell_hinges' count): 1 where the hinge is cut on the current
    // flags; counts: null, or the cut hinges per cloth
    std::vector<uint8_t> ShellCutHinges(size_t n_hinges, std::vector<uint32_t>* counts = nullptr) const {
        expect("ShellCutHinges", "n_hinges", n_hinges, ShellHingeCount());
        size_t n = 0;
        mpm_check(mpm_shell_cut_hinges(h_, nullptr, nullptr, 0, &n));
        std::vector<uint8_t> cut(n_hinges);
        std::vector<uint32_t> c(n);
        mpm_check(mpm_shell_cut_hinges(h_, cut.data(), c.data(), n, &n));
        if (counts) counts->swap(c);
        return cut;
    }
    // per cloth: 1 where a gas cloth is vented on the current flags
    std::vector<uint8_t> PressureVented() const {
        size_t n = 0;
        mpm_check(mpm_pressure_vented(h_, nullptr, 0, &n));
        std::vector<uint8_t> v(n);
        mpm_check(mpm_pressure_vented(h_, v.data(), n, &n));
        return v;
    }
    // Extension: the rest shape apart from the pose (mpm_set_rest_shape) -- Dm^-1, volumes and masses computed again from
    // rest_pos (3 floats per vertex in the numbering of DumpCpuState), as Finalize would have on cloths added there; the
    // state and the particle order stay.  Mass follows the rest shape.  Refused while a table derived from the rest shape
    // is in force (see mpm_hip.h).  A synchronisation point, like SetBending.
    void SetRestShape(const std::vector<float>& rest_pos) {
        if (rest_pos.size() != 3 * n_verts()) throw std::invalid_argument("SetRestShape: three floats per vertex");
        mpm_check(mpm_set_rest_shape(h_, rest_pos.data()));
    }
    // back to the positions as added
    void ClearRestShape() { mpm_check(mpm_set_rest_shape(h_, nullptr)); }
    // the rest shape in force; is_set: null, or whether the caller gave it
    std::vector<float> GetRestShape(bool* is_set = nullptr) const {
        std::vector<float> out(3 * n_verts());
        int set = 0;
        mpm_check(mpm_get_rest_shape(h_, out.data(), &set));
        if (is_set) *is_set = set != 0;
        return out;
    }
    // Extension: links between cloth vertices (mpm_set_links) -- seams, springs, tension-only cords; an empty vector
    // clears them.  A synchronisation point, like SetBending.
    void SetLinks(const std::vector<mpm_link_t>& links) { mpm_check(mpm_set_links(h_, links.size(), links.data())); }
    std::vector<mpm_link_t> GetLinks() const { return table<mpm_link_t>(mpm_get_links); }
    // the links' force on the current positions and velocities, 3 floats per vertex in the numbering of DumpCpuState
    std::vector<float> LinkForces(size_t n_verts) const { return vertex_forces(mpm_link_forces, n_verts, "LinkForces"); }
    // sum of 1/2 k (l - L)^2 over the links that act; `lengths`, if given, receives every link's float length
    double LinkEnergy(std::vector<float>* lengths = nullptr) const {
        double e = 0.0;
        if (lengths) {
            size_t n = 0;
            mpm_check(mpm_get_links(h_, nullptr, 0, &n));
            lengths->resize(n);
        }
        mpm_check(mpm_link_energy(h_, &e, lengths && !lengths->empty() ? lengths->data() : nullptr));
        return e;
    }
    // the dt above which the substep entry points refuse an engine with links (+inf while the table is empty)
    float LinksMaxStableDt() const { return max_stable_dt(mpm_links_max_stable_dt); }
    // one link's force on its end a, on the host: see mpm_link_force
    static void LinkForce(const mpm_link_t& link, const float xa[3], const float xb[3], const float va[3], const float vb[3],
                          float f_on_a[3]) {
        mpm_check(mpm_link_force(&link, xa, xb, va, vb, f_on_a));
    }
    // Extension: breakable links (mpm_set_link_limits) -- one break_length per link (0: never breaks; else finite and >
    // rest_length); a link whose length exceeds it breaks for good and acts no more.  An empty vector switches every limit
    // off.  A synchronisation point, like SetLinks.
    void SetLinkLimits(const std::vector<float>& break_lengths) {
        mpm_check(mpm_set_link_limits(h_, break_lengths.size(), break_lengths.data()));
    }
    std::vector<float> GetLinkLimits() const { return table<float>(mpm_get_link_limits); }
    // scissors / restore: one byte per link in link order, non-zero = broken; replaces every flag
    void SetBrokenLinks(const std::vector<uint8_t>& broken) { mpm_check(mpm_set_broken_links(h_, broken.size(), broken.data())); }
    // the flags per link; count: null, or the number of broken links
    std::vector<uint8_t> LinkBreakState(uint32_t* count = nullptr) const {
        size_t n = 0;
        mpm_check(mpm_get_links(h_, nullptr, 0, &n));
        std::vector<uint8_t> broken(n);
        uint32_t k = 0;
        mpm_check(mpm_link_break_state(h_, broken.data(), &k));
        if (count) *count = k;
        return broken;
    }
    // l2 per link on the current positions; would_break: null, or the verdict per link
    std::vector<float> LinkBreakMeasure(std::vector<uint8_t>* would_break = nullptr) const {
        size_t n = 0;
        mpm_check(mpm_get_links(h_, nullptr, 0, &n));
        std::vector<float> l2(n);
        if (would_break) would_break->assign(n, 0);
        mpm_check(mpm_link_break_measure(h_, l2.data(), would_break ? would_break->data() : nullptr));
        return l2;
    }
    // Extension: anchors (mpm_set_anchors) -- springs and tension-only cords from cloth vertices to points of rigid bodies,
    // whose motions are those of SetBodyMotions and whose reactions arrive where the pins' do; an empty vector clears them.
    // A synchronisation point, like SetLinks.
    void SetAnchors(const std::vector<mpm_anchor_t>& anchors) { mpm_check(mpm_set_anchors(h_, anchors.size(), anchors.data())); }
    std::vector<mpm_anchor_t> GetAnchors() const { return table<mpm_anchor_t>(mpm_get_anchors); }
    // the anchors' force on the current state at the bodies' current clocks, 3 floats per vertex; adds no impulse
    std::vector<float> AnchorForces(size_t n_verts) const { return vertex_forces(mpm_anchor_forces, n_verts, "AnchorForces"); }
    // sum of 1/2 k (l - L)^2 over the anchors that act; `lengths` and `points` (3 per anchor), if given, receive every
    // anchor's float length and attachment point; `impulse_quantum`, if given, the quantum of the bodies' accumulators
    double AnchorState(std::vector<float>* lengths = nullptr, std::vector<float>* points = nullptr,
                       double* impulse_quantum = nullptr) const {
        double e = 0.0;
        size_t n = 0;
        mpm_check(mpm_get_anchors(h_, nullptr, 0, &n));
        if (lengths) lengths->resize(n);
        if (points) points->resize(3 * n);
        mpm_check(mpm_anchor_state(h_, &e, lengths && n ? lengths->data() : nullptr, points && n ? points->data() : nullptr,
                                   impulse_quantum));
        return e;
    }
    // the dt above which the substep entry points refuse an engine with anchors (+inf while the table is empty)
    float AnchorsMaxStableDt() const { return max_stable_dt(mpm_anchors_max_stable_dt); }
    // the attachment point of p_BQ and its velocity at the body's clock t, on the host: see mpm_anchor_point
    static void AnchorPoint(const mpm_body_motion_t& motion, double t, const float p_BQ[3], float y[3], float v_Q[3]) {
        mpm_check(mpm_anchor_point(&motion, t, p_BQ, y, v_Q));
    }
    // Extension: enclosed-volume pressure per cloth (mpm_set_pressure) -- one entry per cloth in AddQRCloth order; an
    // empty vector turns it off.  A synchronisation point, like SetBending.  There is no dt guard: watch PressureState.
    void SetPressure(const std::vector<mpm_cloth_pressure_t>& per_cloth) {
        mpm_check(mpm_set_pressure(h_, per_cloth.size(), per_cloth.data()));
    }
    std::vector<mpm_cloth_pressure_t> GetPressure() const { return table<mpm_cloth_pressure_t>(mpm_get_pressure); }
    // the pressure force on the current positions, 3 floats per vertex in the numbering of DumpCpuState
    std::vector<float> PressureForces(size_t n_verts) const { return vertex_forces(mpm_pressure_forces, n_verts, "PressureForces"); }
    // volume, energy, gauge pressure and cap of every cloth on the current positions
    std::vector<mpm_cloth_pressure_state_t> PressureState() const { return table<mpm_cloth_pressure_state_t>(mpm_pressure_state); }
    // host only: is the mesh closed and consistently wound?  `edge`, if given, receives the first offending directed edge
    static bool MeshIsClosed(const std::vector<int32_t>& indices, size_t n_verts, int32_t* edge = nullptr) {
        const int rc = mpm_mesh_is_closed(indices.data(), indices.size() / 3, n_verts, edge);
        if (rc < 0) mpm_check(rc);
        return rc == 1;
    }
    // host only: one row of the pressure kernel, see mpm_pressure_vertex_force
    static void PressureVertexForce(float g, const float x_own[3], size_t n, const float* x_b, const float* x_c, float f_out[3]) {
        mpm_check(mpm_pressure_vertex_force(g, x_own, n, x_b, x_c, f_out));
    }
    // Extension: shell bending about a curved rest shape (mpm_set_shell_bending), the hinge-angle model in psi = 2 sin(theta / 2)
    // -- one entry per cloth in AddQRCloth order; rest_pos: 3 floats per vertex in the numbering of DumpCpuState, or empty:
    // the mesh as added.  All zeros or an empty vector switches it off.  A synchronisation point, like SetBending.
    void SetShellBending(const std::vector<mpm_cloth_shell_t>& per_cloth, const std::vector<float>& rest_pos = {}) {
        mpm_check(mpm_set_shell_bending(h_, per_cloth.size(), per_cloth.data(), rest_pos.empty() ? nullptr : rest_pos.data()));
    }
    std::vector<mpm_cloth_shell_t> GetShellBending() const { return table<mpm_cloth_shell_t>(mpm_get_shell_bending); }
    // the hinges of the table in force (mpm_shell_hinges' count): the extent of ShellCutHinges, CreaseState, CreaseMeasure
    size_t ShellHingeCount() const {
        size_t n = 0;
        mpm_check(mpm_shell_hinges(h_, nullptr, nullptr, nullptr, 0, &n));
        return n;
    }
    // Extension: hinge damping (mpm_set_shell_damping) -- stiffness-proportional damping of the shell hinges, one {beta, 0}
    // per cloth (beta in seconds, 0: not damped); all zeros or an empty vector switches it off.  State of shell bending:
    // needs SetShellBending first, which also drops the table.  Tightens ShellMaxStableDt.  A synchronisation point.
    void SetShellDamping(const std::vector<mpm_cloth_shell_damping_t>& per_cloth) {
        mpm_check(mpm_set_shell_damping(h_, per_cloth.size(), per_cloth.data()));
    }
    std::vector<mpm_cloth_shell_damping_t> GetShellDamping() const { return table<mpm_cloth_shell_damping_t>(mpm_get_shell_damping); }
    // the damping part alone on the current positions and velocities, 3 floats per vertex in the numbering of DumpCpuState
    std::vector<float> ShellDampingForces(size_t n_verts) const { return vertex_forces(mpm_shell_damping_forces, n_verts, "ShellDampingForces"); }
    // the power the hinge dampers of every cloth dissipate on the current state
    std::vector<double> ShellDampingPower(size_t n_cloths) const {
        expect("ShellDampingPower", "n_cloths", n_cloths, this->n_cloths());
        std::vector<double> p(n_cloths);
        mpm_check(mpm_shell_damping_state(h_, p.data(), nullptr));
        return p;
    }
    // Extension: creases (mpm_set_creases) -- plastic shell hinges, one {yield_angle, hardening, max_angle} per cloth
    // (yield_angle 0: elastic); all zeros or an empty vector switches yielding off and keeps the creases made so far.
    // Needs SetShellBending first, which also drops the crease parameters and state.  A synchronisation point.
    void SetCreases(const std::vector<mpm_cloth_crease_t>& per_cloth) { mpm_check(mpm_set_creases(h_, per_cloth.size(), per_cloth.data())); }
    std::vector<mpm_cloth_crease_t> GetCreases() const { return table<mpm_cloth_crease_t>(mpm_get_creases); }
    // scissors / restore: one psibar per hinge in hinge order replaces every hinge's; an empty vector irons the cloth
    void SetCreaseState(const std::vector<float>& psibar) { mpm_check(mpm_set_crease_state(h_, psibar.empty() ? nullptr : psibar.data())); }
    // the psibar in force per hinge; counts: null, or the creased hinges per cloth
    std::vector<float> CreaseState(std::vector<uint32_t>* counts = nullptr) const {
        size_t n = 0, n_hinges = 0;
        mpm_check(mpm_crease_state(h_, nullptr, nullptr, 0, &n));
        mpm_check(mpm_shell_hinges(h_, nullptr, nullptr, nullptr, 0, &n_hinges));
        std::vector<float> psibar(n_hinges);
        std::vector<uint32_t> c(n);
        mpm_check(mpm_crease_state(h_, psibar.data(), c.data(), n, &n));
        if (counts) counts->swap(c);
        return psibar;
    }
    // the substep's hinge function on the current positions, state untouched: the psibar the next substep would leave;
    // psi and dpsi per hinge where asked for
    std::vector<float> CreaseMeasure(std::vector<float>* psi = nullptr, std::vector<float>* dpsi = nullptr) const {
        size_t n = 0;
        mpm_check(mpm_shell_hinges(h_, nullptr, nullptr, nullptr, 0, &n));
        std::vector<float> next(n);
        if (psi) psi->resize(n);
        if (dpsi) dpsi->resize(n);
        mpm_check(mpm_crease_measure(h_, psi ? psi->data() : nullptr, dpsi ? dpsi->data() : nullptr, next.data()));
        return next;
    }
    // the shell force on the current positions, 3 floats per vertex in the numbering of DumpCpuState
    std::vector<float> ShellForces(size_t n_verts) const { return vertex_forces(mpm_shell_forces, n_verts, "ShellForces"); }
    // the shell energy of every cloth on the current positions (not part of Measure's record)
    std::vector<double> ShellEnergy(size_t n_cloths) const {
        expect("ShellEnergy", "n_cloths", n_cloths, this->n_cloths());
        std::vector<double> e(n_cloths);
        mpm_check(mpm_shell_state(h_, e.data(), nullptr, nullptr));
        return e;
    }
    // the dt above which the substep entry points refuse an engine with shell bending (+inf while it is off); a guard at
    // the rest shape
    float ShellMaxStableDt() const { return max_stable_dt(mpm_shell_max_stable_dt); }
    // Extension: the per-cloth report (mpm_measure) -- masses, momenta, kinetic, potential, elastic and bending energies,
    // strain extremes, reduced on the device in double.  One row per cloth; `total`, if given, receives their sum.
    // System::CalcKineticEnergy is total.kinetic + total.kinetic_affine, CalcPotentialEnergy is gravity_potential +
    // elastic_in_plane + elastic_normal + elastic_shear + bending.  A synchronisation point.
    std::vector<mpm_cloth_measure_t> Measure(mpm_cloth_measure_t* total = nullptr) const {
        size_t n = 0;
        mpm_check(mpm_cloth_count(h_, &n));
        std::vector<mpm_cloth_measure_t> rows(n);
        mpm_check(mpm_measure(h_, rows.data(), n, &n, total));
        return rows;
    }
    double CalcKineticEnergy() const {
        mpm_cloth_measure_t t;
        mpm_check(mpm_measure(h_, nullptr, 0, nullptr, &t));
        return t.kinetic + t.kinetic_affine;
    }
    double CalcPotentialEnergy() const {
        mpm_cloth_measure_t t;
        mpm_check(mpm_measure(h_, nullptr, 0, nullptr, &t));
        return t.gravity_potential + t.elastic_in_plane + t.elastic_normal + t.elastic_shear + t.bending;
    }
    // (s1, s2, r22, V psi) per face in original face order (mpm_face_strain; single engines only)
    std::vector<float> FaceStrain(size_t n_faces) const {
        expect("FaceStrain", "n_faces", n_faces, this->n_faces());
        std::vector<float> s(4 * n_faces);
        mpm_check(mpm_face_strain(h_, s.data()));
        return s;
    }
    std::vector<Vec3<T>>& positions_host() { return h_positions_; }
    const std::vector<Vec3<T>>& positions_host() const { return h_positions_; }
    ExternalSpatialForce<T>& external_forces_host() { return h_external_forces_; }
    const ExternalSpatialForce<T>& external_forces_host() const { return h_external_forces_; }
    size_t num_external_bodies() const { return n_bodies_; }
    size_t num_contacts() const { return n_contacts_; }
    int total_contact_iteration_count = 0;

  private:
    template <typename U> friend class GpuMpmSolver;
    // the two-call getter of a table: the count, then that many records
    template <class R>
    std::vector<R> table(int (*get)(mpm_handle_t, R*, size_t, size_t*)) const {
        size_t n = 0;
        mpm_check(get(h_, nullptr, 0, &n));
        std::vector<R> out(n);
        mpm_check(get(h_, out.data(), n, &n));
        return out;
    }
    float max_stable_dt(int (*get)(mpm_handle_t, float*)) const {
        float dt = 0.f;
        mpm_check(get(h_, &dt));
        return dt;
    }
    // the evaluators take their extent from the caller, as the reference's signatures do; the C ABI writes the engine's
    // own, so any other number is refused here instead of overrunning (or half filling) the buffer
    static void expect(const char* method, const char* what, size_t given, size_t engine) {
        if (given != engine)
            throw std::invalid_argument(std::string(method) + ": " + what + " is " + std::to_string(given) +
                                        ", the engine has " + std::to_string(engine));
    }
    std::vector<float> vertex_forces(int (*get)(mpm_handle_t, float*), size_t n_verts, const char* method) const {
        expect(method, "n_verts", n_verts, this->n_verts());
        std::vector<float> f(3 * n_verts);
        mpm_check(get(h_, f.data()));
        return f;
    }
    mpm_handle_t h_ = nullptr;
    size_t n_bodies_ = 0, n_contacts_ = 0;
    std::vector<Vec3<T>> h_positions_;
    ExternalSpatialForce<T> h_external_forces_;
};

// cuda_mpm_solver.cuh:19-35 (stateless, all const)
template <typename T>
class GpuMpmSolver {
  public:
    void RebuildMapping(GpuMpmState<T>* s, bool sort) const { mpm_check(mpm_rebuild_mapping(s->h_, sort)); }
    void CalcFemStateAndForce(GpuMpmState<T>* s, const T& dt) const { mpm_check(mpm_calc_fem_state_and_force(s->h_, dt)); }
    void ParticleToGrid(GpuMpmState<T>* s, const T& dt) const { mpm_check(mpm_particle_to_grid(s->h_, dt)); }
    void UpdateGrid(GpuMpmState<T>* s, int mpm_bc = -1) const { mpm_check(mpm_update_grid(s->h_, mpm_bc)); }
    void GridToParticle(GpuMpmState<T>* s, const T& dt) const { mpm_check(mpm_grid_to_particle(s->h_, dt)); }
    void GpuSync() const { mpm_check(mpm_device_synchronize()); }   // cuda_mpm_solver.cu:164-166
    void GpuSync(GpuMpmState<T>* s) const { mpm_check(mpm_sync(s->h_)); }
    void SyncParticleStateToCpu(GpuMpmState<T>* s) const {
        s->h_positions_.resize(s->n_particles());
        mpm_check(mpm_sync_particle_state_to_cpu(s->h_, reinterpret_cast<float*>(s->h_positions_.data())));
    }
    void Dump(const GpuMpmState<T>& s, std::string filename) const { mpm_check(mpm_dump_obj(s.h_, filename.c_str())); }
    void CopyContactPairs(GpuMpmState<T>* s, const MpmParticleContactPairs<T>& c) const {
        s->n_contacts_ = c.size();
        mpm_check(mpm_copy_contact_pairs(s->h_, c.size(), c.particle_in_contact_index.data(), c.non_mpm_id.data(),
                                         c.penetration_distance.data(), reinterpret_cast<const float*>(c.normal.data()),
                                         reinterpret_cast<const float*>(c.particle_in_contact_position.data()),
                                         reinterpret_cast<const float*>(c.rigid_v.data()),
                                         reinterpret_cast<const float*>(c.rigid_p_WB.data())));
    }
    // Extension: CalcMpmContactPairs + CopyContactPairs on the device for bodies with
    // analytic signed distance fields; nothing travels to the host but the pair count.
    size_t GenerateContactPairs(GpuMpmState<T>* s, const std::vector<mpm_collider_t>& colliders) const {
        size_t n = 0;
        mpm_check(mpm_generate_contact_pairs(s->h_, colliders.size(), colliders.data(), &n));
        s->n_contacts_ = n;
        return n;
    }
    // The same without the count: nothing at all travels to the host, UpdateContact works from the device's count
    // (mpm_hip.h, mpm_generate_contact_pairs with n_out = NULL).
    void GenerateContactPairsOnDevice(GpuMpmState<T>* s, const std::vector<mpm_collider_t>& colliders) const {
        mpm_check(mpm_generate_contact_pairs(s->h_, colliders.size(), colliders.data(), nullptr));
    }
    // Extension: QueryObject::ComputeSignedDistanceToPoint for one analytic collider (any of the six kinds) at n world
    // points, by the pair generator's distance function: phi (n) and the unit world gradient (3n) into phi / grad_W.
    void ColliderSignedDistance(const GpuMpmState<T>& s, const mpm_collider_t& c, const std::vector<T>& p_WQ,
                                std::vector<T>* phi, std::vector<T>* grad_W) const {
        const size_t n = p_WQ.size() / 3;
        phi->resize(n);
        grad_W->resize(3 * n);
        mpm_check(mpm_collider_signed_distance(s.h_, &c, n, p_WQ.data(), phi->data(), grad_W->data()));
    }
    // Extension: mesh colliders (a Drake Mesh / Convex: the OBJ's vertices with the scale and X_BG baked in, body frame).
    // The lattice is built once on the device; the set is posed once per step and tested after the analytic colliders
    // by every pair generation.
    uint32_t SdfShapeFromMesh(GpuMpmState<T>* s, const std::vector<float>& verts_B, const std::vector<int32_t>& tris,
                              float cell, int pad_cells = 2) const {
        uint32_t id = 0;
        mpm_check(mpm_sdf_shape_from_mesh(s->h_, verts_B.data(), verts_B.size() / 3, tris.data(), tris.size() / 3, cell,
                                          pad_cells, &id));
        return id;
    }
    void SetSdfColliders(GpuMpmState<T>* s, const std::vector<mpm_sdf_collider_t>& colliders) const {
        mpm_check(mpm_set_sdf_colliders(s->h_, colliders.size(), colliders.data()));
    }
    // Extension: contact material per rigid body (Drake keeps coulomb_friction, point_stiffness and
    // hunt_crossley_dissipation in the ProximityProperties of a geometry).  materials[b] belongs to body b; a field < 0
    // and every body >= materials.size() take what UpdateContact / RunCoupledSubsteps pass.  An empty vector clears the
    // table.  Once per plant step at most; every solve enqueued afterwards uses it.  See mpm_set_body_contact_materials.
    void SetBodyContactMaterials(GpuMpmState<T>* s, const std::vector<mpm_contact_material_t>& materials) const {
        mpm_check(mpm_set_body_contact_materials(s->h_, materials.size(), materials.data()));
    }
    std::vector<mpm_contact_material_t> GetBodyContactMaterials(const GpuMpmState<T>& s) const {
        size_t n = 0;
        mpm_check(mpm_get_body_contact_materials(s.h_, nullptr, 0, &n));
        std::vector<mpm_contact_material_t> out(n);
        mpm_check(mpm_get_body_contact_materials(s.h_, out.data(), n, &n));
        return out;
    }
    void SdfColliderSignedDistance(const GpuMpmState<T>& s, const mpm_sdf_collider_t& c, const std::vector<T>& p_WQ,
                                   std::vector<T>* phi, std::vector<T>* grad_W) const {
        const size_t n = p_WQ.size() / 3;
        phi->resize(n);
        grad_W->resize(3 * n);
        mpm_check(mpm_sdf_collider_signed_distance(s.h_, &c, n, p_WQ.data(), phi->data(), grad_W->data()));
    }
    size_t ContactPairCount(GpuMpmState<T>* s) const {
        size_t n = 0;
        mpm_check(mpm_get_contact_pair_count(s->h_, &n));
        s->n_contacts_ = n;
        return n;
    }
    // Extension: the body of DeformableDriver::CalcAbstractStates' loop (deformable_driver.h:240-258) n times in one
    // call, for bodies with analytic signed distance fields: RebuildMapping, CalcFemStateAndForce, ParticleToGrid,
    // UpdateGrid, pairs on the device, UpdateContact, GridToParticle.  Same results as the seven calls.
    std::vector<mpm_coupled_result_t> RunCoupledSubsteps(GpuMpmState<T>* s, int n, const T& dt, int mpm_bc, const T& friction_mu,
                                                         const T& stiffness, const T& damping, bool exact_line_search,
                                                         const std::vector<mpm_collider_t>& colliders) const {
        mpm_coupled_params_t p{};
        p.dt = dt; p.mpm_bc = mpm_bc; p.friction_mu = friction_mu; p.stiffness = stiffness; p.damping = damping;
        p.exact_line_search = exact_line_search ? 1 : 0;
        p.max_newton_iterations = 0;
        std::vector<mpm_coupled_result_t> r(n > 0 ? size_t(n) : 0);
        mpm_check(mpm_run_coupled_substeps(s->h_, n, &p, colliders.size(), colliders.data(), r.data()));
        for (const auto& q : r) s->total_contact_iteration_count += q.iterations;
        if (!r.empty()) s->n_contacts_ = r.back().contacts;
        return r;
    }
    // Extension: the arithmetic of CalcFemStateAndForce (correctly rounded by default, like the reference's build).
    void SetFastMath(GpuMpmState<T>* s, bool on) const { mpm_check(mpm_set_fast_math(s->h_, on ? 1 : 0)); }
    void DownloadContactPairs(const GpuMpmState<T>& s, MpmParticleContactPairs<T>* c) const {
        // the engine writes the pairs it holds: its own count, not the one this object last heard of (none after
        // GenerateContactPairsOnDevice, an older one after a call made through another copy of the state)
        size_t n = 0;
        mpm_check(mpm_get_contact_pair_count(s.h_, &n));
        c->particle_in_contact_index.resize(n); c->non_mpm_id.resize(n); c->penetration_distance.resize(n);
        c->normal.resize(n); c->particle_in_contact_position.resize(n); c->rigid_v.resize(n); c->rigid_p_WB.resize(n);
        mpm_check(mpm_download_contact_pairs(s.h_, c->particle_in_contact_index.data(), c->non_mpm_id.data(),
                                             c->penetration_distance.data(), reinterpret_cast<float*>(c->normal.data()),
                                             reinterpret_cast<float*>(c->particle_in_contact_position.data()),
                                             reinterpret_cast<float*>(c->rigid_v.data()),
                                             reinterpret_cast<float*>(c->rigid_p_WB.data())));
    }
    void UpdateContact(GpuMpmState<T>* s, const int frame, const int substep, const T& dt, const T& friction_mu,
                       const T& stiffness, const T& damping, const bool dump, const bool exact_line_search) const {
        int it = 0;
        float res = 0;
        mpm_check(mpm_update_contact(s->h_, frame, substep, dt, friction_mu, stiffness, damping, dump,
                                     exact_line_search, 0, &it, &res));
        s->total_contact_iteration_count += it;
    }
};

// ---- rigid feedback wire format: the three steps either side of the substep loop --------------

// DeformableDriver::InitalizeExternalContactForces (multibody/plant/deformable_driver.h:196-208):
// size and zero the per-body accumulators; p_BoBq_B temporarily carries the body origins in the
// world (the reference stores EvalBodyPoseInWorld(...).translation() there for the contact-pair
// generator and clears it again in Finalize).
template <typename T>
inline void InitalizeExternalContactForces(GpuMpmState<T>* s, const std::vector<Vec3<T>>& body_origins_W) {
    s->ReallocateExternelBodies(body_origins_W.size());
    auto& F = s->external_forces_host();
    F.resize(body_origins_W.size());
    for (size_t i = 0; i < F.size(); ++i) {
        F.p_BoBq_B[i] = body_origins_W[i];
        F.F_Bq_W_tau[i] = {0, 0, 0};
        F.F_Bq_W_f[i] = {0, 0, 0};
    }
}

// DeformableDriver::FinalizeExternalContactForces (deformable_driver.h:210-219): impulses of the
// plant step dt -> forces, p_BoBq_B reset to zero (the torques are already about the body origins).
template <typename T>
inline void FinalizeExternalContactForces(GpuMpmState<T>* s, const T& dt) {
    auto& F = s->external_forces_host();
    F.resize(s->num_external_bodies());
    mpm_check(mpm_finalize_external_contact_forces(s->handle(), dt, reinterpret_cast<float*>(F.F_Bq_W_tau.data()),
                                                   reinterpret_cast<float*>(F.F_Bq_W_f.data())));
    for (auto& p : F.p_BoBq_B) p = {0, 0, 0};
}

// The MPM block of MultibodyPlant::AddAppliedExternalSpatialForces (multibody_plant.cc:2385-2407):
// F_BBo_W_array[i] += SpatialForce(tau_i, f_i).Shift(-(R_WB_i * p_BoBq_B_i)).  R_WB row major.
template <typename T>
inline void AddAppliedExternalSpatialForces(const GpuMpmState<T>& s, const std::vector<std::array<T, 9>>& R_WB,
                                            std::vector<Vec3<T>>* tau_BBo_W, std::vector<Vec3<T>>* f_BBo_W) {
    const auto& F = s.external_forces_host();
    const size_t n = F.size();
    if (R_WB.size() != n || tau_BBo_W->size() != n || f_BBo_W->size() != n)
        throw std::logic_error("AddAppliedExternalSpatialForces: one pose and one spatial force slot per body");
    std::vector<Vec3<T>> shifted(n);
    mpm_check(mpm_external_forces_at_body_origin(n, reinterpret_cast<const float*>(R_WB.data()),
                                                 reinterpret_cast<const float*>(F.p_BoBq_B.data()),
                                                 reinterpret_cast<const float*>(F.F_Bq_W_tau.data()),
                                                 reinterpret_cast<const float*>(F.F_Bq_W_f.data()),
                                                 reinterpret_cast<float*>(shifted.data())));
    for (size_t i = 0; i < n; ++i)
        for (int d = 0; d < 3; ++d) {
            (*tau_BBo_W)[i][d] += shifted[i][d];
            (*f_BBo_W)[i][d] += F.F_Bq_W_f[i][d];
        }
}

}  // namespace gmpm
}  // namespace multibody
}  // namespace drake
