// Host side of the engine and the C ABI declared in include/mpm_hip.h.
// One translation unit: the kernels are header-only so hipcc can inline the
// device math into them.
// This file holds EVERY entry point of the C ABI, the substep's launch sequence (launch_*, enqueue_substep_front / _rest),
// settle and the deferral of phase calls, the halo entry points and the run, profile and coupled drivers.  What a feature
// does behind its entry points is in the feature's host header (mpm_io.h, mpm_contact.h, mpm_cloth_host.h,
// mpm_bodies_host.h, mpm_dist_host.h, mpm_chain_host.h): an entry point here checks its arguments and makes one call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <functional>
#include <mutex>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

#include "../../include/mpm_hip.h"
#include "mpm_host.h"
#include "mpm_io.h"
#include "mpm_debug_tables.h"
#include "mpm_contact.h"
#include "mpm_chain.h"
#include "mpm_feedback.h"
#include "mpm_dist.h"
#include "mpm_cloth_host.h"
#include "mpm_bodies_host.h"
#include "mpm_dist_host.h"
#include "mpm_chain_host.h"

// every engine alive in this process (mpm_device_synchronize)
static std::mutex g_live_mutex;
static std::vector<mpm_engine*> g_live;

extern "C" {

const char* mpm_last_error(void) { return g_last_error.c_str(); }

int mpm_default_material(mpm_material_t* m) try {
    REQUIRE(m, "null material");
    m->youngs_modulus = 400000.f;
    m->poisson_ratio = .3f;
    m->density = 2000.f;
    m->gamma = 0.f;
    m->K = 100000.f;
    m->V = .8f;
    m->c_F = 0.f;
    m->sdf_friction = .3f;
    m->gravity = -9.8f;
    m->epsv = 1e-3f;
    m->gravity_axis = 2;
    m->wall_cells = 3;
    return 0;
} MPM_CATCH_ALL

int mpm_create(int domain_bits, const mpm_material_t* material, int device, mpm_handle_t* out) try {
    REQUIRE(out, "null handle pointer");
    REQUIRE(domain_bits >= 4 && domain_bits <= 8, "domain_bits must be in [4,8] (16^3 .. 256^3 cells)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(MPM_ERR_NO_DEVICE, "no HIP device visible: the engine has no CPU fallback");
    REQUIRE(device >= 0 && device < ndev, "device ordinal out of range");
    mpm_engine* e = new mpm_engine();
    e->device = device;
    e->bits = domain_bits;
    if (material) e->mat = *material; else mpm_default_material(&e->mat);
    if (e->mat.gravity_axis < 0 || e->mat.gravity_axis > 2) {
        delete e;
        return fail(MPM_ERR_INVALID, "gravity_axis must be 0, 1 or 2");
    }
    hipError_t err = hipSetDevice(device);
    if (err == hipSuccess) err = hipStreamCreateWithFlags(&e->own_stream, hipStreamNonBlocking);
    if (err != hipSuccess) {
        delete e;
        return fail(MPM_ERR_HIP, std::string("mpm_create: ") + hipGetErrorString(err));
    }
    e->stream = e->own_stream;
    if (getenv("MPM_RESORT_EVERY")) e->check_every = std::max(1, atoi(getenv("MPM_RESORT_EVERY")));
    if (getenv("MPM_DEFER_PHASES")) e->defer_phases = atoi(getenv("MPM_DEFER_PHASES")) != 0;
    if (getenv("MPM_QUIET_FACTOR")) e->quiet_factor = std::min(1.f, std::max(0.f, (float)atof(getenv("MPM_QUIET_FACTOR"))));
    {
        std::lock_guard<std::mutex> lock(g_live_mutex);
        g_live.push_back(e);
    }
    *out = e;
    return 0;
} MPM_CATCH_ALL

// (m: the cloth's own material, or null for the engine's; checked by the caller.  Nothing is recorded on a refusal.)
static int add_cloth(mpm_engine* e, const float* pos, const float* vel, size_t n_verts, const int32_t* indices,
                     size_t n_faces, const mpm_cloth_material_t* m) {
    REQUIRE(e, "null handle");
    REQUIRE(!e->finalized, "AddQRCloth after Finalize");
    REQUIRE(pos && vel && (indices || n_faces == 0), "null input array");
    for (size_t i = 0; i < n_faces * 3; ++i)
        REQUIRE(indices[i] >= 0 && (size_t)indices[i] < n_verts, "triangle index out of range");
    REQUIRE(!(e->multi_mat || m) || e->cloths.size() < MAX_CLOTH_MATERIALS,
            "more than 256 cloths in a multi-material engine (mpm_add_qr_cloth_with_material)");
    mpm_engine::Cloth c{e->nv, n_verts, e->nf, n_faces, {}};
    c.m = m ? *m : engine_cloth_material(e);
    e->cloths.push_back(c);
    if (m) e->multi_mat = true;
    for (size_t i = 0; i < n_faces * 3; ++i) e->h_idx.push_back(indices[i] + (int)e->nv);
    e->h_pos.insert(e->h_pos.end(), pos, pos + 3 * n_verts);
    e->h_vel.insert(e->h_vel.end(), vel, vel + 3 * n_verts);
    e->nv += n_verts;
    e->nf += n_faces;
    e->np = e->nv + e->nf;
    return 0;
}

int mpm_add_qr_cloth(mpm_handle_t e, const float* pos, const float* vel, size_t n_verts, const int32_t* indices,
                     size_t n_faces) try {
    return add_cloth(e, pos, vel, n_verts, indices, n_faces, nullptr);
} MPM_CATCH_ALL

int mpm_add_qr_cloth_with_material(mpm_handle_t e, const float* pos, const float* vel, size_t n_verts,
                                   const int32_t* indices, size_t n_faces, const mpm_cloth_material_t* m) try {
    REQUIRE(e, "null handle");
    const mpm_cloth_material_t c = m ? *m : engine_cloth_material(e);
    REQUIRE(std::isfinite(c.youngs_modulus) && std::isfinite(c.poisson_ratio) && std::isfinite(c.density) &&
                std::isfinite(c.gamma) && std::isfinite(c.K) && std::isfinite(c.c_F),
            "cloth material: a field is not finite");
    REQUIRE(c.youngs_modulus > 0.f, "cloth material: youngs_modulus must be > 0");
    REQUIRE(c.poisson_ratio >= 0.f && c.poisson_ratio < .5f, "cloth material: poisson_ratio must be in [0, 0.5)");
    REQUIRE(c.density > 0.f, "cloth material: density must be > 0");
    REQUIRE(c.gamma >= 0.f && c.K >= 0.f && c.c_F >= 0.f, "cloth material: gamma, K and c_F must be >= 0");
    return add_cloth(e, pos, vel, n_verts, indices, n_faces, &c);
} MPM_CATCH_ALL

int mpm_cloth_count(mpm_handle_t e, size_t* n_out) try {
    REQUIRE(e && n_out, "null argument");
    *n_out = e->cloths.size();
    return 0;
} MPM_CATCH_ALL

int mpm_get_cloth_info(mpm_handle_t e, size_t cloth, size_t* first_vertex, size_t* n_verts, size_t* first_face,
                       size_t* n_faces, mpm_cloth_material_t* m) try {
    REQUIRE(e, "null handle");
    REQUIRE(cloth < e->cloths.size(), "cloth index out of range");
    const mpm_engine::Cloth& c = e->cloths[cloth];
    if (first_vertex) *first_vertex = c.first_vertex;
    if (n_verts) *n_verts = c.n_verts;
    if (first_face) *first_face = c.first_face;
    if (n_faces) *n_faces = c.n_faces;
    if (m) *m = c.m;
    return 0;
} MPM_CATCH_ALL

// The conditional re-sort.  lean: CalcFemStateAndForce follows at once (DP::lean_resort).  dt: the length of the substep the
// launches belong to, where there is one -- the anticipatory binning then uses it; the last known length stays otherwise.
// (The block tables may change: the contact solve's guess of how many blocks are active survives that, k_ct_keys verifies
// it on the device.)
static void launch_rebuild(mpm_engine* e, DP p, bool lean, float dt) {
    if (dt > 0.f) e->last_dt = dt;
    p.anticip = e->anticipation();
    p.lean_resort = lean && !p.dist.on;
    e->checks_launched += 1;
    TraceRange tr("mpm:RebuildMapping (conditional re-sort)");
    hipLaunchKernelGGL(k_rb_count, dim3(std::min(e->g_np, e->g_rb)), dim3(256), 0, e->stream, p);
    hipLaunchKernelGGL(k_rb_tables, dim3(33), dim3(1024), 0, e->stream, p);
    hipLaunchKernelGGL(k_rb_scatter, dim3(std::min(e->g_np, e->g_rb)), dim3(256), 0, e->stream, p);
    if (e->deterministic) hipLaunchKernelGGL(k_rb_canon, dim3(512), dim3(256), 0, e->stream, p);
    hipLaunchKernelGGL(k_rb_finish, dim3((std::min(e->g_np, e->g_rb) + 7u) & ~7u), dim3(256), 0, e->stream, p);
}

// The launch helpers below take the DP of the launch: e->dp, or a copy of it with the per-launch fields set (DP::lean_g2p,
// gated, watch_base, halo_hdr, halo_*).  Nothing writes those fields of e->dp itself.
static void launch_fem_faces(mpm_engine* e, const DP& p, float dt) {
    TraceRange tr("mpm:CalcFemStateAndForce (faces)");
    if (!e->nf) return;
    const dim3 g((e->g_nf + 7u) & ~7u), b(256);
    if (e->multi_mat) {   // (per-cloth materials, mpm_add_qr_cloth_with_material)
        const ClothMat* t = e->d_cloth_mat;
        if (e->fast_math) hipLaunchKernelGGL(k_fem_mat<1>, g, b, 0, e->stream, p, dt, t);
        else hipLaunchKernelGGL(k_fem_mat<0>, g, b, 0, e->stream, p, dt, t);
    } else if (e->fast_math) hipLaunchKernelGGL(k_fem<1>, g, b, 0, e->stream, p, dt);
    else hipLaunchKernelGGL(k_fem<0>, g, b, 0, e->stream, p, dt);
    // (an engine with a weave, mpm_set_weave: the same faces again, adding to the records just written.  The order k_fem,
    // k_weave, k_damp is part of the result: a record is the float sum in that order)
    if (e->weave.on()) hipLaunchKernelGGL(k_weave, g, b, 0, e->stream, p, e->weave.args);
    // (an engine with membrane damping, mpm_set_damping: the same faces once more)
    if (e->damp.membrane()) hipLaunchKernelGGL(k_damp, g, b, 0, e->stream, p, e->damp.args);
    // (an engine with a tear limit or a torn face, mpm_set_tearing / mpm_set_torn_faces: last, it owns a torn face's records)
    if (e->tear.on()) hipLaunchKernelGGL(k_tear, g, b, 0, e->stream, p, e->tear.args);
}
static void launch_fem_vertices(mpm_engine* e, const DP& p, float dt) {
    TraceRange tr("mpm:CalcFemStateAndForce (vertex forces)");
    // (the instance that reads as many planes of DP::VF as the meshes' largest valence needs: vf_planes_of)
    if (e->nv) {
        const dim3 g((e->g_nv + 7u) & ~7u), b(256);
        if (vf_planes_of(e->max_valence) == VF_PLANES_REGULAR) hipLaunchKernelGGL(k_vforce<VF_PLANES_REGULAR>, g, b, 0, e->stream, p);
        else hipLaunchKernelGGL(k_vforce<VF_PLANES_ALL>, g, b, 0, e->stream, p);
    }
    // (an engine with bending stiffness, mpm_set_bending: f += -k Q x on the forces k_vforce has just written)
    if (e->bend.on()) hipLaunchKernelGGL(k_bend, rows_grid(e->bend.args.n_rows), dim3(256), 0, e->stream, p, e->bend.args);
    // (... and with bending damping, mpm_set_damping: f += -beta k Q v from the same table)
    if (e->bend.on() && e->damp.bending())
        hipLaunchKernelGGL(k_bend_damp, rows_grid(e->bend.args.n_rows), dim3(256), 0, e->stream, p, e->bend.args,
                           (const float*)e->damp.d_beta_vertex);
    // (an engine with links, mpm_set_links: f += the seams', springs' and cords' forces, one lane per linked vertex; while
    // some link has a break limit or is broken, mpm_set_link_limits / mpm_set_broken_links, k_link_break first: one lane
    // per link, it owns a broken link's two records)
    if (e->links.on() && e->links.breaking())
        hipLaunchKernelGGL(k_link_break, rows_grid(e->links.brk.n), dim3(256), 0, e->stream, p, e->links.brk);
    if (e->links.on()) hipLaunchKernelGGL(k_link, rows_grid(e->links.args.n_rows), dim3(256), 0, e->stream, p, e->links.args);
    // (an engine with pressure, mpm_set_pressure: where a cloth is in gas mode, the gas cloths' volumes and gauge pressures
    // from the current positions, on the device; then f += the pressure force, one lane per vertex of a pressurised cloth)
    // TEARING COMPOSED WITH GAS AND SHELL BENDING (mpm_set_tear_coupling).  The order is part of the result: k_tear ran LAST
    // in launch_fem_faces, in front of every kernel here, so the tear flags these kernels read are this substep's -- a face
    // that fails in a substep vents its cloth (k_pressure_volume, k_pressure_gauge) and cuts its hinges (k_crease, k_hinge)
    // in that same substep, whatever the particle order and the determinism mode; a substep that skips itself marks
    // nothing and changes nothing.  The pointer to the flags goes into a copy of the arguments per launch
    // (pressure_volume_args, crease_args, hinge_args) and is null while the mode is off: the launches of an engine without it.
    if (e->pressure.on()) {
        const mpm_engine::Pressure& ps = e->pressure;
        if (ps.gas()) {
            PressureVolumeArgs va = pressure_volume_args(e);
            va.ranges = ps.d_ranges_gas;
            va.only_gas = 1;
            hipLaunchKernelGGL(k_pressure_volume, dim3((unsigned)ps.n_gas_chunks), dim3(256), 0, e->stream, p, va, 0);
            hipLaunchKernelGGL(k_pressure_gauge, dim3((unsigned)e->cloths.size()), dim3(64), 0, e->stream, p, va);
        }
        hipLaunchKernelGGL(k_pressure, rows_grid(ps.args.n_rows), dim3(256), 0, e->stream, p, ps.args);
    }
    // (an engine with shell bending, mpm_set_shell_bending: the corner records of every hinge, one lane per hinge; then
    // f += the records of every vertex, one lane per vertex of a cloth with k > 0; while some cloth creases or some hinge
    // is creased, mpm_set_creases / mpm_set_crease_state, k_crease first: one lane per hinge, it owns the psibar k_hinge reads;
    // while some cloth's hinges are damped, mpm_set_shell_damping, k_hinge<1> in k_hinge<0>'s place: no further launch)
    if (e->shell.on() && e->shell.creasing())
        hipLaunchKernelGGL(k_crease, rows_grid(e->shell.cr.n), dim3(256), 0, e->stream, p, crease_args(e));
    if (e->shell.on()) {
        if (e->shell.damped()) hipLaunchKernelGGL(k_hinge<1>, rows_grid(e->shell.hinge.n), dim3(256), 0, e->stream, p, hinge_args(e));
        else hipLaunchKernelGGL(k_hinge<0>, rows_grid(e->shell.hinge.n), dim3(256), 0, e->stream, p, hinge_args(e));
        hipLaunchKernelGGL(k_hinge_gather, rows_grid(e->shell.args.n_rows), dim3(256), 0, e->stream, p, e->shell.args);
    }
    // (an engine with anchors, mpm_set_anchors: the bodies' poses at their clocks, one lane per motion; then f += the
    // springs' and cords' forces, one lane per anchored vertex, and the reactions into the bodies' accumulators)
    if (e->anchors.on()) {
        const AnchorArgs a = anchors_posed(e);
        const AnchorAcc acc{e->cb.body_acc, (int)e->cb.n_bodies, p.fix_p};
        hipLaunchKernelGGL(k_anchor, rows_grid(a.n_rows), dim3(256), 0, e->stream, p, a, acc, dt);
    }
}
// (mpm_calc_fem_state_and_force: the two FEM kernels, whose forces a caller may read)
static void launch_fem(mpm_engine* e, const DP& p, float dt) {
    e->last_dt = dt;
    launch_fem_faces(e, p, dt);
    launch_fem_vertices(e, p, dt);
}
// `forces`: where k_p2g's vertex lanes find the force on their vertex (the kernel's template parameter: 0 = in p.f,
// k_vforce ran; 1 = summed inside the kernel)
static void launch_p2g(mpm_engine* e, const DP& p, float dt, int forces = 0) {
    TraceRange tr(forces ? "mpm:ParticleToGrid (+ vertex forces)" : "mpm:ParticleToGrid");
    const dim3 g(e->g_tile), b(P2G_THREADS);
    // (deterministic mode accumulates in fixed point: exact sums whatever the order of arrival, see k_p2g's EXACT)
    const bool exact = e->deterministic || e->p2g_fixed_point;
    // (V: the planes of DP::VF the vertex lanes read, from the meshes' largest valence -- vf_planes_of; only the
    // FORCES = 1 instances read them)
#define MPM_P2G_LAUNCH(F, V)                                                                       \
    do {                                                                                           \
        if (exact) hipLaunchKernelGGL((k_p2g<F, 1, 0, V>), g, b, 0, e->stream, p, dt);             \
        else hipLaunchKernelGGL((k_p2g<F, 0, 0, V>), g, b, 0, e->stream, p, dt);                   \
    } while (0)
    // (an engine with a table of force fields: the instances that evaluate it, mpm_set_force_fields)
#define MPM_P2G_LAUNCH_FIELDS(F, V)                                                                                   \
    do {                                                                                                              \
        const ForceFieldTable* t = e->d_force_fields;                                                                 \
        if (exact) hipLaunchKernelGGL((k_p2g<F, 1, 1, V, ForceFieldTable>), g, b, 0, e->stream, p, dt, t);     \
        else hipLaunchKernelGGL((k_p2g<F, 0, 1, V, ForceFieldTable>), g, b, 0, e->stream, p, dt, t);           \
    } while (0)
    const bool regular = vf_planes_of(e->max_valence) == VF_PLANES_REGULAR;
    if (!e->force_fields.empty()) {
        if (forces == 1 && regular) MPM_P2G_LAUNCH_FIELDS(1, VF_PLANES_REGULAR);
        else if (forces == 1) MPM_P2G_LAUNCH_FIELDS(1, VF_PLANES_ALL);
        else MPM_P2G_LAUNCH_FIELDS(0, VF_PLANES_ALL);
    } else if (forces == 1 && regular) MPM_P2G_LAUNCH(1, VF_PLANES_REGULAR);
    else if (forces == 1) MPM_P2G_LAUNCH(1, VF_PLANES_ALL);
    else MPM_P2G_LAUNCH(0, VF_PLANES_ALL);
#undef MPM_P2G_LAUNCH_FIELDS
#undef MPM_P2G_LAUNCH
}
// the vertex forces inside k_p2g, from the vertices' entries of DP::VF (single and partitioned domains alike since round
// 5); a mesh with a vertex of more than eight faces keeps the k_vforce launch, and so does an engine with a feature whose
// kernel adds to the forces in DP::f (FeatureRow::adds_to_f, mpm_features.h)
static int fused_forces(const mpm_engine* e) { return forces_fusable(feature_state(e), e->max_valence) ? 1 : 0; }
// the pins behind GridToParticle (k_pin, mpm_pins.h); only an engine with pins or anchors launches it (pins_ready has
// resolved the table).  An engine with anchors and no pins launches it with zero pins and one workgroup: its tail
// advances the bodies' clocks.  Everything after GridToParticle -- the coupled path's watch kernel included -- comes
// after it on the stream.
static void launch_pins(mpm_engine* e, const DP& p, float dt) {
    TraceRange tr("mpm:Pins");
    const mpm_engine::PinState& ps = e->pin;
    PinArgs a{ps.d_pins, (int)ps.set.size(), ps.d_mot, (int)ps.motion_body.size(), e->cb.body_acc, (int)e->cb.n_bodies,
              p.fix_p, ps.d_ticket};
    const unsigned groups = (unsigned)std::max<size_t>(1, std::min<size_t>((ps.set.size() + 255) / 256, 1024));
    hipLaunchKernelGGL(k_pin, dim3(groups), dim3(256), 0, e->stream, p, a, dt);
}
// (`p` may carry a halo class restriction: only an engine without pins splits GridToParticle, see extensions_refused)
static void launch_g2p(mpm_engine* e, const DP& p, float dt) {
    TraceRange tr("mpm:GridToParticle");
    hipLaunchKernelGGL(k_g2p, dim3(std::min(768u, p.capI)), dim3(G2P_THREADS), 0, e->stream, p, dt);
    if ((!e->pin.set.empty() || e->anchors.on()) && p.halo_cls < 0) launch_pins(e, p, dt);
}
static void launch_grid(mpm_engine* e, const DP& p, const GridColliders& gc) {
    TraceRange tr("mpm:UpdateGrid");
    if (gc.n < 0) {   // MPM_BC_BODIES with a table (grid_colliders_for): the instance the table needs
        const dim3 g(e->g_grid), b(256);
        const GridBodyTable* t = e->d_grid_bodies;
        long long* acc = e->cb.body_acc;
        const int nb = (int)e->cb.n_bodies;
        switch (e->grid_bodies_kinds) {
            case 0: hipLaunchKernelGGL(k_grid_bodies<0>, g, b, 0, e->stream, p, t, acc, nb); break;
            case 1: hipLaunchKernelGGL(k_grid_bodies<1>, g, b, 0, e->stream, p, t, acc, nb); break;
            case 2: hipLaunchKernelGGL(k_grid_bodies<2>, g, b, 0, e->stream, p, t, acc, nb); break;
            default: hipLaunchKernelGGL(k_grid_bodies<3>, g, b, 0, e->stream, p, t, acc, nb); break;
        }
        return;
    }
    hipLaunchKernelGGL(k_grid<1>, dim3(e->g_grid), dim3(256), 0, e->stream, p, gc);
}

// ---- the substep's kernel sequence, stated once --------------------------------------------------------------------------
// Every entry point that runs a substep enqueues it through the two functions below, each from the DP of the launch (e->dp,
// or a copy with the per-launch fields set); only the phase-by-phase calls, whose separate kernels are their contract,
// launch FEM and ParticleToGrid themselves.  `mark`, where given, is called with the number of every phase of
// mpm_profile_substeps' list as its launches end.
using PhaseMark = std::function<void(int)>;
// the re-sort launches in front of a substep: none; lean (FEM follows at once); all of them; the held-back RebuildMapping(false)
// of the phase-by-phase calls, which came before its substep's dt and keeps the last known length for its binning
enum class Resort { None, Lean, Full, Held };
// The front: re-sort launches if asked, FEM faces, vertex forces (and bending) as kernels of their own unless ParticleToGrid
// computes them (fused_forces), ParticleToGrid.
static void enqueue_substep_front(mpm_engine* e, const DP& p, float dt, Resort resort, const PhaseMark& mark = {}) {
    if (resort != Resort::None) launch_rebuild(e, p, resort == Resort::Lean, resort == Resort::Held ? 0.f : dt);
    e->last_dt = dt;
    if (mark) mark(MPM_PHASE_REBUILD);
    launch_fem_faces(e, p, dt);
    if (mark) mark(MPM_PHASE_FEM);
    const int forces = fused_forces(e);
    if (!forces) launch_fem_vertices(e, p, dt);
    if (mark) mark(MPM_PHASE_VFORCE);
    launch_p2g(e, p, dt, forces);
    if (mark) mark(MPM_PHASE_P2G);
}
// The rest: the grid kernel in one of three forms -- the fused update (launch_grid), the gather of the raw sums (a halo
// exchange follows), the update from sums -- from `pg`, then GridToParticle from `*p2`.  p2 == nullptr: no GridToParticle
// (the gather; a coupled substep, whose contact solve comes first and which launches it itself).
enum class GridForm { Fused, Gather, FromSums };
static void enqueue_substep_rest(mpm_engine* e, GridForm form, const DP& pg, const GridColliders& gc, const DP* p2, float dt,
                                 const PhaseMark& mark = {}) {
    const dim3 g(e->g_grid), b(256);
    switch (form) {
        case GridForm::Fused: launch_grid(e, pg, gc); break;
        case GridForm::Gather: hipLaunchKernelGGL(k_grid<0>, g, b, 0, e->stream, pg, GridColliders{}); break;
        case GridForm::FromSums: hipLaunchKernelGGL(k_grid<2>, g, b, 0, e->stream, pg, gc); break;
    }
    if (mark) mark(MPM_PHASE_GRID);
    if (!p2) return;
    launch_g2p(e, *p2, dt);
    if (mark) mark(MPM_PHASE_G2P);
}

// The P2G tiles accumulate in 64-bit fixed point.  Scales are powers of two chosen from the
// total particle mass M: a node can never hold more than M, and its momentum is allowed
// |v| < 2^15 length units per time unit.  Resolution: M * 2^-61 (mass), M * 2^-47 (momentum).
static int set_fixed_point_scales(mpm_engine* e) {
    DP& p = e->dp;
    // (slot space: the whole scene, or -- rare: volumes uploaded to a partitioned engine -- what this rank holds;
    // the scales of mpm_finalize are the whole scene's on every rank, which keeps ghost copies bit-identical)
    const size_t slots = (size_t)p.Np;
    std::vector<float> q0(slots * 4);
    HIP_TRY(hipStreamSynchronize(e->stream));
    Ctl c;
    D2H(e, &c, p.ctl, sizeof(Ctl));
    D2H(e, q0.data(), p.set[c.cur & 1].q[0], slots * 16);
    double mass = 0;
    for (size_t i = 0; i < slots; ++i) mass += std::fabs((double)q0[i * 4 + 3]) * p.M.density;
    if (!(mass > 0) || !std::isfinite(mass)) mass = 1.0;
    const int k = 61 - (int)std::ceil(std::log2(mass));
    p.fix_m = std::ldexp(1.0, k);
    p.fix_p = std::ldexp(1.0, k - 14);
    p.unfix_m = 1.0 / p.fix_m;
    p.unfix_p = 1.0 / p.fix_p;
    return 0;
}

int mpm_finalize(mpm_handle_t e) try {
    REQUIRE(e, "null handle");
    REQUIRE(!e->finalized, "Finalize called twice");
    REQUIRE(e->np > 0, "no particles: call mpm_add_qr_cloth first");
    if (int rc = use(e)) return rc;
    const size_t np = e->np, nf = e->nf, nv = e->nv;
    REQUIRE(np < (size_t)1 << 30, "too many particles");
    DP& p = e->dp;
    p.Np = (int)np; p.Nf = (int)nf; p.Nv = (int)nv;
    p.NpG = (int)np; p.NfG = (int)nf;
    p.bits = e->bits;
    p.dbg = getenv("MPM_DBG") ? atoi(getenv("MPM_DBG")) : 0;
    p.nb = 1 << (e->bits - 2);
    p.ncells = 1u << (3 * e->bits);
    p.nblocks = p.ncells >> 6;
    p.capH = (unsigned)std::min<size_t>(p.nblocks, np);
    p.capA = (unsigned)std::min<size_t>(p.nblocks, (size_t)27 * p.capH);
    p.halo_cls = -1;
    p.fem_fast = e->fast_math ? 1 : 0;
    p.item_groups = getenv("MPM_ITEM_GROUPS") ? std::max(1, atoi(getenv("MPM_ITEM_GROUPS"))) : 48;
    p.item_groups_small = getenv("MPM_ITEM_GROUPS_SMALL") ? std::max(1, atoi(getenv("MPM_ITEM_GROUPS_SMALL"))) : 16;
    p.item_small_below = getenv("MPM_ITEM_SMALL_BELOW") ? atoi(getenv("MPM_ITEM_SMALL_BELOW")) : 6500;
    p.capI = p.capH + (unsigned)(np / (64 * (size_t)std::min(p.item_groups, p.item_groups_small))) + 16u;
    // Slabs (16 KB each) are allocated for the blocks a cloth of this size typically occupies, not for
    // the worst case of one particle per block (capI: 4 GB at 256^3, 33 GB at 512^3); mpm_sync and
    // mpm_get_stats double the pool when it is more than half full (slab_pool_grow).
    p.capS = (unsigned)std::min<size_t>(p.capI, std::max<size_t>(4096, np / 256 + 1024 + np / (64 * (size_t)p.item_groups)));
    if (getenv("MPM_SLAB_CAPACITY")) p.capS = (unsigned)std::min<size_t>(p.capI, std::max(1, atoi(getenv("MPM_SLAB_CAPACITY"))));
    p.dxinv = (float)(1 << e->bits);
    p.dx = 1.f / p.dxinv;
    p.Dinv = 4.f * p.dxinv * p.dxinv;
    const mpm_material_t& m = e->mat;
    lame(m.youngs_modulus, m.poisson_ratio, &p.M.mu, &p.M.lambda);
    p.M.density = m.density; p.M.gamma = m.gamma; p.M.K = m.K; p.M.V = m.V; p.M.cF = m.c_F;
    // a multi-material engine stores each particle's mass in q[0].w (k_init_masses below, k_fem_mat for the faces):
    // every reader that multiplies q[0].w by DP::M.density then gets it unchanged
    if (e->multi_mat) p.M.density = 1.f;
    p.M.sdf_friction = m.sdf_friction; p.M.gravity = m.gravity; p.M.epsv = m.epsv;
    p.M.gravity_axis = m.gravity_axis; p.M.wall = m.wall_cells;

    // ---- device buffers ---------------------------------------------------
    int rc = 0;
    p.q_stride = (unsigned)((np + 63) & ~(size_t)63);
    p.f_stride = (unsigned)((np + 63) & ~(size_t)63);
#define ALLOC(ptr, n, zero)                         \
    if ((rc = e->dalloc(&(ptr), (n), (zero)))) return rc
    ALLOC(p.ctl, 1, true);
    ALLOC(p.dbgbuf, 16, true);
    for (int s = 0; s < 2; ++s) {
        PSet& S = p.set[s];
        // (the four particle planes in one allocation, q_stride apart: k_p2g addresses them from ONE base
        // pointer -- it runs out of scalar registers otherwise)
        {
            float4* base = nullptr;
            ALLOC(base, 4 * (size_t)p.q_stride, true);
            for (int d = 0; d < 4; ++d) S.q[d] = base + (size_t)d * p.q_stride;
        }
        for (int d = 0; d < 4; ++d) ALLOC(S.fq[d], nf, true);
        ALLOC(S.f8, nf, true);
        ALLOC(S.c8, nf, true);
        ALLOC(S.xp, nv, true);   // (per vertex slot: the positions behind F's in-plane columns inside a batch, see PSet)
        ALLOC(S.pid, np, true);
    }
    ALLOC(p.ta, std::max<size_t>(nf, 1), true);   // (k_p2g's vertex lanes read element 0 when an item has no face)
    ALLOC(p.G3, 3 * nf, true);
    ALLOC(p.VF, 3 * vf_entry((unsigned)nv + VF_CHUNK, 0), true);   // (whole chunks; k_p2g's face lanes read vertex 0's entries)
    {
        float* base = nullptr;
        ALLOC(base, 3 * (size_t)p.f_stride, true);
        for (int d = 0; d < 3; ++d) p.f[d] = base + (size_t)d * p.f_stride;
    }
    int* idx_orig[3];
    int *adj_off, *adj_fc;
    for (int d = 0; d < 3; ++d) { ALLOC(idx_orig[d], nf, false); p.idx_orig[d] = idx_orig[d]; }
    ALLOC(adj_off, nv + 1, false);
    ALLOC(adj_fc, 3 * nf, false);
    p.adj_off = adj_off; p.adj_fc = adj_fc;
    ALLOC(p.imap, np, false);
    ALLOC(p.pkey, np, false);
    ALLOC(p.prank, np, false);
    ALLOC(p.src_of, np, false);
    ALLOC(p.dst_of, np, false);
    ALLOC(p.tickets, 32 * 32, true);
    for (int t = 0; t < 2; ++t) {
        ALLOC(p.cellcnt[t], p.ncells, true);
        ALLOC(p.blkcnt[t], p.nblocks, true);
        ALLOC(p.blkstart[t], p.nblocks, true);
    }
    ALLOC(p.lut_home, p.nblocks, false);
    ALLOC(p.lut_act, p.nblocks, false);
    HIP_TRY(hipMemsetAsync(p.lut_home, 0xFF, (size_t)p.nblocks * 4, e->stream));  // -1 = not a home block
    HIP_TRY(hipMemsetAsync(p.lut_act, 0xFF, (size_t)p.nblocks * 4, e->stream));
    ALLOC(p.home_bits, p.nblocks / 32 + 1, true);
    ALLOC(p.home_block, p.capH, true);
    ALLOC(p.home_range, p.capH, true);
    ALLOC(p.home_nbr_act, (size_t)p.capH * 27, true);
    ALLOC(p.item_desc, p.capI, true);
    ALLOC(p.item_order, p.capI, true);
    ALLOC(p.item_flat, (size_t)p.capI * 2, true);
    ALLOC(p.item_rng, p.capI, true);
    ALLOC(p.item_pos, p.capI, true);
    ALLOC(p.home_items, p.capH, true);
    ALLOC(p.act_nbr_items, (size_t)p.capA * 27, true);
    ALLOC(p.home_ngroups, p.capH, true);
    ALLOC(p.home_groups, np / 64 + p.capH + 2, false);
    ALLOC(p.act_block, p.capA, true);
    ALLOC(p.act_nbr_home, (size_t)p.capA * 27, true);
    HIP_TRY(hipMalloc((void**)&p.slab, (size_t)p.capS * TILE_N * sizeof(float4)));   // (not in `allocs`: regrown)
    HIP_TRY(hipMemsetAsync(p.slab, 0, (size_t)p.capS * TILE_N * sizeof(float4), e->stream));
    ALLOC(p.slab_mask, p.capI, true);
    ALLOC(p.gv, (size_t)p.capA * 64, true);
    ALLOC(p.gvs, (size_t)p.capA * 64, true);
    ALLOC(e->d_pids_api, np, false);
    ALLOC(e->d_apimap, np, false);
    float4* dm_orig;
    ALLOC(dm_orig, nf, false);
    p.dm_orig = dm_orig;
#undef ALLOC

    // ---- host-side layout: [faces | verts], indices offset by +nf ---------
    // (cuda_mpm_model.cu:40-45)
    PSet& S0 = p.set[0];
    e->h_rest = e->h_pos;   // (the rest shape is the pose the cloths were added in, until mpm_set_rest_shape)
    e->rest_set = false;
    {
        std::vector<float> q0(np * 4, 0.f), q1(np * 4, 0.f);   // (x,y,z,vol) and (vx,vy,vz,C8); faces are filled on the device
        for (size_t i = 0; i < nv; ++i)
            for (int d = 0; d < 3; ++d) {
                q0[(nf + i) * 4 + d] = e->h_pos[i * 3 + d];
                q1[(nf + i) * 4 + d] = e->h_vel[i * 3 + d];
            }
        H2D(e, S0.q[0], q0.data(), np * 16);
        H2D(e, S0.q[1], q1.data(), np * 16);
    }
    std::vector<int> iota(np);
    std::iota(iota.begin(), iota.end(), 0);
    H2D(e, S0.pid, iota.data(), np * 4);
    H2D(e, p.imap, iota.data(), np * 4);
    H2D(e, e->d_pids_api, iota.data(), np * 4);
    H2D(e, e->d_apimap, iota.data(), np * 4);
    std::vector<int> col(nf);
    for (int d = 0; d < 3; ++d) {
        for (size_t f = 0; f < nf; ++f) col[f] = e->h_idx[f * 3 + d] + (int)nf;
        H2D(e, idx_orig[d], col.data(), nf * 4);
    }
    // corner vertex slots ride in fq[3].yzw (slot == original id before the first sort)
    std::vector<int> f3(nf * 4, 0);
    for (size_t f = 0; f < nf; ++f)
        for (int d = 0; d < 3; ++d) f3[f * 4 + 1 + d] = e->h_idx[f * 3 + d] + (int)nf;
    // a multi-material engine: the face's cloth above the corners' ranks (k_fem_mat; re-sorts move the word whole)
    std::vector<uint8_t> cloth_of_pid;
    if (e->multi_mat) {
        cloth_of_pid.resize(np);
        e->h_rho_of_pid.resize(np);
        for (size_t c = 0; c < e->cloths.size(); ++c) {
            const mpm_engine::Cloth& cl = e->cloths[c];
            for (size_t f = cl.first_face; f < cl.first_face + cl.n_faces; ++f) {
                f3[f * 4] = (int)(c << FACE_CLOTH_SHIFT);
                cloth_of_pid[f] = (uint8_t)c;
                e->h_rho_of_pid[f] = cl.m.density;
            }
            for (size_t v = cl.first_vertex; v < cl.first_vertex + cl.n_verts; ++v) {
                cloth_of_pid[nf + v] = (uint8_t)c;
                e->h_rho_of_pid[nf + v] = cl.m.density;
            }
        }
    }
    // vertex -> (face, corner) adjacency, ascending face id
    std::vector<int> off(nv + 1, 0), fc(3 * nf);
    for (size_t k = 0; k < 3 * nf; ++k) off[e->h_idx[k] + 1]++;
    for (size_t v = 0; v < nv; ++v) off[v + 1] += off[v];
    {
        std::vector<int> fill(off.begin(), off.end() - 1);
        for (size_t f = 0; f < nf; ++f)
            for (int c = 0; c < 3; ++c) {
                const int v = e->h_idx[f * 3 + c];
                const int at = fill[v]++;
                fc[at] = (int)(f << 2) | c;
                // the face's rank around this corner's vertex (DP::VF), 15 = the vertex has more than eight faces
                const int rank = off[v + 1] - off[v] <= 8 ? at - off[v] : 15;
                f3[f * 4] |= rank << (4 * c);
            }
    }
    if (nf) H2D(e, S0.fq[3], f3.data(), nf * 16);
    e->max_valence = 0;
    for (size_t v = 0; v < nv; ++v) e->max_valence = std::max(e->max_valence, off[v + 1] - off[v]);
    H2D(e, adj_off, off.data(), (nv + 1) * 4);
    if (nf) H2D(e, adj_fc, fc.data(), 3 * nf * 4);

    // ---- launch geometry --------------------------------------------------
    e->g_np = (unsigned)((np + 255) / 256);
    e->g_nf = (unsigned)((nf + 255) / 256);
    e->g_nv = (unsigned)((nv + 255) / 256);
    e->g_tile = std::min(512u, p.capI);  // 2 resident workgroups per CU pulling blocks from a queue
    if (getenv("MPM_P2G_WGS")) e->g_tile = (unsigned)std::max(1, atoi(getenv("MPM_P2G_WGS")));   // (tuning experiments)
    e->g_grid = std::min(1024u, (p.capA + 3) / 4);
    e->g_rb = getenv("MPM_RB_WGS") ? (unsigned)atoi(getenv("MPM_RB_WGS")) : 2048u;

    // ---- FEM initialisation (cuda_mpm_kernels.cuh:13-70) + first sort -----
    if (nf) hipLaunchKernelGGL(k_init_faces, dim3(e->g_nf), dim3(256), 0, e->stream, p);
    if (nv) hipLaunchKernelGGL(k_init_vertex_adjacency, dim3(e->g_nv), dim3(256), 0, e->stream, p);
    if (nv) hipLaunchKernelGGL(k_init_vertex_volumes, dim3(e->g_nv), dim3(256), 0, e->stream, p);
    if (e->multi_mat)
        if (int rc2 = init_cloth_materials(e, cloth_of_pid)) return rc2;
    if (int rc2 = set_fixed_point_scales(e)) return rc2;
    Ctl c0{};
    c0.cur = 0;
    c0.need_rebuild = 1;
    c0.nfa = (int)nf;
    c0.nva = (int)nv;
    HIP_TRY(hipMemcpyAsync(p.ctl, &c0, sizeof(Ctl), hipMemcpyHostToDevice, e->stream));
    launch_rebuild(e, e->dp);
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipGetLastError());
    {
        // a scene with few particles per block needs more slabs than the estimate above: grow and re-sort
        Ctl c;
        D2H(e, &c, p.ctl, sizeof(Ctl));
        if (int rc2 = recover_slab_overflow(e, c)) return rc2;
    }
    if (p.dbg) {
        int a = 0, b = 0, c = 0;
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&a, k_p2g<1, 0>, P2G_THREADS, 0);
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, k_g2p, G2P_THREADS, 0);
        (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&c, k_fem<0>, 256, 0);
        std::fprintf(stderr, "[mpm_hip] resident workgroups per CU: p2g %d, g2p %d, fem %d\n", a, b, c);
    }
    e->finalized = true;
    if (int rc2 = mpm_sync(e)) return rc2;
    {
        // the first re-sort's quiet time: the first batch of substeps starts with it (launch_substep)
        Ctl c;
        D2H(e, &c, p.ctl, sizeof(Ctl));
        e->quiet_left = c.error || c.need_rebuild ? 0.f : c.quiet_time;
    }
    return 0;
} MPM_CATCH_ALL

int mpm_destroy(mpm_handle_t e) try {
    if (!e) return 0;
    {
        std::lock_guard<std::mutex> lock(g_live_mutex);
        g_live.erase(std::remove(g_live.begin(), g_live.end(), e), g_live.end());
    }
    while (e->pins.load() > 0) std::this_thread::yield();   // (a GpuSync() of another thread is settling this engine)
    hipSetDevice(e->device);
    if (e->own_stream) hipStreamSynchronize(e->own_stream);
    (void)mpm_chain_destroy(e);
    for (void* a : e->allocs) hipFree(a);
    if (e->dp.slab) hipFree(e->dp.slab);
    if (e->d_stage) hipFree(e->d_stage);
    if (e->h_ctl) (void)hipHostFree(e->h_ctl);
    e->cb.release();
    if (e->own_stream) hipStreamDestroy(e->own_stream);
    delete e;
    return 0;
} MPM_CATCH_ALL

int mpm_counts(mpm_handle_t e, size_t* nv, size_t* nf, size_t* np) try {
    REQUIRE(e, "null handle");
    if (nv) *nv = e->nv;
    if (nf) *nf = e->nf;
    if (np) *np = e->np;
    return 0;
} MPM_CATCH_ALL

int mpm_set_deterministic(mpm_handle_t e, int on) try {
    REQUIRE(e, "null handle");
    if (e->finalized) {
        if (int rc = use(e)) return rc;
        if (int rc = settle(e)) return rc;
    }
    e->deterministic = on != 0;
    return 0;
} MPM_CATCH_ALL

int mpm_set_fast_math(mpm_handle_t e, int on) try {
    REQUIRE(e, "null handle");
    if (e->finalized) {
        if (int rc = use(e)) return rc;
        if (int rc = settle(e)) return rc;   // (owed substeps run with the arithmetic they were enqueued with)
    }
    e->fast_math = on != 0;
    e->dp.fem_fast = e->fast_math ? 1 : 0;
    return 0;
} MPM_CATCH_ALL

int mpm_get_fast_math(mpm_handle_t e, int* on_out) try {
    REQUIRE(e && on_out, "null argument");
    *on_out = e->fast_math ? 1 : 0;
    return 0;
} MPM_CATCH_ALL

int mpm_set_stream(mpm_handle_t e, void* s) try {
    REQUIRE(e, "null handle");
    if (int rc = use(e)) return rc;
    if (e->finalized)
        if (int rc = settle(e)) return rc;
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->stream = s ? static_cast<hipStream_t>(s) : e->own_stream;
    return 0;
} MPM_CATCH_ALL

// The stream is idle and `c` is the current control block: double the slab pool when the work items
// fill more than half of it.  Slabs only live from ParticleToGrid to UpdateGrid, so between substeps
// there is nothing to copy; between those two calls the old contents are kept.
static int slab_pool_grow(mpm_engine* e, const Ctl& c) {
    DP& p = e->dp;
    const unsigned items = std::max(c.n_items, c.n_items_wanted);
    if (p.capS >= p.capI || items * 2u <= p.capS) return 0;
    unsigned want = p.capS;
    while (want < p.capI && items * 2u > want) want = (unsigned)std::min<size_t>(p.capI, (size_t)want * 2);
    float4* bigger = nullptr;
    HIP_TRY(hipMalloc((void**)&bigger, (size_t)want * TILE_N * sizeof(float4)));
    HIP_TRY(hipMemcpyAsync(bigger, p.slab, (size_t)p.capS * TILE_N * sizeof(float4), hipMemcpyDeviceToDevice, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    HIP_TRY(hipFree(p.slab));
    p.slab = bigger;
    p.capS = want;
    return 0;
}

// The stream is idle and `c` is the control block.  If the last re-sort made more work items than the slab pool
// holds and nothing else is wrong, grow the pool to twice the wanted count, clear the flag and repeat the re-sort;
// `c` is refreshed.  Only legitimate while no substep has used the truncated tables: right after a re-sort
// (mpm_finalize, mpm_dist_init) or when every substep since has skipped itself (DP::gated bit 1).
static int recover_slab_overflow(mpm_engine* e, Ctl& c) {
    for (int round = 0; round < 4 && (c.error & ERR_SLABS); ++round) {
        if (c.error & ~ERR_SLABS) break;        // something else failed too: report it
        if (e->dp.capS >= e->dp.capI) break;    // (cannot happen: capI covers every legal item count)
        if (int rc = slab_pool_grow(e, c)) return rc;
        const unsigned zero = 0;
        const int one = 1;
        H2D(e, &e->dp.ctl->error, &zero, sizeof(unsigned));
        H2D(e, &e->dp.ctl->need_rebuild, &one, sizeof(int));
        launch_rebuild(e, e->dp);
        D2H(e, &c, e->dp.ctl, sizeof(Ctl));
    }
    return 0;
}

// `c` is the control block as it stands on an idle stream: what is left of the quiet time the last re-sort estimated
// (Ctl::quiet_time).  Nothing while a re-sort is pending, substeps are owed or an error flag is up.
static float quiet_time_left(const Ctl& c) {
    return c.skipped || c.need_rebuild || c.error ? 0.f : std::max(0.f, c.quiet_time - c.time_since_resort);
}
// Substeps enqueued right after go without check launches while it lasts (launch_substep); any call that may change the
// state resets it (settle_owed).
static void note_quiet_time(mpm_engine* e, const Ctl& c) { e->quiet_left = quiet_time_left(c); }

int mpm_sync(mpm_handle_t e) try {
    REQUIRE(e, "null handle");
    if (int rc = use(e)) return rc;
    Ctl c;
    e->settle_read_ctl = false;
    if (e->finalized)
        if (int rc = settle(e, &c)) return rc;
    if (!e->settle_read_ctl) {   // (otherwise settle() has just synchronised and read the control block: once is enough)
        HIP_TRY(hipStreamSynchronize(e->stream));
        HIP_TRY(hipGetLastError());
        if (!e->finalized && !e->dp.ctl) return 0;
        D2H(e, &c, e->dp.ctl, sizeof(Ctl));
    }
    if (e->finalized && !c.error)
        if (int rc = slab_pool_grow(e, c)) return rc;
    if (e->finalized) note_quiet_time(e, c);   // (also when settle() had nothing to do and this call read the block itself)
    if (c.error & ERR_DRIFT)
        return fail(MPM_ERR_DRIFT,
                    "a face particle was re-centred on its corners out of its block's tile: the corner "
                    "velocities differ by cells per substep, the state is diverging -- reduce dt");
    if (c.error & ERR_DOMAIN)
        return fail(MPM_ERR_DOMAIN, "a particle left the grid; results are invalid");
    if (c.error & ERR_HALO)
        return fail(MPM_ERR_HALO,
                    "partitioned domain: a particle left the zone shared with the neighbouring rank (or reached a "
                    "rank that is not a neighbour): migrate more often, or widen the zone / ghost band");
    if (c.error & ERR_RANGE)
        return fail(MPM_ERR_RANGE,
                    "a node sum of ParticleToGrid was not finite or exceeded the fixed-point range "
                    "(|node momentum| >= total mass * 2^15 length units per time unit): the state has diverged");
    // (last: a diverging state also scatters particles over so many blocks that tables overflow)
    if (c.error & (ERR_CAPACITY | ERR_SLABS))
        return fail(MPM_ERR_CAPACITY,
                    "a table of the engine overflowed (home / active blocks, slabs of the work items -- the pool is "
                    "grown at synchronisation points: call mpm_sync more often while a cloth spreads out, or set "
                    "MPM_SLAB_CAPACITY --, slabs over one block, halo or migration buffers)");
    return 0;
} MPM_CATCH_ALL

// partitioned and multi-rank engines take none of the features of mpm_features.h (FeatureRow::partitioned; out of scope).
// set_up: the call partitions the engine or joins it to other ranks (mpm_dist_init, chain, team, world), which an engine
// with a rest shape of its own refuses too; the halo substeps of a single engine run on whatever rest state it holds.
static int extensions_refused(const mpm_engine* e, const char* what, bool set_up = true) {
    const Feature f = partition_blocker(feature_state(e), set_up);
    if (f == F_NONE) return 0;
    const FeatureRow& r = FEATURES[f];
    return fail(MPM_ERR_INVALID, std::string(what) + ": not available on " + (r.on_tail ? r.on_tail : std::string("an engine with ") + r.phrase));
}
// An explicit linear drag beyond dt * gamma = 1 reverses the relative velocity: the substep entry points that take a dt
// refuse it, once per call, before anything is enqueued.  (An engine without a table never gets past the first test.)
// The same entry points refuse a dt above mpm_<guard>_max_stable_dt of a feature in force that has a guard (the rows of
// mpm_features.h; each guard is explained in its feature's header): of several, the last in table order.
// Each guard bounds its own force alone, at the rest shape, with the membrane force left out, and each is tested alone: a
// dt that every guard accepts can still be unstable for the sum of the forces ("What the dt guards bound",
// has the measured margins and a counter-example).  A step of 1 / sum_f (1 / max_dt_f) over the guards in force is
// sufficient for the sum; this function does not ask for it.
static int fields_stable(const mpm_engine* e, float dt) {
    const FeatureState s = feature_state(e);
    const Feature f = violated_guard(s, dt);
    if (f != F_NONE) {
        const FeatureRow& r = FEATURES[f];
        char msg[200];
        std::snprintf(msg, sizeof msg, "%s: dt = %g is above the limit mpm_%s_max_stable_dt = %g: the explicit %s force is unstable -- "
                      "reduce %s", r.guard, (double)dt, r.guard, (double)s.max_dt[f], r.force, r.reduce);
        return fail(MPM_ERR_INVALID, msg);
    }
    if (!s.on[F_FORCE_FIELDS]) return 0;
    if (!((double)dt * e->force_fields_gamma <= 1.0))
        return fail(MPM_ERR_INVALID, "force fields: dt * (sum of gamma over the linear drag fields) = " +
                                         std::to_string((double)dt * e->force_fields_gamma) + " > 1: the explicit drag is unstable -- reduce dt or gamma");
    return 0;
}
// The quiet-time hint of the re-sort (Ctl::quiet_time) assumes gravity alone: while a feature that moves the cloth otherwise
// is in force (FeatureRow::ends_quiet_hint) the host takes it as 0, i.e. every batch starts with its re-sort check launches.
static float quiet_hint(const mpm_engine* e, float seconds) { return quiet_hint_holds(feature_state(e)) ? seconds : 0.f; }

// ---- the solver calls -----------------------------------------------------
static void launch_substep(mpm_engine* e, float dt, const GridColliders& gc, bool allow_gate, bool lean = false);

// Substeps that mpm_run_substeps enqueued without their re-sort launches and that found a re-sort pending
// did nothing (Ctl::skipped): run them now, each with the re-sort in front.  Called by every entry point
// before it looks at or changes the state.
// `fresh`: receives the control block if this call read it and enqueued nothing afterwards (the stream is idle and
// *fresh is the state); untouched otherwise.
static int flush_phases(mpm_engine* e);
static int settle_owed(mpm_engine* e, Ctl* fresh);
static int settle(mpm_engine* e, Ctl* fresh) {
    if (int rc = settle_owed(e, fresh)) return rc;
    // phase calls that were waiting for the rest of their substep (see PendingPhases) come after everything owed
    if (e->pend.n) {
        e->settle_read_ctl = false;   // (what settle_owed read is no longer the state)
        return flush_phases(e);
    }
    return 0;
}
static int settle_owed(mpm_engine* e, Ctl* fresh) {
    e->force_check = true;   // whatever comes next starts with the re-sort launches
    e->quiet_left = 0.f;     // (the call that settles may change the state: the hint is only kept from a settle that
                             // has just read it, below, to the substeps enqueued right after)
    if (!e->maybe_owed) return 0;
    // (a few rounds: a substep that is run again may itself overflow the slab pool -- a cloth that keeps spreading)
    for (int round = 0; round < 8 && e->maybe_owed; ++round) {
        e->maybe_owed = false;
        Ctl c;
        // (synchronises the stream.  Into pinned memory: a copy into pageable memory is staged by the runtime and
        // costs ~10 us more, which a caller that synchronises after every frame of substeps pays every time)
        if (!e->h_ctl) HIP_TRY(hipHostMalloc((void**)&e->h_ctl, sizeof(Ctl), hipHostMallocDefault));
        D2H(e, e->h_ctl, e->dp.ctl, sizeof(Ctl));
        c = *e->h_ctl;
        // every substep since the overflowing re-sort has skipped itself: the pool can be grown and the re-sort repeated
        if (int rc = recover_slab_overflow(e, c)) return rc;
        const unsigned owed = c.skipped;
        note_quiet_time(e, c);
        if (e->dp.dbg & 32)
            std::fprintf(stderr, "[mpm_hip] settle: quiet time %.4g s, %.4g s since the re-sort, %u owed, re-sort pending %d, checks launched %llu\n",
                         c.quiet_time, c.time_since_resort, owed, c.need_rebuild, (unsigned long long)e->checks_launched);
        if (!owed) {
            if (fresh) {
                *fresh = c;
                e->settle_read_ctl = true;
            }
            break;
        }
        const unsigned zero = 0;
        H2D(e, &e->dp.ctl->skipped, &zero, sizeof(unsigned));
        GridColliders gc;
        if (int rc = grid_colliders_for(e, e->owed_bc, &gc)) return rc;
        for (unsigned k = 0; k < owed; ++k) launch_substep(e, e->owed_dt, gc, false);
    }
    e->force_check = true;
    return 0;
}

int mpm_halo_zone_blocks(mpm_handle_t e, int bx_lo, int bx_hi, uint32_t* count_out) try {
    READY(e);
    REQUIRE(count_out, "null output");
    HIP_TRY(hipStreamSynchronize(e->stream));
    Ctl c;
    D2H(e, &c, e->dp.ctl, sizeof(Ctl));
    std::vector<uint32_t> blocks(c.n_active);
    if (c.n_active) D2H(e, blocks.data(), e->dp.act_block, (size_t)c.n_active * 4);
    auto compact3 = [](uint32_t v) {   // (host copy of mpm_math.h's: every third bit)
        v &= 0x09249249u;
        v = (v ^ (v >> 2)) & 0x030C30C3u;
        v = (v ^ (v >> 4)) & 0x0300F00Fu;
        v = (v ^ (v >> 8)) & 0xFF0000FFu;
        v = (v ^ (v >> 16)) & 0x000003FFu;
        return v;
    };
    uint32_t n = 0;
    for (uint32_t b : blocks) {
        const int bx = (int)compact3(b >> 2);
        n += bx >= bx_lo && bx <= bx_hi;
    }
    *count_out = n;
    return 0;
} MPM_CATCH_ALL

int mpm_contact_frame(const float u[3], float J[9]) try {
    REQUIRE(u && J, "null argument");
    frame_from_normal(u, J);
    return 0;
} MPM_CATCH_ALL

int mpm_profile_contact_iteration(mpm_handle_t e, int reps, float kernel_ms[4]) try {
    READY(e);
    REQUIRE(kernel_ms && reps > 0 && reps <= 1000, "bad arguments");
    return profile_contact_iteration(e, reps, kernel_ms);
} MPM_CATCH_ALL

int mpm_memcpy_d2h(mpm_handle_t e, void* dst_host, const void* src_device, size_t bytes) try {
    REQUIRE(e, "null handle");
    REQUIRE(bytes == 0 || (dst_host && src_device), "null pointer");
    if (int rc = use(e)) return rc;
    if (bytes) D2H(e, dst_host, src_device, bytes);
    return 0;
} MPM_CATCH_ALL

int mpm_memcpy_h2d(mpm_handle_t e, void* dst_device, const void* src_host, size_t bytes) try {
    REQUIRE(e, "null handle");
    REQUIRE(bytes == 0 || (dst_device && src_host), "null pointer");
    if (int rc = use(e)) return rc;
    if (bytes) H2D(e, dst_device, src_host, bytes);
    return 0;
} MPM_CATCH_ALL

int mpm_debug_owed_substeps(mpm_handle_t e, uint32_t* out) try {
    READY_NO_SETTLE(e);
    REQUIRE(out, "null output");
    unsigned owed = 0;
    D2H(e, &owed, &e->dp.ctl->skipped, sizeof(unsigned));
    *out = owed;
    return 0;
} MPM_CATCH_ALL

int mpm_device_synchronize(void) try {
    // The reference's GpuSync() is a plain cudaDeviceSynchronize (cuda_mpm_solver.cu:164-166): it completes the work
    // of the device and says nothing about the state of any simulation.  Here "the work" includes substeps that
    // mpm_run_substeps deferred, so every engine of the device is settled and flushed first; the sticky SIMULATION
    // errors of an engine (diverged, capacity, ...) stay with that engine -- its own mpm_sync / mpm_get_stats report
    // them -- and only a failure of the runtime itself is an error of this call.  The list is walked under the lock
    // that mpm_create / mpm_destroy take: an engine cannot be destroyed by another thread while it is being settled.
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    int first = 0;
    std::string first_msg;
    //  the engines of this device are PINNED under the lock and settled outside it: mpm_create / mpm_destroy of
    // other threads do not stall behind a GPU drain, and mpm_destroy of a pinned engine waits for the pin to go
    std::vector<mpm_engine*> mine;
    {
        std::lock_guard<std::mutex> lock(g_live_mutex);
        for (mpm_engine* e : g_live)
            if (e->device == dev) {
                e->pins.fetch_add(1);
                mine.push_back(e);
            }
    }
    for (mpm_engine* e : mine) {
        const int rc = mpm_sync(e);
        if ((rc == MPM_ERR_HIP || rc == MPM_ERR_NOMEM || rc == MPM_ERR_INTERNAL) && !first) {
            first = rc;
            first_msg = g_last_error;
        }
        e->pins.fetch_sub(1);
    }
    HIP_TRY(hipSetDevice(dev));
    HIP_TRY(hipDeviceSynchronize());
    return first ? fail(first, first_msg) : 0;
} MPM_CATCH_ALL

// The reference's five calls per substep (cuda_mpm_test.cc:64-72, deformable_driver.h:244-258), taken one by one, are
// nine launches with the re-sort check in front of every substep and the vertex forces as a kernel of their own.
// When they arrive in the standard order -- RebuildMapping(false), CalcFemStateAndForce(dt), ParticleToGrid(dt),
// UpdateGrid(bc), GridToParticle(dt) -- nothing is launched until the last one, and the substep then goes through the
// same path as mpm_run_substeps(1): check launches only when a re-sort can be due, vertex forces inside ParticleToGrid,
// deferral if a re-sort is pending.  Any other call in between (a download, the contact calls, a different order, a
// different dt) first launches what was held back, call by call as before, so every intermediate state a caller can
// look at is the one the reference would show.  MPM_DEFER_PHASES=0 turns this off.
static bool can_defer(const mpm_engine* e) { return e->defer_phases && e->finalized && !e->dp.dist.on; }
static int flush_phases(mpm_engine* e) {
    const int n = e->pend.n;
    e->pend.n = 0;
    if (n == 1 || n == 2) launch_rebuild(e, e->dp);
    if (n == 2) launch_fem(e, e->dp, e->pend.dt);
    if (n >= 3) {
        // (nobody looked at the forces between CalcFemStateAndForce and ParticleToGrid: the vertex forces are
        // gathered inside k_p2g, which also writes them out -- one launch less, the same numbers)
        enqueue_substep_front(e, e->dp, e->pend.dt, Resort::Held);
        e->grid_state = 1;
    }
    if (n >= 4) {
        GridColliders gc;
        if (int rc = grid_colliders_for(e, e->pend.bc, &gc)) return rc;
        enqueue_substep_rest(e, GridForm::Fused, e->dp, gc, nullptr, 0.f);
        e->grid_state = 2;
    }
    return 0;
}

int mpm_rebuild_mapping(mpm_handle_t e, int sort) try {
    if (e && can_defer(e) && !sort && e->pend.n == 0) {
        READY_NO_SETTLE(e);
        e->pend.n = 1;
        return 0;
    }
    READY(e);
    launch_rebuild(e, e->dp);
    if (sort) {
        REQUIRE(!e->dp.dist.on, "RebuildMapping(sort = true) is not available on a partitioned domain");
        return api_sort(e);
    }
    return 0;
} MPM_CATCH_ALL

int mpm_calc_fem_state_and_force(mpm_handle_t e, float dt) try {
    if (e && e->finalized)
        if (int rc = anchors_ready(e)) return rc;   // (before the phase is held back or enqueued: k_anchor reads the motions)
    if (e && can_defer(e) && e->pend.n == 1) {
        READY_NO_SETTLE(e);
        e->pend.n = 2;
        e->pend.dt = dt;
        return 0;
    }
    READY(e);
    launch_fem(e, e->dp, dt);
    return 0;
} MPM_CATCH_ALL

int mpm_particle_to_grid(mpm_handle_t e, float dt) try {
    if (e && e->finalized)
        if (int rc = fields_stable(e, dt)) return rc;   // (before the phase is held back or enqueued)
    if (e && can_defer(e) && e->pend.n == 2 && dt == e->pend.dt) {
        READY_NO_SETTLE(e);
        e->pend.n = 3;
        return 0;
    }
    READY(e);
    launch_p2g(e, e->dp, dt);
    e->grid_state = 1;
    return 0;
} MPM_CATCH_ALL

int mpm_update_grid(mpm_handle_t e, int bc) try {
    if (e && can_defer(e) && e->pend.n == 3) {
        READY_NO_SETTLE(e);
        GridColliders probe;
        if (int rc = grid_colliders_for(e, bc, &probe)) return rc;   // (a bad mpm_bc is reported by this call)
        e->pend.n = 4;
        e->pend.bc = bc;
        return 0;
    }
    READY(e);
    REQUIRE(e->grid_state >= 1, "UpdateGrid before ParticleToGrid");
    GridColliders gc;
    if (int rc = grid_colliders_for(e, bc, &gc)) return rc;
    enqueue_substep_rest(e, GridForm::Fused, e->dp, gc, nullptr, 0.f);
    e->grid_state = 2;
    return 0;
} MPM_CATCH_ALL

int mpm_grid_gather(mpm_handle_t e) try {
    READY(e);
    REQUIRE(e->grid_state >= 1, "grid gather before ParticleToGrid");
    enqueue_substep_rest(e, GridForm::Gather, e->dp, GridColliders{}, nullptr, 0.f);
    e->grid_state = 3;  // raw sums in gv
    return 0;
} MPM_CATCH_ALL

size_t mpm_halo_buffer_bytes(size_t cap) { return zone_buffer_bytes(cap, 1); }

int mpm_halo_pack(mpm_handle_t e, int bx_lo, int bx_hi, int shift_bx, void* dev_buf, size_t cap) try {
    READY(e);
    REQUIRE(e->grid_state == 3, "halo pack needs mpm_grid_gather first");
    REQUIRE(dev_buf && cap > 0 && cap < (1u << 24), "bad halo buffer");
    HIP_TRY(hipMemsetAsync(dev_buf, 0, 16, e->stream));
    Zones z{};
    z.lo[0] = bx_lo; z.hi[0] = bx_hi; z.shift[0] = shift_bx;
    z.buf[0] = static_cast<uint32_t*>(dev_buf);
    hipLaunchKernelGGL(k_halo_pack2, dim3(e->g_grid, 1), dim3(256), 0, e->stream, e->dp, z, (unsigned)cap);
    return 0;
} MPM_CATCH_ALL

int mpm_halo_add(mpm_handle_t e, const void* dev_buf, size_t cap) try {
    READY(e);
    REQUIRE(e->grid_state == 3, "halo add needs mpm_grid_gather first");
    REQUIRE(dev_buf && cap > 0, "bad halo buffer");
    Zones z{};
    z.buf[0] = static_cast<uint32_t*>(const_cast<void*>(dev_buf));   // (read only)
    hipLaunchKernelGGL(k_halo_add2, dim3(64, 1), dim3(256), 0, e->stream, e->dp, z, (unsigned)cap);
    return 0;
} MPM_CATCH_ALL

int mpm_update_grid_from_sums(mpm_handle_t e, int bc) try {
    READY(e);
    REQUIRE(e->grid_state == 3, "needs mpm_grid_gather first");
    GridColliders gc;
    if (int rc = grid_colliders_for(e, bc, &gc)) return rc;
    REQUIRE(gc.n >= 0, "MPM_BC_BODIES is not available in the halo substeps (grid bodies: single-engine only)");
    enqueue_substep_rest(e, GridForm::FromSums, e->dp, gc, nullptr, 0.f);
    e->grid_state = 2;
    return 0;
} MPM_CATCH_ALL

int mpm_substep_begin(mpm_handle_t e, float dt) try {
    READY(e);
    if (int rc = fields_stable(e, dt)) return rc;
    if (int rc = anchors_ready(e)) return rc;
    enqueue_substep_front(e, e->dp, dt, Resort::Full);
    enqueue_substep_rest(e, GridForm::Gather, e->dp, GridColliders{}, nullptr, 0.f);
    e->grid_state = 3;
    return 0;
} MPM_CATCH_ALL

int mpm_substep_end(mpm_handle_t e, float dt, int bc) try {
    READY(e);
    if (int rc = pins_ready(e)) return rc;
    REQUIRE(e->grid_state == 3, "mpm_substep_end without mpm_substep_begin");
    GridColliders gc;
    if (int rc = grid_colliders_for(e, bc, &gc)) return rc;
    REQUIRE(gc.n >= 0, "MPM_BC_BODIES is not available in the halo substeps (grid bodies: single-engine only)");
    enqueue_substep_rest(e, GridForm::FromSums, e->dp, gc, &e->dp, dt);
    e->grid_state = 2;
    e->substeps += 1;
    return 0;
} MPM_CATCH_ALL

// lean: another substep of the same batch follows (mpm_chain_substeps, see DP::lean_g2p)
// counters: per zone the word the pack counts its entries in (null: word 0 of the send buffer itself)
static int substep_begin_halo(mpm_handle_t e, float dt, int n, const int* bx_lo, const int* bx_hi, const int* shift_bx,
                              void* const* send_bufs, size_t cap, uint32_t* const* counters, bool lean) {
    READY(e);
    if (int rc = extensions_refused(e, "halo substeps", false)) return rc;
    REQUIRE(n >= 0 && n <= 2 && (n == 0 || (bx_lo && bx_hi && shift_bx && send_bufs)), "bad halo zone list");
    REQUIRE(n == 0 || (cap > 0 && cap < (1u << 24)), "bad halo buffer");
    DP p = e->dp;   // per-launch copy: k_grid<0> packs the zones' sums into the send buffers as it gathers them
    DP pp = e->dp;  // ... and k_p2g, in front of it, resets their entry counters
    p.halo_pn = n;
    p.halo_pcap = (unsigned)cap;
    pp.lean_g2p = lean && !e->dp.dist.on;
    for (int i = 0; i < n; ++i) {
        REQUIRE(send_bufs[i], "null halo buffer");
        pp.halo_hdr[i] = counters && counters[i] ? counters[i] : static_cast<uint32_t*>(send_bufs[i]);
        p.halo_plo[i] = bx_lo[i]; p.halo_phi[i] = bx_hi[i]; p.halo_pshift[i] = shift_bx[i];
        p.halo_pbuf[i] = static_cast<uint32_t*>(send_bufs[i]);
        p.halo_pcnt[i] = counters ? counters[i] : nullptr;
    }
    enqueue_substep_front(e, pp, dt, Resort::Lean);
    enqueue_substep_rest(e, GridForm::Gather, p, GridColliders{}, nullptr, 0.f);
    e->grid_state = 3;
    e->halo_mid_done = false;
    e->halo_nz = n;
    for (int i = 0; i < n; ++i) { e->halo_zlo[i] = bx_lo[i]; e->halo_zhi[i] = bx_hi[i]; }
    return 0;
}
int mpm_substep_begin_halo(mpm_handle_t e, float dt, int n, const int* bx_lo, const int* bx_hi, const int* shift_bx,
                           void* const* send_bufs, size_t cap) try {
    return substep_begin_halo(e, dt, n, bx_lo, bx_hi, shift_bx, send_bufs, cap, nullptr, false);
} MPM_CATCH_ALL

// the zones of the last mpm_substep_begin_halo into a DP's zone list (halo_nz / halo_zlo / halo_zhi of a split update, or
// halo_pn / halo_plo / halo_phi of an update that adds the received sums itself)
static void halo_zones_into(const mpm_engine* e, int* n, int* lo, int* hi) {
    *n = e->halo_nz;
    for (int i = 0; i < e->halo_nz; ++i) { lo[i] = e->halo_zlo[i]; hi[i] = e->halo_zhi[i]; }
}

// Between begin and end: the part of the grid update and of G2P that does not depend on the
// neighbours' sums, to be overlapped with the exchange.  Zones = the ranges given to begin.
int mpm_substep_mid_halo(mpm_handle_t e, float dt, int bc) try {
    READY(e);
    if (int rc = extensions_refused(e, "halo substeps", false)) return rc;
    REQUIRE(e->grid_state == 3 && !e->halo_mid_done, "mpm_substep_mid_halo needs mpm_substep_begin_halo first");
    GridColliders gc;
    if (int rc = grid_colliders_for(e, bc, &gc)) return rc;
    DP p = e->dp;
    p.halo_cls = 0;
    halo_zones_into(e, &p.halo_nz, p.halo_zlo, p.halo_zhi);
    enqueue_substep_rest(e, GridForm::FromSums, p, gc, &p, dt);
    e->halo_mid_done = true;
    return 0;
} MPM_CATCH_ALL

// with_g2p = false: the grid update only -- a coupled substep puts the contact solve between it and GridToParticle
// lean: as for substep_begin_halo
static int substep_end_halo(mpm_handle_t e, float dt, int bc, int n, const void* const* recv_bufs, size_t cap, bool with_g2p,
                            bool lean) {
    READY(e);
    if (int rc = extensions_refused(e, "halo substeps", false)) return rc;
    REQUIRE(n >= 0 && n <= 2 && (n == 0 || recv_bufs), "bad halo buffer list");
    REQUIRE(e->grid_state == 3, "mpm_substep_end_halo without mpm_substep_begin_halo");
    GridColliders gc;
    if (int rc = grid_colliders_for(e, bc, &gc)) return rc;
    Zones b{};   // (read only)
    for (int i = 0; i < n; ++i) {
        REQUIRE(recv_bufs[i], "null halo buffer");
        b.buf[i] = static_cast<uint32_t*>(const_cast<void*>(recv_bufs[i]));
    }
    DP p = e->dp;
    p.lean_g2p = lean && !e->dp.dist.on;
    if (e->halo_mid_done) {   // the interior is done: only what the received sums touch is left
        p.halo_cls = 1;
        halo_zones_into(e, &p.halo_nz, p.halo_zlo, p.halo_zhi);
    }
    // The received sums are added inside the grid update (k_grid<2> looks its zone blocks up in the buffers): one launch
    // less per substep than add + update.  Needs the zones of the matching mpm_substep_begin_halo, buffer i <-> zone i.
    DP pg = p;
    const bool folded = n > 0 && n == e->halo_nz;
    if (folded) {
        halo_zones_into(e, &pg.halo_pn, pg.halo_plo, pg.halo_phi);
        pg.halo_pcap = (unsigned)cap;
        for (int i = 0; i < n; ++i) pg.halo_pbuf[i] = b.buf[i];
    }
    if (n > 0 && !folded) hipLaunchKernelGGL(k_halo_add2, dim3(64, n), dim3(256), 0, e->stream, p, b, (unsigned)cap);
    enqueue_substep_rest(e, GridForm::FromSums, pg, gc, with_g2p ? &p : nullptr, dt);
    e->halo_mid_done = false;
    e->grid_state = 2;
    if (with_g2p) e->substeps += 1;
    return 0;
}
int mpm_substep_end_halo(mpm_handle_t e, float dt, int bc, int n, const void* const* recv_bufs, size_t cap) try {
    return substep_end_halo(e, dt, bc, n, recv_bufs, cap, true, false);
} MPM_CATCH_ALL

// ---- the native chain, its direct halo and the team transport's set-up (mpm_chain_host.h) -----------------------------
int mpm_chain_unique_id(char id_out[128]) try {
    REQUIRE(id_out, "null argument");
    return chain_unique_id(id_out);
} MPM_CATCH_ALL

int mpm_chain_destroy(mpm_handle_t e) try {
    REQUIRE(e, "null handle");
    return chain_destroy(e);
} MPM_CATCH_ALL

int mpm_chain_enable_migration(mpm_handle_t e, int every, size_t capacity_particles) try {
    READY(e);
    if (int rc = extensions_refused(e, "mpm_chain_enable_migration")) return rc;
    return chain_enable_migration(e, every, capacity_particles);
} MPM_CATCH_ALL

int mpm_chain_init(mpm_handle_t e, const char id[128], int rank, int world, int cut_lo_block, int cut_hi_block,
                   int pitch_blocks, int zone_blocks, size_t capacity_blocks, int periodic) try {
    READY(e);
    if (int rc = extensions_refused(e, "mpm_chain_init")) return rc;
    REQUIRE(world >= 1 && rank >= 0 && rank < world, "bad rank / world");
    REQUIRE(zone_blocks >= 1 && capacity_blocks > 0 && capacity_blocks < (1u << 24), "bad halo geometry");
    return chain_init(e, id, rank, world, cut_lo_block, cut_hi_block, pitch_blocks, zone_blocks, capacity_blocks, periodic);
} MPM_CATCH_ALL

int mpm_chain_direct_prepare(mpm_handle_t e, char handle_out[64]) try {
    READY(e);
    if (int rc = extensions_refused(e, "mpm_chain_direct_prepare")) return rc;
    return chain_direct_prepare(e, handle_out);
} MPM_CATCH_ALL

int mpm_chain_direct_connect(mpm_handle_t e, const char left_handle[64], const char right_handle[64]) try {
    READY(e);
    return chain_direct_connect(e, left_handle, right_handle);
} MPM_CATCH_ALL

// Neighbours that live in THIS process (an in-process world: several engines of one partition on one stream, for tests and
// rehearsals of more ranks than a box admits processes): their regions are plain pointers, a HIP IPC handle of one's own
// process cannot be opened.  mpm_chain_direct_base hands a rank's region out, mpm_chain_direct_connect_local takes the
// neighbours'.
int mpm_chain_direct_base(mpm_handle_t e, void** base_out) try {
    READY(e);
    REQUIRE(base_out, "null argument");
    REQUIRE(e->chain.direct_base, "mpm_chain_direct_prepare first");
    *base_out = e->chain.direct_base;
    return 0;
} MPM_CATCH_ALL

int mpm_chain_direct_connect_local(mpm_handle_t e, void* left_base, void* right_base) try {
    READY(e);
    return chain_direct_connect_local(e, left_base, right_base);
} MPM_CATCH_ALL

int mpm_team_prepare(mpm_handle_t e, size_t zone_capacity_blocks, char handle_out[64], void** base_out) try {
    READY(e);
    if (int rc = extensions_refused(e, "mpm_team_prepare")) return rc;
    REQUIRE(e->dp.dist.on, "mpm_dist_init first");
    REQUIRE(e->dp.dist.world <= TEAM_MAX, "the team transport serves the ranks of one node (at most 8)");
    REQUIRE(zone_capacity_blocks > 0 && zone_capacity_blocks < (1u << 20), "bad zone capacity");
    return team_prepare(e, zone_capacity_blocks, handle_out, base_out);
} MPM_CATCH_ALL

// handles: world x 64 bytes (the IPC handles of all ranks, own slot ignored) or NULL; local_bases: world pointers or NULL --
// a rank of this process is named by its region's pointer (mpm_team_prepare's base_out), every other one by its handle
int mpm_team_connect(mpm_handle_t e, const char* handles, void* const* local_bases) try {
    READY(e);
    if (int rc = extensions_refused(e, "mpm_team_connect")) return rc;
    return team_connect(e, handles, local_bases);
} MPM_CATCH_ALL

int mpm_chain_substeps(mpm_handle_t e, int n, float dt, int bc) try {
    READY(e);
    if (int rc = extensions_refused(e, "mpm_chain_substeps")) return rc;
    return chain_substeps(e, n, dt, bc);
} MPM_CATCH_ALL

int mpm_grid_to_particle(mpm_handle_t e, float dt) try {
    if (e && e->finalized)
        if (int rc = pins_ready(e)) return rc;   // (before the held-back phases are let go)
    if (e && can_defer(e) && e->pend.n == 4 && dt == e->pend.dt) {
        // the substep is complete: one gated substep, as mpm_run_substeps(1) enqueues it
        e->pend.n = 0;
        return mpm_run_substeps(e, 1, dt, e->pend.bc);
    }
    READY(e);
    REQUIRE(e->grid_state == 2, "GridToParticle before UpdateGrid");
    launch_g2p(e, e->dp, dt);
    e->substeps += 1;
    return 0;
} MPM_CATCH_ALL

int mpm_substep(mpm_handle_t e, float dt, int bc) try { return mpm_run_substeps(e, 1, dt, bc); } MPM_CATCH_ALL

// allow_gate: the substep may go without the re-sort launches (mpm_run_substeps; settle_owed runs the owed ones with them)
// lean: another substep follows in the same batch, GridToParticle need not refresh what only a download reads
static void launch_substep(mpm_engine* e, float dt, const GridColliders& gc, bool allow_gate, bool lean) {
    // Re-sort check launches: with every substep that may not skip itself; otherwise none while the quiet time that
    // the last re-sort estimated lasts (half of it: the estimate is ballistic, elastic forces are not in it), then
    // with every check_every-th substep.  A wrong guess costs time, not correctness: substeps that find a re-sort
    // pending without their check skip themselves and are run again by settle().
    // (a quiet time left over from the settle() that has just read it also stands for "no re-sort pending, nothing
    // has touched the state since": the check that otherwise follows every other call is not needed either)
    const bool quiet = allow_gate && e->quiet_factor * quiet_hint(e, e->quiet_left) > dt;
    bool check = !allow_gate || (e->force_check && !quiet) || e->check_every <= 1 || e->dp.dist.on;
    if (!check) {
        if (quiet) {
            e->quiet_left -= dt / e->quiet_factor;
        } else {
            e->quiet_left = 0.f;
            check = (e->step_phase % (unsigned)e->check_every) == 0u;
        }
    }
    e->step_phase += 1;
    if (check) e->force_check = false;
    e->maybe_owed = true;
    DP p = e->dp;
    p.gated = check ? 2 : 3;   // (bit 1: it also skips itself while the slab pool is too small, see DP::gated)
    p.lean_g2p = lean && !p.dist.on;   // (k_p2g: the forces stay in LDS; k_g2p: no face x / v records)
    enqueue_substep_front(e, p, dt, check ? Resort::Lean : Resort::None);
    enqueue_substep_rest(e, GridForm::Fused, p, gc, &p, dt);
}

int mpm_run_substeps(mpm_handle_t e, int n, float dt, int bc) try {
    READY_NO_SETTLE(e);
    if (int rc = pins_ready(e)) return rc;
    if (int rc = fields_stable(e, dt)) return rc;
    // owed substeps are run with the parameters they were enqueued with: settle before these change (and before phase
    // calls that were held back, which come first)
    if (e->pend.n || (e->maybe_owed && (dt != e->owed_dt || bc != e->owed_bc || e->grid_colliders_version != e->owed_gcv)))
        if (int rc = settle(e)) return rc;
    e->owed_dt = dt;
    e->owed_bc = bc;
    e->owed_gcv = e->grid_colliders_version;
    GridColliders gc;
    if (int rc = grid_colliders_for(e, bc, &gc)) return rc;
    for (int s = 0; s < n; ++s) launch_substep(e, dt, gc, true, s + 1 < n);
    e->grid_state = 2;
    e->substeps += (uint64_t)std::max(n, 0);
    HIP_TRY(hipGetLastError());
    return 0;
} MPM_CATCH_ALL

int mpm_profile_substeps(mpm_handle_t e, int n, float dt, int bc, float* phase_ms, float* total_ms) try {
    READY(e);
    if (int rc = pins_ready(e)) return rc;
    if (int rc = fields_stable(e, dt)) return rc;
    REQUIRE(n > 0 && n <= 4096, "n out of range");
    GridColliders gc;
    if (int rc = grid_colliders_for(e, bc, &gc)) return rc;
    // (what mpm_run_substeps launches, with events between the phases; but every substep carries its re-sort launches, all
    // of them, and none skips itself)
    const int NE = MPM_PHASE_COUNT + 1;
    Events ev;
    if (int rc = ev.create((size_t)n * NE)) return rc;
    hipError_t err = hipSuccess;
    for (int s = 0; s < n && err == hipSuccess; ++s) {
        const hipEvent_t* q = &ev[(size_t)s * NE];
        const PhaseMark mark = [&](int phase) {
            if (err == hipSuccess) err = hipEventRecord(q[phase + 1], e->stream);
        };
        err = hipEventRecord(q[0], e->stream);
        DP p = e->dp;
        p.lean_g2p = s + 1 < n && !p.dist.on;   // (as in mpm_run_substeps)
        enqueue_substep_front(e, p, dt, Resort::Full, mark);
        enqueue_substep_rest(e, GridForm::Fused, p, gc, &p, dt, mark);
    }
    if (err != hipSuccess) return fail(MPM_ERR_HIP, std::string("hipEventRecord: ") + hipGetErrorString(err));
    e->grid_state = 2;
    e->substeps += (uint64_t)n;
    HIP_TRY(hipStreamSynchronize(e->stream));
    double acc[MPM_PHASE_COUNT] = {}, tot = 0;
    for (int s = 0; s < n; ++s) {
        const hipEvent_t* q = &ev[(size_t)s * NE];
        for (int k = 0; k < MPM_PHASE_COUNT; ++k) {
            float ms = 0;
            HIP_TRY(hipEventElapsedTime(&ms, q[k], q[k + 1]));
            acc[k] += ms;
        }
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, q[0], q[MPM_PHASE_COUNT]));
        tot += ms;
    }
    if (phase_ms)
        for (int k = 0; k < MPM_PHASE_COUNT; ++k) phase_ms[k] = (float)(acc[k] / n);
    if (total_ms) *total_ms = (float)(tot / n);
    return 0;
} MPM_CATCH_ALL

int mpm_get_stats(mpm_handle_t e, mpm_stats_t* out) try {
    READY(e);
    REQUIRE(out, "null stats");
    HIP_TRY(hipStreamSynchronize(e->stream));
    Ctl c;
    D2H(e, &c, e->dp.ctl, sizeof(Ctl));
    out->substeps = e->substeps;
    out->rebuilds = c.rebuilds;
    out->home_blocks = c.n_home;
    out->active_blocks = c.n_active;
    out->error_flags = c.error;
    if (!c.error)
        if (int rc = slab_pool_grow(e, c)) return rc;
    note_quiet_time(e, c);   // (a read-only call: the hint its settle() dropped still holds)
    out->active_faces = (uint32_t)c.nfa;
    out->active_vertices = (uint32_t)c.nva;
    out->face_slots = (uint32_t)e->dp.Nf;
    out->vertex_slots = (uint32_t)e->dp.Nv;
    out->resort_checks = e->checks_launched;
    out->quiet_time_s = c.quiet_time;
    out->since_resort_s = c.time_since_resort;
    {
        const DP& p = e->dp;
        size_t pb = 0, sb = 0;
        for (int s = 0; s < 2; ++s) {
            const PSet& S = p.set[s];
            pb += e->bytes_of(S.q[0]) + e->bytes_of(S.pid) + e->bytes_of(S.f8) + e->bytes_of(S.c8) + e->bytes_of(S.xp) + e->bytes_of(p.fg[s]);
            for (int d = 0; d < 4; ++d) pb += e->bytes_of(S.fq[d]);
            for (int d = 0; d < 2; ++d) pb += e->bytes_of(p.vg[s][d]);
        }
        pb += e->bytes_of(p.ta) + e->bytes_of(p.G3) + e->bytes_of(p.VF) + e->bytes_of(p.f[0]) + e->bytes_of(p.pkey) +
              e->bytes_of(p.prank) + e->bytes_of(p.src_of) + e->bytes_of(p.dst_of) + e->bytes_of(p.home_groups);
        sb += e->bytes_of(p.imap) + e->bytes_of(e->d_pids_api) + e->bytes_of(e->d_apimap) + e->bytes_of(p.dist.prev);
        for (int d = 0; d < 3; ++d) sb += e->bytes_of(p.idx_orig[d]);
        sb += e->bytes_of(p.adj_off) + e->bytes_of(p.adj_fc) + e->bytes_of(p.dm_orig);
        out->particle_bytes = pb;
        out->scene_index_bytes = sb;
    }
    out->touched_blocks = 0;
    if (e->grid_state >= 1) {
        uint32_t cnt = 0;
        if (int rc = touched_flags(e, nullptr, &cnt)) return rc;
        out->touched_blocks = cnt;
    }
    return 0;
} MPM_CATCH_ALL

int mpm_grid_touched_cnt(mpm_handle_t e, uint32_t* out) try {
    READY(e);
    REQUIRE(out, "null output");
    *out = 0;
    if (e->grid_state < 1) return 0;
    return touched_flags(e, nullptr, out);
} MPM_CATCH_ALL

int mpm_download_array(mpm_handle_t e, int which, void* out, size_t bytes, size_t* written) try {
    READY(e);
    REQUIRE(out, "null output");
    return download_array(e, which, out, bytes, written);
} MPM_CATCH_ALL

int mpm_upload_particle_state(mpm_handle_t e, const float* pos, const float* vel, const float* affine,
                              const float* volumes, const float* deformation_gradients) try {
    READY(e);
    if (int rc = upload_state(e, pos, vel, affine, volumes, deformation_gradients)) return rc;
    return volumes ? set_fixed_point_scales(e) : 0;
} MPM_CATCH_ALL

int mpm_sync_particle_state_to_cpu(mpm_handle_t e, float* pos_out) try {
    READY(e);
    REQUIRE(pos_out, "null output");
    return download_array(e, MPM_ARR_POSITIONS, pos_out, e->np * 12, nullptr);
} MPM_CATCH_ALL

int mpm_dump_cpu_state(mpm_handle_t e, float* pos_out, int32_t* idx_out) try {
    READY(e);
    if (pos_out) {
        // original vertex order = original ids nf..np (cuda_mpm_model.cu:257-260)
        if (int rc = download_original_vertices(e, pos_out)) return rc;
    }
    if (idx_out) std::copy(e->h_idx.begin(), e->h_idx.end(), idx_out);
    return 0;
} MPM_CATCH_ALL

int mpm_dump_obj(mpm_handle_t e, const char* filename) try {
    READY(e);
    REQUIRE(filename, "null filename");
    std::vector<float> pos(e->nv * 3);
    if (int rc = download_original_vertices(e, pos.data())) return rc;
    std::ofstream obj(filename);
    if (!obj) return fail(MPM_ERR_INVALID, std::string("cannot open ") + filename);
    for (size_t i = 0; i < e->nv; ++i) obj << "v " << pos[i * 3] << " " << pos[i * 3 + 1] << " " << pos[i * 3 + 2] << "\n";
    for (size_t f = 0; f < e->nf; ++f)
        obj << "f " << e->h_idx[f * 3] + 1 << " " << e->h_idx[f * 3 + 1] + 1 << " " << e->h_idx[f * 3 + 2] + 1 << "\n";
    return 0;
} MPM_CATCH_ALL

int mpm_debug_counters(mpm_handle_t e, uint64_t* out16, int reset) try {
    READY(e);
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (out16) D2H(e, out16, e->dp.dbgbuf, 16 * 8);
    if (reset) HIP_TRY(hipMemsetAsync(e->dp.dbgbuf, 0, 16 * 8, e->stream));
    HIP_TRY(hipStreamSynchronize(e->stream));
    return 0;
} MPM_CATCH_ALL

int mpm_debug_resort_tables(mpm_handle_t e, int which, void* out, size_t capacity_bytes, size_t* count_out) try {
    READY(e);
    REQUIRE(out || capacity_bytes == 0, "null output");
    return debug_resort_table(e, which, out, capacity_bytes, count_out);
} MPM_CATCH_ALL

int mpm_debug_sort_pairs(mpm_handle_t e, const uint32_t* keys, const uint32_t* vals, size_t n, int bits, int device_count,
                         int want_in_place, uint32_t* keys_out, uint32_t* vals_out, int info_out[4]) try {
    REQUIRE(e, "null handle");
    if (int rc = use(e)) return rc;
    return debug_sort_pairs(e, keys, vals, n, bits, device_count, want_in_place, keys_out, vals_out, info_out);
} MPM_CATCH_ALL

int mpm_set_dump_dir(mpm_handle_t e, const char* dir) try {
    REQUIRE(e && dir, "null argument");
    e->dump_dir = dir;
    return 0;
} MPM_CATCH_ALL

int mpm_reallocate_external_bodies(mpm_handle_t e, size_t n) try {
    READY(e);
    if (e->cb.resize_bodies(n, e->stream))
        return fail(MPM_ERR_HIP, "ReallocateExternelBodies: device allocation or reset failed");
    return 0;
} MPM_CATCH_ALL

int mpm_external_body_force_to_host(mpm_handle_t e, float* tau_out, float* f_out) try {
    READY(e);
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (e->cb.n_bodies == 0) return 0;
    // (accumulated as integers in 64-bit fixed point, k_ct_impulse: the same bits whatever order the contacts arrived in)
    std::vector<long long> acc(e->cb.n_bodies * 6);
    D2H(e, acc.data(), e->cb.body_acc, acc.size() * sizeof(long long));
    const double unfix = e->cb.imp_unfix > 0.0 ? e->cb.imp_unfix : e->dp.unfix_p;
    for (size_t b = 0; b < e->cb.n_bodies; ++b)
        for (int a = 0; a < 3; ++a) {
            if (tau_out) tau_out[b * 3 + a] = (float)((double)acc[b * 6 + a] * unfix);
            if (f_out) f_out[b * 3 + a] = (float)((double)acc[b * 6 + 3 + a] * unfix);
        }
    return 0;
} MPM_CATCH_ALL

// ---- partitioned domain (mpm_dist_host.h) -----------------------------------------------------------------------------------
int mpm_dist_init(mpm_handle_t e, const mpm_dist_config_t* cfg) try {
    READY(e);
    if (int rc = extensions_refused(e, "mpm_dist_init")) return rc;
    REQUIRE(cfg, "null configuration");
    REQUIRE(!e->dp.dist.on, "mpm_dist_init called twice");
    REQUIRE(e->api_identity, "mpm_dist_init must precede RebuildMapping(sort = true)");
    return dist_init(e, cfg);
} MPM_CATCH_ALL

int mpm_dist_set_headroom(mpm_handle_t e, float factor) try {
    REQUIRE(e, "null handle");
    REQUIRE(!e->dp.dist.on, "mpm_dist_set_headroom must precede mpm_dist_init");
    REQUIRE(factor == 0.f || factor >= 1.f, "headroom must be 0 (keep the whole scene's size) or >= 1");
    e->dist_headroom = factor;
    return 0;
} MPM_CATCH_ALL

int mpm_dist_get_geometry(mpm_handle_t e, mpm_dist_geometry_t* out) try {
    READY_NO_SETTLE(e);
    REQUIRE(out, "null output");
    REQUIRE(e->dp.dist.on, "mpm_dist_init first");
    return dist_get_geometry(e, out);
} MPM_CATCH_ALL

int mpm_dist_retune(mpm_handle_t e, float quiet_time_all, float dt, int* changed_out) try {
    REQUIRE(e, "null handle");
    REQUIRE(e->dp.dist.on, "mpm_dist_init first");
    return dist_retune(e, quiet_time_all, dt, changed_out);
} MPM_CATCH_ALL

int mpm_dist_migration_quiet_time(mpm_handle_t e, float* seconds_out) try {
    READY(e);
    REQUIRE(seconds_out, "null output");
    REQUIRE(e->dp.dist.on, "mpm_dist_init first");
    D2H(e, seconds_out, &e->dp.ctl->mig_quiet, sizeof(float));
    return 0;
} MPM_CATCH_ALL

size_t mpm_dist_migration_buffer_bytes(size_t capacity_particles) { return 16 + capacity_particles * DIST_REC_F4 * 16; }

int mpm_dist_migrate_pack(mpm_handle_t e, void* send_left, void* send_right, size_t capacity_particles) try {
    READY(e);
    REQUIRE(e->dp.dist.on, "mpm_dist_init first");
    REQUIRE(send_left && send_right && capacity_particles > 0 && capacity_particles < (1u << 28), "bad migration buffers");
    return dist_migrate_pack(e, send_left, send_right, capacity_particles);
} MPM_CATCH_ALL

int mpm_dist_plan_migration(const uint32_t* hdr_left, const uint32_t* hdr_right, size_t capacity_particles, size_t scene_faces,
                            size_t scene_vertices, size_t held_faces, size_t held_vertices, size_t face_slots,
                            size_t vertex_slots, float headroom, size_t out6[6]) try {
    REQUIRE(out6, "null output");
    MigrationPlan m;
    if (int rc = plan_migration(hdr_left, hdr_right, capacity_particles, scene_faces, scene_vertices, held_faces, held_vertices,
                                face_slots, vertex_slots, headroom, &m))
        return rc;
    out6[0] = m.in_f; out6[1] = m.in_v; out6[2] = m.need_f; out6[3] = m.need_v; out6[4] = m.want_f; out6[5] = m.want_v;
    return 0;
} MPM_CATCH_ALL

int mpm_dist_migrate_apply(mpm_handle_t e, const void* recv_left, const void* recv_right, size_t capacity_particles) try {
    READY(e);
    REQUIRE(e->dp.dist.on, "mpm_dist_init first");
    REQUIRE(capacity_particles > 0 && capacity_particles < (1u << 28), "bad migration buffers");
    return dist_migrate_apply(e, recv_left, recv_right, capacity_particles);
} MPM_CATCH_ALL

// Tests of the exception barrier and of the allocation-failure paths.  mpm_debug_throw raises a C++ exception of the given
// kind INSIDE an entry point (0: std::bad_alloc, 1: std::length_error via a container asked for an absurd size, 2: a
// non-std exception) and must come back as MPM_ERR_NOMEM / MPM_ERR_INTERNAL; host code only.  mpm_debug_fail_alloc makes the
// engine's n-th device allocation from now fail as if the device were out of memory (0 = off).
int mpm_debug_throw(int kind) try {
    if (kind == 0) throw std::bad_alloc();
    if (kind == 1) {
        std::vector<float> v;
        v.resize(v.max_size() + 1);   // (what an unchecked count from a buffer does to a container)
        return (int)v.size();
    }
    if (kind == 2) throw 42;
    return fail(MPM_ERR_INVALID, "mpm_debug_throw: kind must be 0, 1 or 2");
} MPM_CATCH_ALL

int mpm_debug_fail_alloc(mpm_handle_t e, int nth) try {
    REQUIRE(e, "null handle");
    REQUIRE(nth >= 0, "nth must not be negative");
    e->fail_alloc_countdown = nth;
    return 0;
} MPM_CATCH_ALL

int mpm_dist_set_transport(mpm_handle_t e, mpm_exchange_fn exchange, mpm_allreduce_fn allreduce, void* user,
                           size_t zone_capacity_blocks) try {
    REQUIRE(e, "null handle");
    REQUIRE(zone_capacity_blocks > 0 && zone_capacity_blocks < (1u << 24), "bad zone capacity");
    e->dist_exchange = exchange;
    e->dist_allreduce = allreduce;
    e->dist_user = user;
    e->dist_zone_cap = zone_capacity_blocks;
    return 0;
} MPM_CATCH_ALL

int mpm_dist_roles(mpm_handle_t e, uint8_t* out) try {
    READY(e);
    REQUIRE(out, "null output");
    return dist_roles(e, out);
} MPM_CATCH_ALL

// ---- analytic colliders of the grid update (mpm_bodies_host.h) ------------------------------------------------------------
int mpm_set_grid_colliders(mpm_handle_t e, size_t n, const mpm_grid_collider_t* colliders) try {
    static_assert(sizeof(GridCollider) == sizeof(mpm_grid_collider_t), "grid collider layouts differ");
    REQUIRE(e, "null handle");
    REQUIRE(n <= (size_t)MAX_GRID_COLLIDERS, "too many grid colliders (at most 16)");
    REQUIRE(n == 0 || colliders, "null collider array");
    return set_grid_colliders(e, n, colliders);
} MPM_CATCH_ALL

int mpm_grid_collider_preset(int mpm_bc, float sdf_friction, mpm_grid_collider_t* out, size_t capacity, size_t* n_out) try {
    REQUIRE(n_out, "null argument");
    return grid_collider_preset_out(mpm_bc, sdf_friction, out, capacity, n_out);
} MPM_CATCH_ALL

int mpm_finalize_external_contact_forces(mpm_handle_t e, float dt, float* tau_out, float* f_out) try {
    READY(e);
    REQUIRE(dt > 0.f, "dt must be positive");
    if (int rc = mpm_external_body_force_to_host(e, tau_out, f_out)) return rc;
    // impulses accumulated over the substeps of one plant step -> forces (deformable_driver.h:214-217)
    for (size_t i = 0; i < e->cb.n_bodies * 3; ++i) {
        if (tau_out) tau_out[i] /= dt;
        if (f_out) f_out[i] /= dt;
    }
    return 0;
} MPM_CATCH_ALL

int mpm_spatial_force_shift(size_t n, const float* tau, const float* f, const float* offset, float* tau_out) try {
    REQUIRE(n == 0 || (tau && f && offset && tau_out), "null argument");
    spatial_force_shift(n, tau, f, offset, tau_out);
    return 0;
} MPM_CATCH_ALL

int mpm_external_forces_at_body_origin(size_t n, const float* R_WB, const float* p_BoBq_B, const float* tau,
                                       const float* f, float* tau_Bo_out) try {
    REQUIRE(n == 0 || (R_WB && p_BoBq_B && tau && f && tau_Bo_out), "null argument");
    forces_at_body_origin(n, R_WB, p_BoBq_B, tau, f, tau_Bo_out);
    return 0;
} MPM_CATCH_ALL

int mpm_copy_contact_pairs(mpm_handle_t e, size_t n, const uint32_t* particle, const uint32_t* body, const float* dist,
                           const float* normal, const float* pos, const float* rigid_v, const float* rigid_p_WB) try {
    READY(e);
    REQUIRE(n == 0 || (particle && body && dist && normal && pos && rigid_v && rigid_p_WB), "null contact array");
    return copy_contacts(e, n, particle, body, dist, normal, pos, rigid_v, rigid_p_WB);
} MPM_CATCH_ALL

int mpm_generate_contact_pairs(mpm_handle_t e, size_t n_colliders, const mpm_collider_t* colliders, size_t* n_out) try {
    READY(e);
    REQUIRE(n_colliders == 0 || colliders, "null collider array");
    REQUIRE(n_colliders <= 1024, "too many colliders");
    return generate_contacts(e, n_colliders, colliders, n_out);
} MPM_CATCH_ALL

int mpm_collider_signed_distance(mpm_handle_t e, const mpm_collider_t* c, size_t n, const float* x_W, float* phi_out,
                                 float* grad_W_out) try {
    READY(e);
    REQUIRE(c && (n == 0 || (x_W && phi_out && grad_W_out)), "null argument");
    return collider_signed_distance(e, c, n, x_W, phi_out, grad_W_out);
} MPM_CATCH_ALL

int mpm_sdf_shape_from_mesh(mpm_handle_t e, const float* verts, size_t n_verts, const int32_t* tris, size_t n_tris, float cell,
                            int pad_cells, uint32_t* shape_out) try {
    READY(e);
    REQUIRE(tris && shape_out, "null argument");
    return sdf_shape_from_mesh(e, verts, n_verts, tris, n_tris, cell, pad_cells, shape_out);
} MPM_CATCH_ALL

int mpm_sdf_shape_info(mpm_handle_t e, uint32_t shape, int32_t n[3], float lo[3], float* cell) try {
    READY(e);
    return sdf_shape_info(e, shape, n, lo, cell);
} MPM_CATCH_ALL

int mpm_sdf_shape_download(mpm_handle_t e, uint32_t shape, float* values) try {
    READY(e);
    REQUIRE(values, "null argument");
    return sdf_shape_download(e, shape, values);
} MPM_CATCH_ALL

int mpm_set_sdf_colliders(mpm_handle_t e, size_t n, const mpm_sdf_collider_t* colliders) try {
    READY(e);
    REQUIRE(n == 0 || colliders, "null collider array");
    REQUIRE(n <= 1024, "too many mesh colliders");
    return set_sdf_colliders(e, n, colliders);
} MPM_CATCH_ALL

int mpm_set_body_contact_materials(mpm_handle_t e, size_t n, const mpm_contact_material_t* materials) try {
    REQUIRE(e, "null handle");
    REQUIRE(n == 0 || materials, "null material array");
    if (int rc = validate_body_contact_materials(n, materials)) return rc;   // (before anything is enqueued or allocated)
    READY(e);
    return set_body_contact_materials(e, n, materials);
} MPM_CATCH_ALL

int mpm_get_body_contact_materials(mpm_handle_t e, mpm_contact_material_t* out, size_t capacity, size_t* n_out) try {
    REQUIRE(e, "null handle");
    REQUIRE(capacity == 0 || out, "null argument");
    return copy_out(e->cb.materials, out, capacity, n_out);
} MPM_CATCH_ALL

int mpm_sdf_collider_signed_distance(mpm_handle_t e, const mpm_sdf_collider_t* c, size_t n, const float* x_W, float* phi_out,
                                     float* grad_W_out) try {
    READY(e);
    REQUIRE(c && (n == 0 || (x_W && phi_out && grad_W_out)), "null argument");
    return sdf_collider_signed_distance(e, c, n, x_W, phi_out, grad_W_out);
} MPM_CATCH_ALL

int mpm_download_contact_pairs(mpm_handle_t e, uint32_t* particle, uint32_t* body, float* dist, float* normal,
                               float* pos, float* rigid_v, float* p_WB) try {
    READY(e);
    return download_contacts(e, particle, body, dist, normal, pos, rigid_v, p_WB);
} MPM_CATCH_ALL

int mpm_last_contact_counts(mpm_handle_t e, uint32_t* contacts_out, uint32_t* nodes_out, int* setup_reused_out) try {
    REQUIRE(e, "null handle");
    if (contacts_out) *contacts_out = e->last_contact.contacts;
    if (nodes_out) *nodes_out = e->last_contact.nodes;
    if (setup_reused_out) *setup_reused_out = e->last_contact_reused ? 1 : 0;
    return 0;
} MPM_CATCH_ALL

int mpm_debug_contact_counters(mpm_handle_t e, uint64_t out4[6]) try {
    REQUIRE(e && out4, "null argument");
    for (int k = 0; k < 6; ++k) out4[k] = e->ct_counters[k];
    return 0;
} MPM_CATCH_ALL

// Tests of the invariant "no kernel indexes a per-pair array with a count it has not clamped": overwrites the pair count
// that mpm_generate_contact_pairs left on the device (count >= 0) and / or moves the stamp of the generation that wrote
// it (stamp_delta != 0: the count of "another" generation, i.e. a stale one).  The next mpm_update_contact must refuse.
int mpm_debug_contact_count(mpm_handle_t e, int count, int stamp_delta) try {
    READY(e);
    REQUIRE(e->cb.st && e->cb.dev_counted, "mpm_debug_contact_count: needs pairs counted on the device (mpm_generate_contact_pairs without a count)");
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (count >= 0) H2D(e, &e->cb.st->n, &count, sizeof(int));
    if (stamp_delta) {
        unsigned stamp = 0;
        D2H(e, &stamp, &e->cb.st->n_stamp, sizeof(unsigned));
        stamp += (unsigned)stamp_delta;
        H2D(e, &e->cb.st->n_stamp, &stamp, sizeof(unsigned));
    }
    return 0;
} MPM_CATCH_ALL

// Tests of k_ct_watch alone: see include/mpm_hip.h.  (READY: Finalize's first re-sort has set Ctl::nfa / nva.)
int mpm_debug_contact_watch(mpm_handle_t e, size_t n_colliders, const mpm_collider_t* colliders, int* hit_out) try {
    READY(e);
    REQUIRE(hit_out, "null output");
    REQUIRE(n_colliders == 0 || colliders, "null collider array");
    REQUIRE(n_colliders <= 1024, "too many colliders");
    return debug_contact_watch(e, n_colliders, colliders, hit_out);
} MPM_CATCH_ALL

int mpm_get_contact_pair_count(mpm_handle_t e, size_t* n_out) try {
    READY(e);
    REQUIRE(n_out, "null output");
    if (int rc = resolve_contact_count(e)) return rc;
    *n_out = e->cb.n;
    return 0;
} MPM_CATCH_ALL

int mpm_download_contact_log(mpm_handle_t e, float* rows_out, size_t capacity_rows, size_t* n_rows_out) try {
    READY(e);
    REQUIRE(n_rows_out, "null output");
    static_assert(CT_LOG_F == MPM_CONTACT_LOG_FLOATS, "contact log layouts differ");
    const size_t rows = (size_t)std::min(std::max(e->cb.last_iters, 0), CT_LOG);
    *n_rows_out = rows;
    if (!rows_out || rows == 0) return 0;
    REQUIRE(capacity_rows >= rows, "output array too small");
    REQUIRE(e->cb.it_log, "no contact solve has run");
    D2H(e, rows_out, e->cb.it_log, rows * CT_LOG_F * sizeof(float));
    return 0;
} MPM_CATCH_ALL

int mpm_get_contact_stats(mpm_handle_t e, mpm_contact_stats_t* out) try {
    READY(e);
    REQUIRE(out, "null stats");
    if (int rc = contact_stats_from_device(e)) return rc;
    *out = e->last_contact;
    return 0;
} MPM_CATCH_ALL

int mpm_update_contact(mpm_handle_t e, int frame, int substep, float dt, float mu, float stiffness, float damping,
                       int dump, int exact, int max_iters, int* iters_out, float* residual_out) try {
    READY(e);
    if (iters_out) *iters_out = 0;
    if (residual_out) *residual_out = 0.f;
    e->last_contact = mpm_contact_stats_t{};
    // (a rank of a partitioned domain takes part in the solve whatever its own pair count, on the team transport and on
    // the host-driven ones, once it has a transport: "no contacts" is decided by all ranks together)
    if (!e->cb.dev_counted && e->cb.n == 0 && !(e->dp.dist.on && (e->team.on || (e->dp.dist.world > 1 && (e->dist_allreduce || e->chain.comm))))) return 0;  // cuda_mpm_solver.cu:216-217
    REQUIRE(e->grid_state == 2, "UpdateContact before UpdateGrid");
    return update_contact(e, frame, substep, SolveParams(dt, mu, stiffness, damping, exact, max_iters), dump, iters_out, residual_out,
                          nullptr);
} MPM_CATCH_ALL

static SolveParams solve_params(const mpm_coupled_params_t* prm) {
    return SolveParams(prm->dt, prm->friction_mu, prm->stiffness, prm->damping, prm->exact_line_search, prm->max_newton_iterations);
}

// The body of DeformableDriver::CalcAbstractStates' substep loop (multibody/plant/deformable_driver.h:240-258) for
// rigid bodies with analytic signed distance fields, n times, in one call: RebuildMapping, CalcFemStateAndForce,
// ParticleToGrid, UpdateGrid, CalcMpmContactPairs + CopyContactPairs (on the device), UpdateContact, GridToParticle.
// What the seven calls per substep cost a caller on top of the kernels is the host's share: ~45 launches per coupled
// substep at ~3.5 us each, issued in bursts behind every point where the host has to wait (the solve's end), with the
// caller's own code in between.  Here the host waits exactly once per substep -- for the mailbox word that says the solve
// has converged -- and has the next substep's long kernels (FEM, ParticleToGrid) enqueued before the short ones of the
// contact set-up are due; between two substeps of the call GridToParticle and ParticleToGrid leave out what only a
// download would read (DP::lean_g2p), as mpm_run_substeps does.
// Coupled substeps of a PARTITIONED domain (BASELINE config 5's path): the same loop body on every
// local rank of the team, enqueued phase by phase across them -- halo of the raw node sums over the DIRECT transport, grid
// update, pairs of the particles each rank owns (counted on the device), the TEAM solve (mpm_team.h: zone exchange of the
// per-node Hessian / gradient sums with the neighbours and rank-ordered sums of the line-search rows, all on the engines'
// streams), GridToParticle, impulses (per-rank partial sums).  The host waits once per substep, for the mailbox.  No
// migration in here: the caller runs the substeps between two migrations in one call (DomainChain / LocalWorld decide when
// one is due); no contact-free speculation either -- "does any rank have a pair" is part of the solve's first exchange.
static int team_coupled_substeps(const std::vector<mpm_engine*>& L, int n, const mpm_coupled_params_t* prm, size_t n_colliders,
                                 const mpm_collider_t* colliders, mpm_coupled_result_t* const* results) {
    const float dt = prm->dt;
    for (mpm_engine* e : L) {
        if (int rc = extensions_refused(e, "team coupled substeps")) return rc;
        REQUIRE(e->dp.dist.on && e->team.on && e->chain.direct,
                "coupled substeps on a partitioned domain need the direct halo (mpm_chain_direct_connect) and the team transport (mpm_team_connect)");
        REQUIRE(e->chain.pitch == 0, "coupled substeps: a partitioned domain has pitch 0");
    }
    GridColliders gc;
    if (int rc = grid_colliders_for(L[0], prm->mpm_bc, &gc)) return rc;
    const SolveParams solve = solve_params(prm);
    for (int s = 0; s < n; ++s) {
        for (mpm_engine* e : L)
            if (int rc = chain_direct_begin(e, dt, false)) return rc;
        for (mpm_engine* e : L)
            if (int rc = chain_direct_end(e, dt, prm->mpm_bc, false, false)) return rc;
        for (mpm_engine* e : L)
            if (int rc = generate_contacts(e, n_colliders, colliders, nullptr)) return rc;
        std::vector<SolveOutcome> ocs;
        auto g2p = [&](size_t i) { launch_g2p(L[i], L[i]->dp, dt); };
        if (int rc = team_solve(L, solve, g2p, &ocs)) return rc;
        for (size_t i = 0; i < L.size(); ++i) {
            mpm_engine* e = L[i];
            e->substeps += 1;
            e->grid_state = 2;
            if (results && results[i]) {
                mpm_coupled_result_t& r = results[i][s];
                r.iterations = ocs[i].mb.iters;
                r.contacts = e->last_contact.contacts;
                r.nodes = e->last_contact.nodes;
                r.residual = ocs[i].mb.residual;
                r.setup_reused = 0;
            }
        }
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

// The ranks of ONE partition that live in this process (an in-process world: tests and rehearsals with more ranks than a
// box admits processes), all on one stream: n coupled substeps of the whole world in one call.  results: n_local arrays of
// n entries, or NULL.
int mpm_world_coupled_substeps(mpm_handle_t* handles, int n_local, int n, const mpm_coupled_params_t* prm, size_t n_colliders,
                               const mpm_collider_t* colliders, mpm_coupled_result_t* const* results) try {
    REQUIRE(handles && n_local >= 1 && n_local <= TEAM_MAX && prm && n >= 0, "bad arguments");
    REQUIRE((n_colliders == 0 || colliders) && n_colliders <= 1024, "bad collider array");
    if (int rc = validate_colliders(n_colliders, colliders)) return rc;   // (before any substep is enqueued)
    std::vector<mpm_engine*> L(handles, handles + n_local);
    for (mpm_engine* e : L) {
        // (body ids are global: the ranks solve ONE problem, with one table; refused before anything is enqueued)
        REQUIRE(e, "null handle");
        REQUIRE(same_body_contact_materials(e, L[0]), "the ranks of a world hold different body contact materials");
    }
    for (mpm_engine* e : L) {
        READY(e);
        REQUIRE(e->stream == L[0]->stream, "an in-process world runs on ONE stream (mpm_set_stream)");
        // (colliders: the call's analytic ones and each rank's mesh colliders)
        REQUIRE(n_colliders + e->cb.mesh_set.size() > 0, "bad collider array");
        if (int rc = validate_mesh_bodies(e)) return rc;
    }
    return team_coupled_substeps(L, n, prm, n_colliders, colliders, results);
} MPM_CATCH_ALL

// The state that mpm_run_coupled_substeps carries from one substep to the next.
// Re-sort check launches (four kernels that return at once unless GridToParticle has raised need_rebuild): with every
// substep that may not skip itself; none while the quiet time that the last re-sort estimated lasts -- the host learns
// what is left of it from every solve's publication.  A substep that goes without them and finds a re-sort pending
// skips itself as a whole (DP::gated: transfer kernels, contact solve, GridToParticle) and is run again, with the
// re-sort in front: a wrong guess costs time, not correctness.
// Contact-free stretches (round 5): when a coupled substep had no pairs, a watch kernel behind its GridToParticle asks
// whether the NEXT one would have any (k_ct_watch: exact); the following substeps are then enqueued in chunks WITHOUT
// pair generation, contact solve or any wait, each with its own watch behind it and the gate "skip yourself if a watch
// since `watch_base` has seen a particle in a collider" (DP::gated bit 2).  After a chunk the host synchronises once and
// reads how many of its substeps skipped themselves -- always the last ones: a hit is sticky -- and runs those as
// coupled substeps.  A cloth that falls towards a body costs a contact-free substep plus the watch until it arrives.
struct CoupledSpec {
    bool spec = false;            // the next substeps go in contact-free chunks
    int chunk = 2;                // substeps of the next chunk
    unsigned watch_base = 0;      // the watch that opened the stretch
    bool spec_check = true;       // the next chunk's substeps all carry their re-sort launches
    float spec_quiet_left = 0.f;  // seconds of quiet time left as of the last look at the control block
    bool force_check = true;      // the next coupled substep carries its re-sort launches
};
// (MPM_CT_DEBUG: where the HOST's time of the call goes)
struct CoupledTimes {
    double base = 0, gen = 0, solve = 0, tail = 0;
};

// Coupled substep s of n: pairs, contact solve, GridToParticle in front of the solve's impulses.  *done: 1, or 0 when the
// substep skipped itself as a whole (last_contact_gated) and is to be run again.
static int coupled_substep(mpm_engine* e, int s, int n, const mpm_coupled_params_t* prm, const GridColliders& gc,
                           size_t n_colliders, const mpm_collider_t* colliders, CoupledSpec* sp, CoupledTimes* t,
                           mpm_coupled_result_t* results, int* done) {
    using clk = std::chrono::steady_clock;
    auto since = [](clk::time_point a) { return std::chrono::duration<double, std::micro>(clk::now() - a).count(); };
    const float dt = prm->dt;
    *done = 0;
    auto t0 = clk::now();
    const bool gate = !sp->force_check && (e->ct_gate_always || e->quiet_factor * e->ct_quiet_left > 2.f * dt);
    DP p = e->dp;
    p.gated = gate ? 1 : 0;
    p.lean_g2p = s + 1 < n;
    int iters = 0;
    float residual = 0.f;
    bool g2p_done = false;
    enqueue_substep_front(e, p, dt, gate ? Resort::None : Resort::Lean);
    enqueue_substep_rest(e, GridForm::Fused, p, gc, nullptr, dt);   // (GridToParticle: inside the solve, or below)
    sp->force_check = false;
    e->grid_state = 2;
    t->base += since(t0); t0 = clk::now();
    // (the pair generation's kernels do not read the gate: its pairs are refused with the solve, k_ct_keys)
    if (int rc = generate_contacts(e, n_colliders, colliders, nullptr)) return rc;
    t->gen += since(t0); t0 = clk::now();
    e->last_contact_gated = false;
    if (e->cb.dev_counted || e->cb.n > 0) {
        SolveParams solve = solve_params(prm);
        solve.gated = p.gated;
        if (int rc = update_contact(e, 0, s, solve, 0, &iters, &residual, [&](size_t) {
                launch_g2p(e, p, dt);
                g2p_done = true;
            }))
            return rc;
    } else {
        e->last_contact = mpm_contact_stats_t{};
    }
    t->solve += since(t0); t0 = clk::now();
    if (!g2p_done) launch_g2p(e, p, dt);
    t->tail += since(t0);
    if (e->last_contact_gated) {
        // nothing of this substep has run (its GridToParticle counted it in Ctl::skipped, which belongs to
        // mpm_run_substeps' bookkeeping: cleared): once more, with the re-sort in front
        REQUIRE(gate, "contact solve: a substep with its re-sort launches reported itself as skipped");
        HIP_TRY(hipMemsetAsync(&e->dp.ctl->skipped, 0, sizeof(unsigned), e->stream));
        e->ct_counters[2] += 1;
        e->ct_quiet_left = 0.f;
        sp->force_check = true;
        return 0;
    }
    *done = 1;
    e->substeps += 1;
    if (results) {
        mpm_coupled_result_t& r = results[s];
        r.iterations = iters;
        r.contacts = e->last_contact.contacts;
        r.nodes = e->last_contact.nodes;
        r.residual = residual;
        r.setup_reused = e->last_contact_reused ? 1 : 0;
    }
    // no pairs in this substep: ask whether the next one has any, and go on without pair generation while it has not
    if (!e->ct_no_watch && s + 1 < n && e->last_contact.contacts == 0 && !e->cb.dev_counted) {
        sp->watch_base = ++e->watch_seq;
        launch_contact_watch(e, e->dp, sp->watch_base);
        sp->spec = true;
        sp->spec_check = false;
        sp->spec_quiet_left = quiet_hint(e, e->ct_quiet_left);   // (what the solve's publication said is left of the quiet time)
    }
    return 0;
}

// A contact-free chunk from substep s of n (see CoupledSpec).  *done: how many of its substeps ran.
static int coupled_chunk(mpm_engine* e, int s, int n, float dt, const GridColliders& gc, CoupledSpec* sp,
                         mpm_coupled_result_t* results, int* done) {
    const int m = std::min(sp->chunk, n - s);
    // (the re-sort checks of a chunk: none while the quiet time lasts that the last look at the control block left
    // -- a substep that meets a pending re-sort then skips itself like one that meets a hit, and the chunk's tail is
    // repeated with the checks --, else with every substep)
    float quiet = sp->spec_check ? 0.f : e->quiet_factor * sp->spec_quiet_left;
    for (int q = 0; q < m; ++q) {
        const bool unchecked = quiet > 2.f * dt;
        quiet -= dt;
        DP p = e->dp;
        p.gated = 4 | (unchecked ? 1 : 0);
        p.watch_base = sp->watch_base;
        p.lean_g2p = s + q + 1 < n;
        enqueue_substep_front(e, p, dt, unchecked ? Resort::None : Resort::Lean);
        enqueue_substep_rest(e, GridForm::Fused, p, gc, &p, dt);
        launch_contact_watch(e, p, ++e->watch_seq);
    }
    e->grid_state = 2;
    HIP_TRY(hipStreamSynchronize(e->stream));
    Ctl c;
    D2H(e, &c, e->dp.ctl, sizeof(Ctl));
    const int skipped = (int)std::min<unsigned>(c.skipped, (unsigned)m);
    if (c.skipped) {
        const unsigned zero = 0;
        H2D(e, &e->dp.ctl->skipped, &zero, sizeof(unsigned));
    }
    const int ran = m - skipped;
    const bool hit = (int)(c.watch_hit - sp->watch_base) >= 0;
    e->ct_counters[4] += (uint64_t)m;
    e->ct_counters[5] += (uint64_t)skipped;
    for (int q = 0; q < ran; ++q) {
        e->substeps += 1;
        if (results) results[s + q] = mpm_coupled_result_t{};
    }
    if (ran > 0) {
        e->last_contact = mpm_contact_stats_t{};
        e->last_contact_reused = false;
    }
    // (a non-zero c.skipped sets spec_check, which discards the value, or comes with a hit, which ends the speculation)
    sp->spec_quiet_left = quiet_hint(e, quiet_time_left(c));
    sp->spec_check = skipped > 0;   // (whatever made them skip: the repeated ones carry their checks)
    // (an error flag ends the speculation too: the coupled substep that follows reports it where it always was)
    if (hit || c.error) {
        sp->spec = false;
        sp->chunk = 2;
        sp->force_check = true;
    } else if (skipped > 0) {
        sp->chunk = 2;           // a re-sort was pending: the tail of the chunk again, contact-free, with its checks
    } else {
        sp->chunk = std::min(sp->chunk * 2, 32);
    }
    *done = ran;
    return 0;
}

int mpm_run_coupled_substeps(mpm_handle_t e, int n, const mpm_coupled_params_t* prm, size_t n_colliders,
                             const mpm_collider_t* colliders, mpm_coupled_result_t* results) try {
    READY(e);
    REQUIRE(prm && n >= 0, "bad arguments");
    REQUIRE(n_colliders == 0 || colliders, "null collider array");
    REQUIRE(n_colliders <= 1024, "too many colliders");
    if (int rc = validate_colliders(n_colliders, colliders)) return rc;   // (before any substep is enqueued)
    if (int rc = pins_ready(e)) return rc;
    if (int rc = fields_stable(e, prm->dt)) return rc;
    // colliders: the call's analytic ones and the engine's mesh colliders (mpm_set_sdf_colliders)
    const size_t n_all = n_colliders + e->cb.mesh_set.size();
    if (int rc = validate_mesh_bodies(e)) return rc;
    if (e->dp.dist.on) {
        REQUIRE(n_all > 0, "coupled substeps on a partitioned domain need colliders (contact-free: mpm_chain_substeps)");
        mpm_coupled_result_t* one[1] = {results};
        return team_coupled_substeps({e}, n, prm, n_colliders, colliders, results ? one : nullptr);
    }
    if (n_all == 0) {   // nothing to couple with: contact-free substeps
        if (results)
            for (int s = 0; s < n; ++s) results[s] = mpm_coupled_result_t{};
        return mpm_run_substeps(e, n, prm->dt, prm->mpm_bc);
    }
    GridColliders gc;
    if (int rc = grid_colliders_for(e, prm->mpm_bc, &gc)) return rc;
    struct Report {   // (MPM_CT_DEBUG: per substep, however the function is left)
        mpm_engine* e; int n; CoupledTimes t;
        ~Report() {
            if (e->ct_debug && n > 0)
                std::fprintf(stderr, "[mpm_hip] coupled substeps, host us per substep: base launches %.1f, pairs %.1f, solve (set-up + "
                                     "iterations + waits: %.1f polling) %.1f, GridToParticle %.1f\n", t.base / n, t.gen / n, e->ct_wait_us / n,
                             t.solve / n, t.tail / n);
        }
    } report{e, n, {}};
    e->ct_wait_us = 0;
    CoupledSpec sp;
    for (int s = 0; s < n;) {
        int done = 0;
        if (int rc = sp.spec ? coupled_chunk(e, s, n, prm->dt, gc, &sp, results, &done)
                             : coupled_substep(e, s, n, prm, gc, n_colliders, colliders, &sp, &report.t, results, &done))
            return rc;
        s += done;
    }
    HIP_TRY(hipGetLastError());
    return 0;
} MPM_CATCH_ALL

// The root finder of the exact line search behind a C callback, for the known-answer tests (host code only: no device
// is touched; newton_bisect in mpm_rootfind.h).
int mpm_newton_bisect_f64(mpm_rootfind_fn fn, void* user, double x_lo, double x_hi, double guess, double x_tol, double f_tol,
                          int max_evals, int flags, double* root_out, int* evals_out) try {
    REQUIRE(fn && root_out && evals_out, "null argument");
    REQUIRE(x_lo < x_hi && x_lo <= guess && guess <= x_hi && x_tol > 0 && f_tol > 0, "bad bracket / tolerances");
    return newton_bisect(fn, user, x_lo, x_hi, guess, x_tol, f_tol, max_evals, flags, root_out, evals_out);
} MPM_CATCH_ALL
int mpm_newton_bisect_f32(mpm_rootfind_fn fn, void* user, float x_lo, float x_hi, float guess, float x_tol, float f_tol,
                          int max_evals, int flags, float* root_out, int* evals_out) try {
    REQUIRE(fn && root_out && evals_out, "null argument");
    REQUIRE(x_lo < x_hi && x_lo <= guess && guess <= x_hi && x_tol > 0 && f_tol > 0, "bad bracket / tolerances");
    return newton_bisect(fn, user, x_lo, x_hi, guess, x_tol, f_tol, max_evals, flags, root_out, evals_out);
} MPM_CATCH_ALL

// ---- what the features' entry points share ----------------------------------------------------------------------------------
// the preamble of a setter with one record per cloth: a finalized single engine, and a table of mpm_cloth_count records
// (zero_is_off: or none at all)
static int per_cloth_setter(mpm_engine* e, Feature f, const char* call, size_t n_cloths, const void* table, const char* null_table,
                            bool zero_is_off = true) {
    READY_NO_SETTLE(e);
    if (int rc = single_engine_only(e, FEATURES[f].what_is)) return rc;
    REQUIRE((zero_is_off && n_cloths == 0) || n_cloths == e->cloths.size(),
            std::string(call) + ": n_cloths must be mpm_cloth_count" + (zero_is_off ? " (or 0: off)" : ""));
    REQUIRE(n_cloths == 0 || table, null_table);
    return 0;
}
// mpm_<guard>_max_stable_dt: the guard's limit while the feature is in force, +inf otherwise
static int max_stable_dt_out(const mpm_engine* e, Feature f, float* dt_out) {
    REQUIRE(e && dt_out, "null argument");
    *dt_out = max_stable_dt(feature_state(e), f);
    return 0;
}

// ---- fixed constraints (mpm_bodies_host.h) --------------------------------------------------------------------------------
int mpm_set_pins(mpm_handle_t e, size_t n, const mpm_pin_t* pins) try {
    READY(e);
    if (int rc = single_engine_only(e, FEATURES[F_PINS].what_is)) return rc;
    REQUIRE(n == 0 || pins, "null pin array");
    return set_pins(e, n, pins);
} MPM_CATCH_ALL

int mpm_set_body_motions(mpm_handle_t e, size_t n, const mpm_body_motion_t* m) try {
    READY(e);
    if (int rc = single_engine_only(e, FEATURES[F_PINS].what_is)) return rc;
    REQUIRE(n == 0 || m, "null motion array");
    return set_body_motions(e, n, m);
} MPM_CATCH_ALL

int mpm_pins_inside_collider(mpm_handle_t e, const mpm_collider_t* shape, uint32_t body, const float p_WB[3],
                             const float R_WB[9], size_t* n_added) try {
    READY(e);
    if (int rc = single_engine_only(e, FEATURES[F_PINS].what_is)) return rc;
    REQUIRE(shape && p_WB && R_WB, "null argument");
    return pins_inside_collider(e, shape, body, p_WB, R_WB, n_added);
} MPM_CATCH_ALL

int mpm_get_pins(mpm_handle_t e, mpm_pin_t* out, size_t capacity, size_t* n_out) try {
    READY(e);
    REQUIRE(out || capacity == 0, "null output");
    return copy_out(e->pin.set, out, capacity, n_out);
} MPM_CATCH_ALL

// ---- anchors: springs and cords from cloth vertices to rigid bodies (mpm_bodies_host.h; mpm_anchors.h) ------------------------
int mpm_set_anchors(mpm_handle_t e, size_t n, const mpm_anchor_t* anchors) try {
    READY(e);
    if (int rc = single_engine_only(e, FEATURES[F_ANCHORS].what_is)) return rc;
    REQUIRE(n == 0 || anchors, "null anchor array");
    return set_anchors(e, n, anchors);
} MPM_CATCH_ALL

int mpm_get_anchors(mpm_handle_t e, mpm_anchor_t* out, size_t capacity, size_t* n_out) try {
    READY(e);
    REQUIRE(out || capacity == 0, "null output");
    return copy_out(e->anchors.set, out, capacity, n_out);
} MPM_CATCH_ALL

int mpm_anchor_forces(mpm_handle_t e, float* f_out) try {
    READY(e);
    REQUIRE(f_out, "null output");
    return anchor_forces(e, f_out);
} MPM_CATCH_ALL

int mpm_anchor_state(mpm_handle_t e, double* energy_out, float* length_out, float* point_out, double* impulse_quantum_out) try {
    READY(e);
    return anchor_state(e, energy_out, length_out, point_out, impulse_quantum_out);
} MPM_CATCH_ALL

int mpm_anchors_max_stable_dt(mpm_handle_t e, float* dt_out) try {
    return max_stable_dt_out(e, F_ANCHORS, dt_out);
} MPM_CATCH_ALL

int mpm_anchor_point(const mpm_body_motion_t* motion, double t, const float* p_BQ, float* y, float* v_Q) try {
    REQUIRE(motion && p_BQ, "null argument");
    anchor_point_host(motion, t, p_BQ, y, v_Q);
    return 0;
} MPM_CATCH_ALL

// ---- rigid bodies of the grid update (mpm_bodies_host.h; k_grid_bodies in mpm_grid_bodies.h) ------------------------------
int mpm_set_grid_bodies(mpm_handle_t e, size_t n, const mpm_grid_body_t* bodies) try {
    static_assert(sizeof(Collider) == sizeof(mpm_collider_t), "collider layouts differ");
    READY_NO_SETTLE(e);
    if (int rc = single_engine_only(e, FEATURES[F_GRID_BODIES].what_is)) return rc;
    REQUIRE(n <= (size_t)MAX_GRID_COLLIDERS, "too many grid bodies (at most 16)");
    REQUIRE(n == 0 || bodies, "null grid body array");
    return set_grid_bodies(e, n, bodies);
} MPM_CATCH_ALL

int mpm_get_grid_bodies(mpm_handle_t e, mpm_grid_body_t* out, size_t capacity, size_t* n_out) try {
    REQUIRE(e, "null handle");
    REQUIRE(out || capacity == 0, "null output");
    return copy_out(e->grid_bodies, out, capacity, n_out);
} MPM_CATCH_ALL

// ---- external force fields (mpm_cloth_host.h; mpm_fields.h) -----------------------------------------------------------------
int mpm_set_force_fields(mpm_handle_t e, size_t n, const mpm_force_field_t* fields) try {
    READY_NO_SETTLE(e);
    if (int rc = single_engine_only(e, FEATURES[F_FORCE_FIELDS].what_is)) return rc;
    if (int rc = validate_force_fields(n, fields)) return rc;
    return set_force_fields(e, n, fields);
} MPM_CATCH_ALL

int mpm_get_force_fields(mpm_handle_t e, mpm_force_field_t* out, size_t capacity, size_t* n_out) try {
    REQUIRE(e, "null handle");
    REQUIRE(out || capacity == 0, "null output");
    return copy_out(e->force_fields, out, capacity, n_out);
} MPM_CATCH_ALL

int mpm_force_field_acceleration(const mpm_force_field_t* fields, size_t n_fields, size_t n, const float* x, const float* v,
                                 const float* director, float* acc_out) try {
    if (int rc = validate_force_fields(n_fields, fields)) return rc;
    REQUIRE(n == 0 || (x && v && acc_out), "null argument");
    return force_field_accelerations(fields, n_fields, n, x, v, director, acc_out);
} MPM_CATCH_ALL

// ---- bending stiffness (mpm_cloth_host.h; mpm_bending.h) ----------------------------------------------------------------------
int mpm_bending_matrix(const float* pos, size_t n_verts, const int32_t* indices, size_t n_faces, size_t* row_offsets,
                       int32_t* cols, double* vals, size_t capacity, size_t* nnz_out) try {
    REQUIRE((pos || n_verts == 0) && (indices || n_faces == 0), "null input array");
    REQUIRE(capacity == 0 || (cols && vals), "null output");
    REQUIRE(n_verts < (size_t)1 << 30 && n_faces < (size_t)1 << 30, "mesh too large");
    for (size_t i = 0; i < n_faces * 3; ++i)
        REQUIRE(indices[i] >= 0 && (size_t)indices[i] < n_verts, "triangle index out of range");
    return bending_matrix_out(pos, n_verts, indices, n_faces, row_offsets, cols, vals, capacity, nnz_out);
} MPM_CATCH_ALL

int mpm_set_bending(mpm_handle_t e, size_t n_cloths, const float* stiffness) try {
    if (int rc = per_cloth_setter(e, F_BENDING, "mpm_set_bending", n_cloths, stiffness, "null stiffness array")) return rc;
    if (int rc = tear_refuses(e, n_cloths, "mpm_set_bending", [&](size_t c) { return stiffness[c] > 0.f; })) return rc;
    return set_bending(e, n_cloths, stiffness);
} MPM_CATCH_ALL

int mpm_get_bending(mpm_handle_t e, float* out, size_t capacity, size_t* n_out) try {
    REQUIRE(e, "null handle");
    return padded_out(e->bend.k, e->cloths.size(), 0.f, out, capacity, n_out);
} MPM_CATCH_ALL

int mpm_bending_forces(mpm_handle_t e, float* f_out) try {
    READY(e);
    REQUIRE(f_out || e->nv == 0, "null output");
    return bending_forces(e, f_out);
} MPM_CATCH_ALL

int mpm_bending_max_stable_dt(mpm_handle_t e, float* dt_out) try {
    return max_stable_dt_out(e, F_BENDING, dt_out);
} MPM_CATCH_ALL

// ---- stiffness-proportional damping (mpm_cloth_host.h; mpm_damping.h) ------------------------------------------------------
int mpm_set_damping(mpm_handle_t e, size_t n_cloths, const mpm_cloth_damping_t* d) try {
    if (int rc = per_cloth_setter(e, F_DAMPING, "mpm_set_damping", n_cloths, d, "null damping array")) return rc;
    for (size_t c = 0; c < n_cloths; ++c)
        REQUIRE(std::isfinite(d[c].membrane) && d[c].membrane >= 0.f && std::isfinite(d[c].bending) && d[c].bending >= 0.f,
                "damping: a coefficient is negative or not finite");
    // substeps that mpm_run_substeps deferred are owed with the coefficients they were enqueued with
    if (int rc = settle(e)) return rc;
    return damping_apply(e, n_cloths ? std::vector<mpm_cloth_damping_t>(d, d + n_cloths) : std::vector<mpm_cloth_damping_t>());
} MPM_CATCH_ALL

int mpm_get_damping(mpm_handle_t e, mpm_cloth_damping_t* out, size_t capacity, size_t* n_out) try {
    REQUIRE(e, "null handle");
    return padded_out(e->damp.d, e->cloths.size(), mpm_cloth_damping_t{0.f, 0.f}, out, capacity, n_out);
} MPM_CATCH_ALL

int mpm_damping_forces(mpm_handle_t e, float* f_out) try {
    READY(e);
    REQUIRE(f_out || e->nv == 0, "null output");
    return damping_forces(e, f_out);
} MPM_CATCH_ALL

int mpm_damping_max_stable_dt(mpm_handle_t e, float* dt_out) try {
    return max_stable_dt_out(e, F_DAMPING, dt_out);
} MPM_CATCH_ALL

int mpm_damping_face_records(size_t n_faces, const float* dminv3, const float* vol, const float* mu, const float* lambda,
                             const float* beta, const float* x9, const float* v9, float* rec9_out) try {
    REQUIRE((dminv3 && vol && mu && lambda && beta && x9 && v9 && rec9_out) || n_faces == 0, "null array");
    return damping_face_records(n_faces, dminv3, vol, mu, lambda, beta, x9, v9, rec9_out);
} MPM_CATCH_ALL

// ---- woven cloth (mpm_cloth_host.h; mpm_weave.h) ---------------------------------------------------------------------------
int mpm_set_weave(mpm_handle_t e, size_t n_cloths, const mpm_cloth_weave_t* w, const float* face_dirs) try {
    if (int rc = per_cloth_setter(e, F_WEAVE, "mpm_set_weave", n_cloths, w, "null weave array")) return rc;
    for (size_t c = 0; c < n_cloths; ++c) {
        float coef[4];
        REQUIRE(weave_coefficients(w[c].E_warp, w[c].E_weft, w[c].nu, w[c].G, coef),
                "weave: a constant is negative or not finite, D = 1 - nu^2 E_weft / E_warp <= 0, or E_warp = 0 with nu != 0");
        REQUIRE(finite_n(w[c].warp_dir, 3), "weave: warp_dir is not finite");
    }
    if (face_dirs && n_cloths) REQUIRE(finite_n(face_dirs, (int)(3 * e->nf)), "weave: face_dirs is not finite");
    // substeps that mpm_run_substeps deferred are owed with the table they were enqueued with
    if (int rc = settle(e)) return rc;
    return weave_apply(e, n_cloths ? std::vector<mpm_cloth_weave_t>(w, w + n_cloths) : std::vector<mpm_cloth_weave_t>(), face_dirs);
} MPM_CATCH_ALL

int mpm_get_weave(mpm_handle_t e, mpm_cloth_weave_t* out, size_t capacity, size_t* n_out) try {
    REQUIRE(e, "null handle");
    return padded_out(e->weave.w, e->cloths.size(), mpm_cloth_weave_t{0.f, 0.f, 0.f, 0.f, {0.f, 0.f, 0.f}}, out, capacity, n_out);
} MPM_CATCH_ALL

int mpm_weave_axes(mpm_handle_t e, float* cs_out) try {
    REQUIRE(e, "null handle");
    REQUIRE((e)->finalized, "call mpm_finalize first");
    REQUIRE(cs_out || e->nf == 0, "null output");
    if (e->weave.on()) std::copy(e->weave.axis.begin(), e->weave.axis.end(), cs_out);
    else std::fill(cs_out, cs_out + 2 * e->nf, 0.f);
    return 0;
} MPM_CATCH_ALL

int mpm_weave_forces(mpm_handle_t e, float* f_out, float* rec_out) try {
    READY(e);
    REQUIRE(f_out || e->nv == 0, "null output");
    return weave_eval(e, f_out, rec_out, nullptr, nullptr, 0, nullptr, nullptr);
} MPM_CATCH_ALL

int mpm_weave_strain(mpm_handle_t e, float* out) try {
    READY(e);
    REQUIRE(out || e->nf == 0, "null output");
    return weave_eval(e, nullptr, nullptr, out, nullptr, 0, nullptr, nullptr);
} MPM_CATCH_ALL

int mpm_weave_energy(mpm_handle_t e, double* per_cloth, size_t capacity, size_t* n_out, double* total) try {
    READY(e);
    REQUIRE(per_cloth || capacity == 0, "null output");
    double none = 0.0;
    return weave_eval(e, nullptr, nullptr, nullptr, per_cloth, capacity, n_out, total ? total : &none);
} MPM_CATCH_ALL

int mpm_weave_max_stable_dt(mpm_handle_t e, float* dt_out) try {
    return max_stable_dt_out(e, F_WEAVE, dt_out);
} MPM_CATCH_ALL

int mpm_weave_face_records(size_t n, const float* dminv3, const float* vol, const float* coef4, const float* cs2,
                           const float* x9, float* rec9_out, float* strain3_out, float* energy_out) try {
    REQUIRE((dminv3 && vol && coef4 && cs2 && x9) || n == 0, "null array");
    return weave_face_records(n, dminv3, vol, coef4, cs2, x9, rec9_out, strain3_out, energy_out);
} MPM_CATCH_ALL

int mpm_weave_face_axes(size_t n, const float* rest_x9, const float* dir3, float* cs2_out, int32_t* first_bad_out) try {
    REQUIRE((rest_x9 && dir3 && cs2_out) || n == 0, "null array");
    REQUIRE(n < (size_t)1 << 31, "too many faces");
    return weave_face_axes(n, rest_x9, dir3, cs2_out, first_bad_out);
} MPM_CATCH_ALL

// ---- tearing cloth (mpm_cloth_host.h; mpm_tear.h) ------------------------------------------------------------------------------
int mpm_set_tearing(mpm_handle_t e, size_t n_cloths, const mpm_cloth_tear_t* t) try {
    if (int rc = per_cloth_setter(e, F_TEARING, "mpm_set_tearing", n_cloths, t, "null tearing array", false)) return rc;
    for (size_t c = 0; c < n_cloths; ++c) {
        float L;
        REQUIRE(tear_limit(t[c].stretch_limit, &L), "tearing: a stretch_limit is neither 0 nor a finite number > 1");
    }
    return set_tearing(e, n_cloths, t);
} MPM_CATCH_ALL

int mpm_get_tearing(mpm_handle_t e, mpm_cloth_tear_t* out, size_t capacity, size_t* n_out) try {
    REQUIRE(e, "null handle");
    return padded_out(e->tear.t, e->cloths.size(), mpm_cloth_tear_t{0.f, {0.f, 0.f, 0.f}}, out, capacity, n_out);
} MPM_CATCH_ALL

int mpm_set_torn_faces(mpm_handle_t e, const uint8_t* torn) try {
    READY_NO_SETTLE(e);
    if (int rc = single_engine_only(e, FEATURES[F_TEARING].what_is)) return rc;
    REQUIRE(torn || e->nf == 0, "null flag array");
    return set_torn_faces(e, torn);
} MPM_CATCH_ALL

int mpm_tear_state(mpm_handle_t e, uint8_t* torn_out, uint32_t* count_per_cloth, size_t capacity, size_t* n_out) try {
    READY(e);
    REQUIRE(count_per_cloth || capacity == 0, "null output");
    return tear_state(e, torn_out, count_per_cloth, capacity, n_out);
} MPM_CATCH_ALL

int mpm_tear_measure(mpm_handle_t e, float* mq_out, uint8_t* would_fail_out) try {
    READY(e);
    if (int rc = single_engine_only(e, "mpm_tear_measure is")) return rc;
    return tear_measure(e, mq_out, would_fail_out);
} MPM_CATCH_ALL

int mpm_tear_face(size_t n, const float* dminv3, const float* x9, const float* L, float* mq_out, uint8_t* fails_out) try {
    REQUIRE((dminv3 && x9 && L) || n == 0, "null array");
    return tear_faces(n, dminv3, x9, L, mq_out, fails_out);
} MPM_CATCH_ALL

// ---- tearing composed with shell bending and gas (mpm_cloth_host.h; mpm_shell.h, mpm_pressure.h) -------------------------------
int mpm_set_tear_coupling(mpm_handle_t e, uint32_t mask) try {
    READY_NO_SETTLE(e);
    if (int rc = single_engine_only(e, "tear coupling is")) return rc;
    REQUIRE((mask & ~(MPM_TEAR_CUTS_HINGES | MPM_TEAR_VENTS_GAS)) == 0u, "mpm_set_tear_coupling: unknown bit in the mask");
    // substeps that mpm_run_substeps deferred are owed with the mode they were enqueued with
    if (int rc = settle(e)) return rc;
    return set_tear_coupling(e, mask);
} MPM_CATCH_ALL

int mpm_get_tear_coupling(mpm_handle_t e, uint32_t* mask_out) try {
    REQUIRE(e, "null handle");
    REQUIRE(mask_out, "null output");
    *mask_out = e->tear_coupling;
    return 0;
} MPM_CATCH_ALL

int mpm_shell_cut_hinges(mpm_handle_t e, uint8_t* cut_out, uint32_t* cut_per_cloth, size_t capacity, size_t* n_out) try {
    READY(e);
    if (int rc = single_engine_only(e, "mpm_shell_cut_hinges is")) return rc;
    REQUIRE(cut_per_cloth || capacity == 0, "null output");
    return shell_cut_hinges(e, cut_out, cut_per_cloth, capacity, n_out);
} MPM_CATCH_ALL

int mpm_pressure_vented(mpm_handle_t e, uint8_t* vented_per_cloth, size_t capacity, size_t* n_out) try {
    READY(e);
    if (int rc = single_engine_only(e, "mpm_pressure_vented is")) return rc;
    REQUIRE(vented_per_cloth || capacity == 0, "null output");
    return pressure_vented_cloths(e, vented_per_cloth, capacity, n_out);
} MPM_CATCH_ALL

int mpm_mesh_hinge_faces(const int32_t* indices, size_t n_faces, size_t n_verts, int32_t* faces2, size_t capacity, size_t* n_out) try {
    REQUIRE(indices || n_faces == 0, "null indices");
    REQUIRE(faces2 || capacity == 0, "null output");
    REQUIRE(n_faces < (size_t)1 << 30, "mesh too large");
    for (size_t k = 0; k < 3 * n_faces; ++k)
        REQUIRE(indices[k] >= 0 && (size_t)indices[k] < n_verts, "mpm_mesh_hinge_faces: a vertex id is out of range");
    return mesh_hinge_faces(indices, n_faces, faces2, capacity, n_out);
} MPM_CATCH_ALL

// ---- the rest shape apart from the pose (mpm_cloth_host.h; mpm_rest.h) ----------------------------------------------------------
int mpm_set_rest_shape(mpm_handle_t e, const float* rest_pos) try {
    READY_NO_SETTLE(e);
    if (int rc = single_engine_only(e, FEATURES[F_REST_SHAPE].what_is)) return rc;
    return set_rest_shape(e, rest_pos);
} MPM_CATCH_ALL

int mpm_get_rest_shape(mpm_handle_t e, float* rest_pos_out, int* is_set_out) try {
    REQUIRE(e, "null handle");
    REQUIRE(e->finalized, "call mpm_finalize first");
    if (rest_pos_out) std::copy(e->h_rest.begin(), e->h_rest.end(), rest_pos_out);
    if (is_set_out) *is_set_out = e->rest_set ? 1 : 0;
    return 0;
} MPM_CATCH_ALL

int mpm_rest_shape_check(const float* rest_pos, size_t n_verts, const int32_t* indices, size_t n_faces, int32_t* first_bad_face_out) try {
    REQUIRE((rest_pos || n_verts == 0) && (indices || n_faces == 0), "null array");
    REQUIRE(n_faces < (size_t)1 << 31, "too many faces");
    return rest_shape_check(rest_pos, n_verts, indices, n_faces, first_bad_face_out);
} MPM_CATCH_ALL

// ---- links between cloth vertices (mpm_cloth_host.h; mpm_links.h) --------------------------------------------------------------
int mpm_set_links(mpm_handle_t e, size_t n, const mpm_link_t* links) try {
    READY_NO_SETTLE(e);
    if (int rc = single_engine_only(e, FEATURES[F_LINKS].what_is)) return rc;
    REQUIRE(n == 0 || links, "null link array");
    return set_links(e, n, links);
} MPM_CATCH_ALL

int mpm_get_links(mpm_handle_t e, mpm_link_t* out, size_t capacity, size_t* n_out) try {
    REQUIRE(e, "null handle");
    REQUIRE(out || capacity == 0, "null output");
    return copy_out(e->links.set, out, capacity, n_out);
} MPM_CATCH_ALL

int mpm_link_forces(mpm_handle_t e, float* f_out) try {
    READY(e);
    REQUIRE(f_out || e->nv == 0, "null output");
    return link_forces(e, f_out);
} MPM_CATCH_ALL

int mpm_link_energy(mpm_handle_t e, double* energy_out, float* length_out) try {
    READY(e);
    REQUIRE(energy_out, "null output");
    return link_energy(e, energy_out, length_out);
} MPM_CATCH_ALL

int mpm_links_max_stable_dt(mpm_handle_t e, float* dt_out) try {
    return max_stable_dt_out(e, F_LINKS, dt_out);
} MPM_CATCH_ALL

int mpm_link_force(const mpm_link_t* link, const float* xa, const float* xb, const float* va, const float* vb, float* f_on_a) try {
    REQUIRE(link && xa && xb && va && vb && f_on_a, "null argument");
    const float d[3] = {xb[0] - xa[0], xb[1] - xa[1], xb[2] - xa[2]}, w[3] = {vb[0] - va[0], vb[1] - va[1], vb[2] - va[2]};
    link_force(link->stiffness, link->rest_length, link->damping, (link->flags & MPM_LINK_TENSION_ONLY) != 0u, d, w, f_on_a);
    return 0;
} MPM_CATCH_ALL

// ---- breakable links (mpm_cloth_host.h; mpm_links.h) ----------------------------------------------------------------------------
int mpm_set_link_limits(mpm_handle_t e, size_t n, const float* break_length) try {
    READY_NO_SETTLE(e);
    if (int rc = single_engine_only(e, "link limits are")) return rc;
    REQUIRE(n == 0 || n == e->links.set.size(), "mpm_set_link_limits: n must be the link count or 0");
    REQUIRE(n == 0 || break_length, "null limit array");
    std::vector<float> limits(break_length, break_length + n), B2(std::max<size_t>(n, 1));
    const std::string refusal = link_limits(limits.data(), reinterpret_cast<const Link*>(e->links.set.data()), n, B2.data());
    if (!refusal.empty()) return fail(MPM_ERR_INVALID, refusal);
    // substeps that mpm_run_substeps deferred are owed with the limits they were enqueued with
    if (int rc = settle(e)) return rc;
    return link_break_apply(e, limits, nullptr);
} MPM_CATCH_ALL

int mpm_get_link_limits(mpm_handle_t e, float* out, size_t capacity, size_t* n_out) try {
    REQUIRE(e, "null handle");
    return padded_out(e->links.limits, e->links.set.size(), 0.f, out, capacity, n_out);
} MPM_CATCH_ALL

int mpm_set_broken_links(mpm_handle_t e, size_t n, const uint8_t* broken) try {
    READY_NO_SETTLE(e);
    if (int rc = single_engine_only(e, "breakable links are")) return rc;
    REQUIRE(n == e->links.set.size(), "mpm_set_broken_links: n must be the link count");
    REQUIRE(n == 0 || broken, "null flag array");
    if (int rc = settle(e)) return rc;
    return link_break_apply(e, e->links.limits, broken);
} MPM_CATCH_ALL

int mpm_link_break_state(mpm_handle_t e, uint8_t* broken_out, uint32_t* count_out) try {
    READY(e);
    return link_break_state(e, broken_out, count_out);
} MPM_CATCH_ALL

int mpm_link_break_measure(mpm_handle_t e, float* l2_out, uint8_t* would_break_out) try {
    READY(e);
    if (int rc = single_engine_only(e, "mpm_link_break_measure is")) return rc;
    return link_break_measure(e, l2_out, would_break_out);
} MPM_CATCH_ALL

int mpm_link_breaks(size_t n, const float* xa3, const float* xb3, const float* B2, float* l2_out, uint8_t* breaks_out) try {
    REQUIRE((xa3 && xb3 && B2) || n == 0, "null array");
    return link_breaks_host(n, xa3, xb3, B2, l2_out, breaks_out);
} MPM_CATCH_ALL

// ---- enclosed-volume pressure per cloth (mpm_cloth_host.h; mpm_pressure.h) ------------------------------------------------------
int mpm_set_pressure(mpm_handle_t e, size_t n_cloths, const mpm_cloth_pressure_t* per_cloth) try {
    if (int rc = per_cloth_setter(e, F_PRESSURE, "mpm_set_pressure", n_cloths, per_cloth, "null pressure array")) return rc;
    // (with MPM_TEAR_VENTS_GAS in force, mpm_set_tear_coupling, gas mode alone composes with tearing)
    if (int rc = tear_refuses(e, n_cloths, "mpm_set_pressure", [&](size_t c) {
            return per_cloth[c].mode != MPM_PRESSURE_OFF && !tear_couples_pressure(e, per_cloth[c].mode);
        })) return rc;
    return set_pressure(e, n_cloths, per_cloth);
} MPM_CATCH_ALL

int mpm_get_pressure(mpm_handle_t e, mpm_cloth_pressure_t* out, size_t capacity, size_t* n_out) try {
    REQUIRE(e, "null handle");
    return padded_out(e->pressure.set, e->cloths.size(), mpm_cloth_pressure_t{MPM_PRESSURE_OFF, 0.f, 0.f, 0.f, 0.f}, out, capacity, n_out);
} MPM_CATCH_ALL

int mpm_pressure_forces(mpm_handle_t e, float* f_out) try {
    READY(e);
    REQUIRE(f_out || e->nv == 0, "null output");
    return pressure_forces(e, f_out);
} MPM_CATCH_ALL

int mpm_pressure_state(mpm_handle_t e, mpm_cloth_pressure_state_t* out, size_t capacity, size_t* n_out) try {
    READY(e);
    if (int rc = single_engine_only(e, "mpm_pressure_state is")) return rc;
    REQUIRE(out || capacity == 0, "null output");
    return pressure_state(e, out, capacity, n_out);
} MPM_CATCH_ALL

int mpm_mesh_is_closed(const int32_t* indices, size_t n_faces, size_t n_verts, int32_t* edge_out) try {
    REQUIRE(indices || n_faces == 0, "null indices");
    for (size_t k = 0; k < 3 * n_faces; ++k)
        REQUIRE(indices[k] >= 0 && (size_t)indices[k] < n_verts, "mpm_mesh_is_closed: a vertex id is out of range");
    int32_t edge[2] = {0, 0};
    const bool closed = mesh_is_closed(indices, n_faces, edge);
    if (!closed && edge_out) {
        edge_out[0] = edge[0];
        edge_out[1] = edge[1];
    }
    return closed ? 1 : 0;
} MPM_CATCH_ALL

int mpm_pressure_vertex_force(float g, const float* x_own, size_t n, const float* x_b, const float* x_c, float* f_out) try {
    REQUIRE(x_own && f_out && (n == 0 || (x_b && x_c)), "null argument");
    pressure_vertex_force(g, x_own, n, x_b, x_c, f_out);
    return 0;
} MPM_CATCH_ALL

// ---- shell bending about a curved rest shape (mpm_cloth_host.h; mpm_shell.h) -------------------------------------------------------
int mpm_set_shell_bending(mpm_handle_t e, size_t n_cloths, const mpm_cloth_shell_t* per_cloth, const float* rest_pos) try {
    if (int rc = per_cloth_setter(e, F_SHELL, "mpm_set_shell_bending", n_cloths, per_cloth, "null shell bending array")) return rc;
    // (with MPM_TEAR_CUTS_HINGES in force, mpm_set_tear_coupling, shell bending composes with tearing)
    if (int rc = tear_refuses(e, n_cloths, "mpm_set_shell_bending", [&](size_t c) {
            return per_cloth[c].stiffness > 0.f && !tear_couples_shell(e);
        })) return rc;
    return set_shell_bending(e, n_cloths, per_cloth, rest_pos);
} MPM_CATCH_ALL

int mpm_get_shell_bending(mpm_handle_t e, mpm_cloth_shell_t* out, size_t capacity, size_t* n_out) try {
    REQUIRE(e, "null handle");
    return padded_out(e->shell.set, e->cloths.size(), mpm_cloth_shell_t{0.f, MPM_SHELL_REST_SHAPE}, out, capacity, n_out);
} MPM_CATCH_ALL

int mpm_shell_hinges(mpm_handle_t e, int32_t* ids4, float* kc, float* psibar, size_t capacity, size_t* n_out) try {
    REQUIRE(e, "null handle");
    REQUIRE(capacity == 0 || (ids4 && kc && psibar), "null output");
    const mpm_engine::Shell& sh = e->shell;
    const size_t n = std::min(capacity, sh.kc.size());
    std::copy(sh.ids4.begin(), sh.ids4.begin() + (long)(4 * n), ids4);
    std::copy(sh.kc.begin(), sh.kc.begin() + (long)n, kc);
    std::copy(sh.psibar.begin(), sh.psibar.begin() + (long)n, psibar);
    if (n_out) *n_out = sh.kc.size();
    return 0;
} MPM_CATCH_ALL

int mpm_shell_forces(mpm_handle_t e, float* f_out) try {
    READY(e);
    REQUIRE(f_out || e->nv == 0, "null output");
    return shell_forces(e, f_out);
} MPM_CATCH_ALL

int mpm_shell_state(mpm_handle_t e, double* energy_per_cloth, float* psi_out, uint32_t* inactive_out) try {
    READY(e);
    REQUIRE(energy_per_cloth || e->cloths.empty(), "null output");
    return shell_state(e, energy_per_cloth, psi_out, inactive_out);
} MPM_CATCH_ALL

int mpm_shell_max_stable_dt(mpm_handle_t e, float* dt_out) try {
    return max_stable_dt_out(e, F_SHELL, dt_out);
} MPM_CATCH_ALL

int mpm_mesh_hinges(const int32_t* indices, size_t n_faces, size_t n_verts, int32_t* ids4, size_t capacity, size_t* n_out) try {
    REQUIRE(indices || n_faces == 0, "null indices");
    REQUIRE(ids4 || capacity == 0, "null output");
    REQUIRE(n_faces < (size_t)1 << 30, "mesh too large");
    for (size_t k = 0; k < 3 * n_faces; ++k)
        REQUIRE(indices[k] >= 0 && (size_t)indices[k] < n_verts, "mpm_mesh_hinges: a vertex id is out of range");
    std::vector<ShellHinge> H;
    mesh_hinges(indices, n_faces, H);
    for (size_t h = 0; h < std::min(capacity, H.size()); ++h)
        for (int j = 0; j < 4; ++j) ids4[4 * h + j] = H[h].v[j];
    if (n_out) *n_out = H.size();
    return 0;
} MPM_CATCH_ALL

int mpm_shell_hinge(const float* x12, float kc, float psibar, float* rec12_out, float* psi_out) try {
    REQUIRE(x12 && rec12_out, "null argument");
    float rec[4][3], psi;
    const int on = shell_hinge(x12, x12 + 3, x12 + 6, x12 + 9, kc, psibar, rec, &psi) ? 1 : 0;
    std::memcpy(rec12_out, rec, sizeof rec);
    if (psi_out) *psi_out = psi;
    return on;
} MPM_CATCH_ALL

// ---- hinge damping: state of shell bending (mpm_cloth_host.h; mpm_shell.h HINGE DAMPING) ---------------------------------------
int mpm_set_shell_damping(mpm_handle_t e, size_t n_cloths, const mpm_cloth_shell_damping_t* per_cloth) try {
    READY_NO_SETTLE(e);
    if (int rc = single_engine_only(e, "shell damping is")) return rc;
    REQUIRE(e->shell.on(), "shell damping needs shell bending (mpm_set_shell_bending) on");
    REQUIRE(n_cloths == 0 || n_cloths == e->cloths.size(), "mpm_set_shell_damping: n_cloths must be the cloth count or 0");
    REQUIRE(n_cloths == 0 || per_cloth, "null shell damping array");
    const std::string refusal = shell_damping_refusal(reinterpret_cast<const ClothShellDamping*>(per_cloth), n_cloths);
    if (!refusal.empty()) return fail(MPM_ERR_INVALID, refusal);
    // substeps that mpm_run_substeps deferred are owed with the table they were enqueued with
    if (int rc = settle(e)) return rc;
    return set_shell_damping(e, n_cloths, per_cloth);
} MPM_CATCH_ALL

int mpm_get_shell_damping(mpm_handle_t e, mpm_cloth_shell_damping_t* out, size_t capacity, size_t* n_out) try {
    REQUIRE(e, "null handle");
    return padded_out(e->shell.damping, e->cloths.size(), mpm_cloth_shell_damping_t{0.f, 0.f}, out, capacity, n_out);
} MPM_CATCH_ALL

int mpm_shell_damping_forces(mpm_handle_t e, float* f_out) try {
    READY(e);
    REQUIRE(f_out || e->nv == 0, "null output");
    return shell_damping_forces(e, f_out);
} MPM_CATCH_ALL

int mpm_shell_damping_state(mpm_handle_t e, double* power_per_cloth, float* psidot_out) try {
    READY(e);
    REQUIRE(power_per_cloth || e->cloths.empty(), "null output");
    return shell_damping_state(e, power_per_cloth, psidot_out);
} MPM_CATCH_ALL

int mpm_shell_hinge_damped(const float* x12, const float* v12, float kc, float psibar, float bkc, float* rec12_out, float* psi_out,
                           float* psidot_out) try {
    REQUIRE(x12 && v12 && rec12_out, "null argument");
    float rec[4][3], psi, psidot, power;
    const int on = shell_hinge_damped(reinterpret_cast<const float(*)[3]>(x12), reinterpret_cast<const float(*)[3]>(v12), kc, psibar, bkc,
                                      rec, &psi, &psidot, &power) ? 1 : 0;
    std::memcpy(rec12_out, rec, sizeof rec);
    if (psi_out) *psi_out = psi;
    if (psidot_out) *psidot_out = psidot;
    return on;
} MPM_CATCH_ALL

// ---- creases: plastic shell hinges (mpm_cloth_host.h; mpm_shell.h) ----------------------------------------------------------------
// what the crease setters check first
static int creases_ready(mpm_engine* e, const char* what_is) {
    if (int rc = single_engine_only(e, what_is)) return rc;
    REQUIRE(e->shell.on(), "creases need shell bending (mpm_set_shell_bending) on");
    return 0;
}
int mpm_set_creases(mpm_handle_t e, size_t n_cloths, const mpm_cloth_crease_t* per_cloth) try {
    READY_NO_SETTLE(e);
    if (int rc = creases_ready(e, "creases are")) return rc;
    REQUIRE(n_cloths == 0 || n_cloths == e->cloths.size(), "mpm_set_creases: n_cloths must be the cloth count or 0");
    REQUIRE(n_cloths == 0 || per_cloth, "null crease array");
    std::vector<mpm_cloth_crease_t> table(per_cloth, per_cloth + n_cloths);
    std::vector<float> yep(3 * std::max<size_t>(n_cloths, 1));
    const std::string refusal = crease_params(reinterpret_cast<const ClothCrease*>(table.data()), n_cloths, yep.data());
    if (!refusal.empty()) return fail(MPM_ERR_INVALID, refusal);
    // substeps that mpm_run_substeps deferred are owed with the parameters they were enqueued with
    if (int rc = settle(e)) return rc;
    return crease_apply(e, table, false, nullptr);
} MPM_CATCH_ALL

int mpm_get_creases(mpm_handle_t e, mpm_cloth_crease_t* out, size_t capacity, size_t* n_out) try {
    REQUIRE(e, "null handle");
    return padded_out(e->shell.crease, e->cloths.size(), mpm_cloth_crease_t{0.f, 0.f, 0.f, 0.f}, out, capacity, n_out);
} MPM_CATCH_ALL

int mpm_set_crease_state(mpm_handle_t e, const float* psibar) try {
    READY_NO_SETTLE(e);
    if (int rc = creases_ready(e, "creases are")) return rc;
    if (int rc = settle(e)) return rc;
    return crease_apply(e, e->shell.crease, true, psibar);
} MPM_CATCH_ALL

int mpm_crease_state(mpm_handle_t e, float* psibar_out, uint32_t* creased_per_cloth, size_t capacity, size_t* n_out) try {
    READY(e);
    REQUIRE(creased_per_cloth || capacity == 0, "null output");
    return crease_state(e, psibar_out, creased_per_cloth, capacity, n_out);
} MPM_CATCH_ALL

int mpm_crease_measure(mpm_handle_t e, float* psi_out, float* dpsi_out, float* psibar_next_out) try {
    READY(e);
    if (int rc = single_engine_only(e, "mpm_crease_measure is")) return rc;
    return crease_measure(e, psi_out, dpsi_out, psibar_next_out);
} MPM_CATCH_ALL

int mpm_crease_hinge(size_t n, const float* x12, const float* psibar, const float* y, const float* eta, const float* P, float* psi_out,
                     float* dpsi_out, float* psibar_out, uint8_t* yields_out) try {
    REQUIRE((x12 && psibar && y && eta && P) || n == 0, "null array");
    return crease_hinge_host(n, x12, psibar, y, eta, P, psi_out, dpsi_out, psibar_out, yields_out);
} MPM_CATCH_ALL

// ---- the per-cloth report (mpm_cloth_host.h; mpm_measure.h) --------------------------------------------------------------------
int mpm_measure(mpm_handle_t e, mpm_cloth_measure_t* per_cloth, size_t capacity, size_t* n_cloths_out,
                mpm_cloth_measure_t* total) try {
    READY(e);
    REQUIRE(per_cloth || capacity == 0, "null output");
    return measure_cloths(e, per_cloth, capacity, n_cloths_out, total);
} MPM_CATCH_ALL

int mpm_face_strain(mpm_handle_t e, float* out) try {
    READY_NO_SETTLE(e);
    if (int rc = single_engine_only(e, "mpm_face_strain is")) return rc;
    REQUIRE(out || e->nf == 0, "null output");
    if (int rc = settle(e)) return rc;
    return face_strain(e, out);
} MPM_CATCH_ALL

int mpm_cloth_energy_density(const mpm_cloth_material_t* m, size_t n, const float* F, double* out) try {
    REQUIRE(m, "null material");
    REQUIRE((F && out) || n == 0, "null array");
    return cloth_energy_densities(m, n, F, out);
} MPM_CATCH_ALL

}  // extern "C"
