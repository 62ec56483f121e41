// Host-side engine object shared by the C-ABI implementation: mpm_engine.hip (every entry point, the substep's launch
// sequence, settle and the drivers) and the host headers it includes -- mpm_io.h, mpm_contact.h, mpm_sort.h, and per
// feature mpm_cloth_host.h, mpm_bodies_host.h, mpm_dist_host.h, mpm_chain_host.h.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <exception>
#include <functional>
#include <new>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/mpm_hip.h"
#include "mpm_device.h"
#include "mpm_features.h"
#include "mpm_rebuild.h"
#include "mpm_step.h"
#include "mpm_contact_dev.h"
#include "mpm_pins.h"
#include "mpm_bending.h"
#include "mpm_damping.h"
#include "mpm_weave.h"
#include "mpm_tear.h"
#include "mpm_rest.h"
#include "mpm_links.h"
#include "mpm_pressure.h"
#include "mpm_shell.h"
#include "mpm_anchors.h"
#include "mpm_measure.h"
#include "mpm_grid_bodies.h"
#include "mpm_team.h"
#include "mpm_trace.h"

using namespace mpm;

static thread_local std::string g_last_error;

// (never throws: the message of a failure must not become a second failure -- the catch-all of the C ABI calls this)
static int fail(int code, const std::string& msg) noexcept {
    try {
        g_last_error = msg;
    } catch (...) {
        g_last_error.clear();
    }
    return code;
}
static int fail(int code, const char* msg) noexcept {
    try {
        g_last_error = msg;
    } catch (...) {
        g_last_error.clear();
    }
    return code;
}

// The exception barrier of the C ABI (include/mpm_hip.h: "errors never kill the caller", the reference's
// settings.h:11-25 contract turned round: CUDA_SAFE_CALL throws only in DEBUG builds, nothing else does).  Every
// extern "C" entry point is a function-try-block that ends in MPM_CATCH_ALL: a C++ exception raised anywhere below it
// (std::bad_alloc / std::length_error from a container sized by a count that came off the device or out of a buffer, a
// std::function that is empty, an ofstream failure with exceptions on ...) becomes a status code and a message instead
// of std::terminate -- which, inside Drake, would take the whole simulation process down.
static int exception_to_status() noexcept {
    try {
        throw;
    } catch (const std::bad_alloc&) {
        return fail(MPM_ERR_NOMEM, "host memory exhausted (std::bad_alloc) inside the engine");
    } catch (const std::exception& ex) {
        try {
            return fail(MPM_ERR_INTERNAL, std::string("C++ exception inside the engine: ") + ex.what());
        } catch (...) {
            return fail(MPM_ERR_INTERNAL, "C++ exception inside the engine");
        }
    } catch (...) {
        return fail(MPM_ERR_INTERNAL, "unknown C++ exception inside the engine");
    }
}
#define MPM_CATCH_ALL \
    catch (...) { return exception_to_status(); }

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e__ = (expr);                                                                        \
        if (e__ != hipSuccess)                                                                          \
            return fail(e__ == hipErrorOutOfMemory ? MPM_ERR_NOMEM : MPM_ERR_HIP,                       \
                        std::string(#expr) + ": " + hipGetErrorString(e__));                            \
    } while (0)

#define REQUIRE(cond, msg)                                   \
    do {                                                     \
        if (!(cond)) return fail(MPM_ERR_INVALID, (msg));    \
    } while (0)

constexpr size_t MAX_CLOTH_MATERIALS = 256;

// What the caller of a contact solve sets (mpm_update_contact, mpm_coupled_params_t)
struct SolveParams {
    float dt = 0.f, mu = 0.f, stiffness = 0.f, damping = 0.f;
    int exact = 0, max_iters = 0;
    int gated = 0;   // DP::gated of the coupled substep the solve belongs to (k_ct_keys reads its verdict); 0: none
    SolveParams() = default;
    SolveParams(float dt, float mu, float stiffness, float damping, int exact, int max_iters)
        : dt(dt), mu(mu), stiffness(stiffness), damping(damping), exact(exact), max_iters(max_iters > 0 ? max_iters : 2000) {}   // cuda_mpm_solver.cu:234
};

struct mpm_engine {
    std::atomic<int> pins{0};   // mpm_device_synchronize of another thread is working on this engine (mpm_destroy waits)
    int device = 0;
    int bits = 7;
    mpm_material_t mat{};
    hipStream_t stream = nullptr, own_stream = nullptr;
    bool finalized = false;
    // staged cloth (AddQRCloth)
    std::vector<float> h_pos, h_vel;
    std::vector<int> h_idx;  // vertex ids local to the vertex array
    // the rest shape (mpm_set_rest_shape; mpm_rest.h): the vertex positions the rest state in force was computed from --
    // h_pos from mpm_finalize until the call.  What derives a table from the rest shape reads this, not the pose h_pos.
    std::vector<float> h_rest;
    bool rest_set = false;   // a rest shape other than the positions as added is in force
    size_t nv = 0, nf = 0, np = 0;
    // every cloth in call order, and the per-cloth materials (mpm_add_qr_cloth_with_material: at most
    // MAX_CLOTH_MATERIALS cloths; a face's cloth rides in fq[3].x, see FACE_CLOTH_SHIFT)
    struct Cloth {
        size_t first_vertex, n_verts, first_face, n_faces;
        mpm_cloth_material_t m;
    };
    std::vector<Cloth> cloths;
    bool multi_mat = false;             // some cloth came with a material of its own: k_fem_mat, q[0].w holds the mass
    ClothMat* d_cloth_mat = nullptr;    // [cloth] k_fem_mat's table (multi-material engines)
    std::vector<float> h_rho_of_pid;    // [original particle id] the density of its cloth (multi-material engines)
    // Per-launch fields (gated, lean_g2p, lean_resort, watch_base, anticip, every halo_* field) keep mpm_finalize's values
    // for the engine's life: a launch that needs one sets it in a copy of its own (launch_rebuild, enqueue_substep_*).
    DP dp{};
    std::vector<void*> allocs;
    std::vector<size_t> alloc_bytes;   // (parallel to allocs)
    // slot (API) order bookkeeping: slot -> original id and its inverse
    int* d_pids_api = nullptr;
    int* d_apimap = nullptr;
    // RebuildMapping(sort = true): scratch of the device radix sort, second pids buffer
    uint32_t *d_sort_keys = nullptr, *d_sort_vals = nullptr, *d_sort_keys2 = nullptr, *d_sort_vals2 = nullptr;
    int* d_sort_hist = nullptr;
    float last_dt = 0.f;   // length of the last substep (anticipatory binning of the re-sort)
    // gated substeps of mpm_run_substeps (see gated_out in mpm_step.h)
    // the re-sort launches precede every check_every-th substep of mpm_run_substeps (1 = all); read from
    // MPM_RESORT_EVERY when the engine is created: per handle, not per process
    int check_every = 4;
    unsigned step_phase = 0;
    bool force_check = true;   // the next substep gets them whatever its number (after any other call)
    float quiet_left = 0.f;    // seconds of Ctl::quiet_time left as of the last settle() (0: unknown)
    // phase calls of a substep in the reference's order that have been accepted but not launched (mpm_engine.hip,
    // mpm_rebuild_mapping): n of RebuildMapping(false), CalcFemStateAndForce(dt), ParticleToGrid(dt), UpdateGrid(bc)
    struct PendingPhases {
        int n = 0;
        float dt = 0.f;
        int bc = 0;
    } pend;
    bool defer_phases = true;       // MPM_DEFER_PHASES=0: every phase call launches its kernels at once
    uint64_t checks_launched = 0;   // (diagnostics)
    Ctl* h_ctl = nullptr;           // pinned landing place of the control block (settle)
    bool settle_read_ctl = false;   // settle() handed its copy of the control block to the caller (mpm_sync)
    float quiet_factor = .5f;  // share of it that is trusted (MPM_QUIET_FACTOR; 0 = check launches as before)
    bool maybe_owed = false;   // gated substeps were enqueued since the last settle()
    float owed_dt = 0.f;
    int owed_bc = 0;
    uint64_t owed_gcv = 0;
    int* d_pids_api2 = nullptr;
    int* d_iota = nullptr;     // identity map, created on first use (views in original order)
    bool api_identity = true;
    bool deterministic = getenv("MPM_DETERMINISTIC") != nullptr;  // see mpm_set_deterministic
    // mpm_set_fast_math / MPM_FAST_MATH=1: k_fem's divisions and square roots by the hardware approximation + one Newton
    // step (mpm_math.h, FM = 1) instead of correctly rounded (the default)
    bool fast_math = getenv("MPM_FAST_MATH") != nullptr && atoi(getenv("MPM_FAST_MATH")) != 0;
    bool p2g_fixed_point = getenv("MPM_P2G_FIXED") != nullptr;    // the fixed-point LDS tile of k_p2g outside deterministic mode too (A/B)
    // native chain (mpm_chain_*): communicator, neighbours, device buffers
    struct Chain {
        void* comm = nullptr;
        int rank = 0, world = 1, left = -1, right = -1;
        int zone_lo[2] = {0, 0}, zone_hi[2] = {0, 0}, pitch = 0;
        size_t cap = 0, bytes = 0;
        void *send_l = nullptr, *send_r = nullptr, *recv_l = nullptr, *recv_r = nullptr;
        // partitioned domain: migration records every mig_every substeps
        int mig_every = 0;         // 0 with mig_cap > 0: adaptive (see mpm_chain_substeps)
        float mig_budget = 0.f, mig_elapsed = 0.f;   // adaptive cadence: seconds until the next migration / since the last
        float* mig_quiet_all = nullptr;              // device: the ranks' common estimate (ncclMin)
        size_t mig_cap = 0, mig_bytes = 0;
        void *mig_send_l = nullptr, *mig_send_r = nullptr, *mig_recv_l = nullptr, *mig_recv_r = nullptr;
        uint64_t steps = 0;
        // DIRECT halo (mpm_chain_direct_*): the pack kernel stores the zone sums straight into the NEIGHBOUR's receive
        // buffer (peer memory mapped through an IPC handle), a one-thread kernel raises a sequence flag over there, the
        // receiver's one-workgroup kernel waits for it: no RCCL kernel, no staging copy on the per-substep path.
        // One allocation per rank: [from-left parity 0 | from-left parity 1 | from-right 0 | from-right 1 | flags].
        bool direct = false;
        void* direct_base = nullptr;            // this rank's allocation (fine-grained device memory)
        void* peer_base[2] = {nullptr, nullptr};   // the left / right neighbour's, as mapped here
        bool peer_mapped[2] = {false, false};      // ... through hipIpcOpenMemHandle (else: this rank itself)
        float direct_timeout_s = 5.f;
        bool direct_mute = false;   // MPM_HALO_DEBUG_MUTE (tests): the signal kernel is left out
        uint32_t* direct_cnt = nullptr;   // [2] entry counters of the two zones a substep packs, in THIS device's memory
    } chain;
    // TEAM transport of the distributed contact solve (mpm_team.h, mpm_team_prepare / _connect): this rank's region, every
    // rank's region as mapped here, the device-side exchange counters
    struct Team {
        bool on = false;
        int rank = 0, world = 1;
        void* base = nullptr;                 // this rank's region (fine-grained device memory)
        void* peer[TEAM_MAX] = {};            // every rank's, as this rank addresses it (peer[rank] == base)
        bool mapped[TEAM_MAX] = {};           // ... through hipIpcOpenMemHandle (else: a pointer of this process)
        size_t zone_cap = 0, zone_bytes = 0;
        TeamState* ts = nullptr;
        float timeout_s = 5.f;
    } team;
    bool halo_mid_done = false;   // mpm_substep_mid_halo ran in this substep
    int halo_nz = 0, halo_zlo[2] = {0, 0}, halo_zhi[2] = {0, 0};
    unsigned g_rb = 2048;  // workgroups of the particle-parallel re-sort kernels
    int grid_state = 0;  // 0 nothing, 1 slabs valid (after P2G), 2 grid updated
    uint64_t substeps = 0;
    // analytic colliders of the grid update selected by mpm_bc = MPM_BC_TABLE (mpm_set_grid_colliders)
    GridColliders grid_colliders{};
    uint64_t grid_colliders_version = 0;   // (counts the changes of both tables: substeps are owed with the tables of their call)
    // rigid bodies of the grid update selected by mpm_bc = MPM_BC_BODIES (mpm_set_grid_bodies; k_grid_bodies)
    std::vector<mpm_grid_body_t> grid_bodies;   // the caller's table, as given
    GridBodyTable* d_grid_bodies = nullptr;     // ... as the kernel reads it
    int grid_bodies_kinds = 0;                  // the instance it needs (bit 0: an ellipsoid, bit 1: a mesh body)
    // external force fields (mpm_set_force_fields; mpm_fields.h): a non-empty table selects k_p2g's FIELDS instances
    std::vector<mpm_force_field_t> force_fields;   // the caller's table, as given
    ForceFieldTable* d_force_fields = nullptr;     // ... as the kernel reads it
    double force_fields_gamma = 0.0;               // sum of gamma over the linear drags: dt * this <= 1 (fields_stable)
    // bending stiffness (mpm_set_bending; mpm_bending.h): a cloth with k > 0 switches k_bend on behind k_vforce
    struct Bending {
        std::vector<float> k;            // [cloth] as given; empty or all zero: off
        BendArgs args{};                 // the table as k_bend reads it (device memory, in `allocs`)
        float max_dt = INFINITY;         // 2 / sqrt(max_i (1 / m_i) sum_j |k Q_ij|) (fields_stable)
        std::vector<int> row_vertex;     // [row] its vertex (original, 0-based), and
        std::vector<double> abs_sum;     // sum_j |k Q_ij| of the row, the diagonal included (mpm_damping_max_stable_dt)
        bool on() const { return args.n_rows > 0; }
    } bend;
    // stiffness-proportional damping (mpm_set_damping; mpm_damping.h): k_damp behind k_fem for the cloths with
    // beta_membrane > 0, k_bend_damp behind k_bend for those with beta_bending > 0 and bending stiffness k > 0
    struct Damping {
        std::vector<mpm_cloth_damping_t> d;   // [cloth] as given; empty or all zero: off
        DampArgs args{};                      // k_damp's tables (device memory, in `allocs`); coef == nullptr: no membrane damping
        float* d_beta_vertex = nullptr;       // [vertex] its cloth's beta_bending, for k_bend_damp; null: none is > 0
        std::vector<float> beta_vertex;       // ... on the host
        std::vector<double> D_membrane, mass; // [vertex] Gershgorin row sum of the membrane's damping matrix at the rest shape; mass
        bool bend_rows = false;               // the bending table in force has a row with beta_bending > 0 (damping_limit)
        float max_dt = INFINITY;              // 2 / max_i (D_i / m_i) (damping_limit, fields_stable)
        bool membrane() const { return args.coef != nullptr; }
        bool bending() const { return d_beta_vertex != nullptr && bend_rows; }
        bool any() const {                    // some coefficient > 0: the feature is on
            for (const mpm_cloth_damping_t& c : d)
                if (c.membrane > 0.f || c.bending > 0.f) return true;
            return false;
        }
    } damp;
    // woven cloth (mpm_set_weave; mpm_weave.h): k_weave behind k_fem and before k_damp for the cloths with a weave
    struct Weave {
        std::vector<mpm_cloth_weave_t> w;     // [cloth] as given; empty or all zero: off
        std::vector<float> axis;              // [face][2] (c, s) by original face id, on the host (mpm_weave_axes)
        WeaveArgs args{};                     // k_weave's tables (device memory, in `allocs`); coef == nullptr: off
        const int2* d_ranges = nullptr;       // [cloth] (first face, end face) for k_weave_energy
        float max_dt = INFINITY;              // 2 / sqrt(max_i (K_i / m_i)) (fields_stable)
        bool on() const { return args.coef != nullptr; }
    } weave;
    // tearing cloth (mpm_set_tearing, mpm_set_torn_faces; mpm_tear.h): k_tear last in the face chain while the tables exist
    struct Tear {
        std::vector<mpm_cloth_tear_t> t;      // [cloth] as given; empty or all zero: no cloth has a limit
        TearArgs args{};                      // k_tear's tables (device memory, in `allocs`); torn == nullptr: off
        const int2* d_ranges = nullptr;       // [cloth] (first face, end face) for k_tear_count
        uint32_t* d_count = nullptr;          // [cloth] k_tear_count's output
        bool on() const { return args.torn != nullptr; }
        bool limit(size_t c) const { return c < t.size() && t[c].stretch_limit > 0.f; }
    } tear;
    // tearing composed with shell bending and gas (mpm_set_tear_coupling): MPM_TEAR_CUTS_HINGES | MPM_TEAR_VENTS_GAS.  No
    // state but this mask: cut hinges and vented cloths are functions of tear.args.torn, evaluated in the substep
    uint32_t tear_coupling = 0u;
    // links between cloth vertices (mpm_set_links; mpm_links.h): a non-empty table switches k_link on behind k_vforce
    struct Links {
        std::vector<mpm_link_t> set;     // the caller's table, as given
        LinkArgs args{};                 // ... as k_link reads it (device memory, in `allocs`)
        const float4* d_pair = nullptr;  // [link] k_link_energy's records
        float max_dt = INFINITY;         // the positive root of W dt^2 + 2 G dt = 4 (fields_stable)
        // breakable links (mpm_set_link_limits, mpm_set_broken_links): the tables exist while some link has a limit or some
        // flag is set, and k_link_break then runs in front of k_link; they go with the table they belonged to
        std::vector<float> limits;       // [link] break_length as given; empty: all off
        LinkBreakArgs brk{};             // k_link_break's tables (device memory, in `allocs`); B2 == nullptr: none
        const int2* d_range = nullptr;   // the single range (0, n) for k_tear_count
        uint32_t* d_count = nullptr;     // ... and its output
        bool on() const { return args.n_rows > 0; }
        bool breaking() const { return brk.B2 != nullptr; }
    } links;
    // enclosed-volume pressure per cloth (mpm_set_pressure; mpm_pressure.h): a table with a pressurised cloth switches
    // k_pressure on behind k_link, and a cloth in gas mode k_pressure_volume and k_pressure_gauge in front of it.  The
    // chunk arrays hold the gas cloths' chunks, then all cloths' (mpm_pressure_state); made at first use (`built`).
    struct Pressure {
        std::vector<mpm_cloth_pressure_t> set;   // the caller's table, as given (empty: off)
        PressureArgs args{};                     // ... as k_pressure reads it (device memory, in `allocs`)
        PressureVolumeArgs vol{};                // chunks, partial sums, parameters and state; ranges: all cloths'
        const int4* d_ranges_gas = nullptr;      // [cloth] its chunks in the gas cloths' list
        int n_gas_chunks = 0, n_all_chunks = 0;
        bool built = false;
        bool on() const { return args.n_rows > 0; }
        bool gas() const { return n_gas_chunks > 0; }
    } pressure;
    // shell bending about a curved rest shape (mpm_set_shell_bending; mpm_shell.h): a cloth with k > 0 and a hinge switches
    // k_hinge and k_hinge_gather on behind k_pressure
    struct Shell {
        std::vector<mpm_cloth_shell_t> set;   // the caller's table, as given (empty: off)
        HingeArgs hinge{};                    // the hinge table as k_hinge reads it (device memory, in `allocs`)
        ShellArgs args{};                     // the gather table as k_hinge_gather reads it
        std::vector<int32_t> ids4;            // [4 hinge] vertex ids, and
        std::vector<float> kc, psibar;        // [hinge] float(k cbar), the psi of the rest shape (mpm_shell_hinges)
        std::vector<int> hinge_cloth;         // [hinge]
        float max_dt = INFINITY;              // the guard at the rest shape (fields_stable)
        // creases (mpm_set_creases, mpm_set_crease_state): the tables exist while some cloth has a yield angle or some
        // hinge's psibar in force (hinge.par[h].y) differs from `psibar`, and k_crease then runs in front of k_hinge; they
        // go with the hinge table they belonged to
        std::vector<mpm_cloth_crease_t> crease;   // [cloth] as given; empty: all off
        CreaseArgs cr{};                      // k_crease's tables (device memory, in `allocs`); cr == nullptr: none
        // hinge damping (mpm_set_shell_damping; mpm_shell.h HINGE DAMPING): the tables exist while some cloth has beta > 0,
        // and k_hinge<1> then runs in k_hinge<0>'s place; they go with the hinge table they belonged to
        std::vector<mpm_cloth_shell_damping_t> damping;   // [cloth] as given; empty: off
        const float* d_bkc = nullptr;         // [hinge] float(beta k cbar) (device memory, in `allocs`); nullptr: off
        std::vector<double> cbar;             // [hinge] 3 |ebar|^2 / (Abar_A + Abar_B), as kc was formed from it
        std::vector<double> row_rate;         // [row] the guard's row sum over the row's mass (inf where the mass is not positive)
        std::vector<int> row_cloth;           // [row] its cloth
        float max_dt_elastic = INFINITY;      // max_dt of the table without a damper, to the bit
        bool on() const { return hinge.n > 0; }
        bool creasing() const { return cr.cr != nullptr; }
        bool damped() const { return d_bkc != nullptr; }
    } shell;
    // anchors: springs and cords from cloth vertices to rigid bodies (mpm_set_anchors; mpm_anchors.h): a non-empty table
    // switches k_anchor_pose and k_anchor on behind k_hinge_gather, and k_pin's clock tail behind GridToParticle
    struct Anchors {
        std::vector<mpm_anchor_t> set;       // the caller's table, as given
        AnchorArgs args{};                   // ... as k_anchor reads it (device memory, in `allocs`)
        const AnchorRec* d_one = nullptr;    // [anchor] k_anchor_energy's records
        AnchorPose* d_pose = nullptr;        // [cap_pose] k_anchor_pose's table
        size_t cap_pose = 0;
        bool unresolved = false;             // some record's body had no motion slot when the table was laid out (anchors_ready)
        float max_dt = INFINITY;             // link_limit of the guard's rates (fields_stable)
        bool on() const { return args.n_rows > 0; }
    } anchors;
    // the per-cloth report (mpm_measure, mpm_face_strain; mpm_measure.h): chunk table and scratch, made at first use
    struct Measure {
        bool built = false;
        std::vector<int4> chunks;        // the host's copy of d_chunks (face chunks, then vertex chunks)
        std::vector<float> k_seen;       // Bending::k the vertex chunks' rows of the bending table were worked out for
        bool rows_stale = true;          // ... not yet
        int n_face_chunks = 0, n_vertex_chunks = 0;
        int4* d_chunks = nullptr;
        int4* d_ranges = nullptr;        // [cloth] its chunks (k_measure_final)
        mpm_cloth_measure_t* d_rows = nullptr;   // [chunk] partial sums
        mpm_cloth_measure_t* d_out = nullptr;    // [cloth]
    } measure;
    // fixed constraints (mpm_set_pins, mpm_set_body_motions; k_pin in mpm_pins.h)
    struct PinState {
        std::vector<mpm_pin_t> set;              // the caller's pins, in order
        std::vector<uint32_t> motion_body;       // body of every motion slot (slots are never given back)
        PinDev* d_pins = nullptr;
        size_t cap_pins = 0;
        BodyMotionDev* d_mot = nullptr;          // [slot] pose, velocity and clock
        size_t cap_mot = 0;
        unsigned* d_ticket = nullptr;
        bool table_dirty = false;                // d_pins is not `set` yet (resolved at the next substep entry point)
    } pin;
    // Most faces around one vertex of any cloth of the engine (Finalize, from the adjacency CSR it builds; a partitioned
    // engine keeps the whole scene's on every rank).  Above 8, k_vforce stays (see fused_forces); at most 6, the kernels
    // that sum a vertex's entries of DP::VF read six planes instead of eight (vf_planes_of, launch_p2g,
    // launch_fem_vertices).  Invariant behind that: the planes at or above this number hold +0 after every re-sort and
    // are never written by k_fem or k_damp (mpm_device.h at VF_PLANES_REGULAR).
    int max_valence = 0;
    // launch geometry
    unsigned g_np = 0, g_nf = 0, g_nv = 0, g_tile = 0, g_grid = 0;
    // contacts / rigid bodies
    ContactBuffers cb{};
    mpm_contact_stats_t last_contact{};   // of the last mpm_update_contact
    bool last_contact_on_device = false;  // ... of which only what the mailbox carries has reached the host (contact_stats_from_device)
    bool last_contact_gated = false;      // ... skipped itself with its whole substep (CT_DONE_GATED)
    float ct_quiet_left = 0.f;            // Ctl::quiet_time left as of the last solve's publication
    bool last_contact_reused = false;     // ... ran on the previous solve's sorted order and node list (settled scene)
    // MPM_CT_NO_REUSE=1: every solve runs the full set-up (sort, per-cell runs, node list), also when the pair list repeats
    bool ct_no_reuse = getenv("MPM_CT_NO_REUSE") != nullptr;
    // MPM_CT_INITIAL_CAPACITY: contacts the buffers of device-made pairs hold at first (tests: a small value makes the
    // overflow-and-repeat path run; default: a sixteenth of the particles, at least 4096)
    size_t ct_initial_capacity = getenv("MPM_CT_INITIAL_CAPACITY") ? (size_t)std::max(1, atoi(getenv("MPM_CT_INITIAL_CAPACITY"))) : 0;
    // MPM_CT_GATE_ALWAYS=1 (tests): mpm_run_coupled_substeps never sends the re-sort launches ahead of a substep on its own
    // estimate: every re-sort is found by a substep skipping itself
    bool ct_gate_always = getenv("MPM_CT_GATE_ALWAYS") != nullptr;
    double ct_wait_us = 0;   // (MPM_CT_DEBUG) host time spent polling the mailbox
    uint64_t ct_counters[6] = {0, 0, 0, 0, 0, 0};   // solves, of them on a reused set-up, refused as stale, repeated after an overflow,
                                                     // coupled substeps that ran contact-free on a watch, of them skipped and repeated
    unsigned watch_seq = 0;                          // number of the last k_ct_watch launch (Ctl::watch_hit)
    bool ct_no_watch = getenv("MPM_CT_NO_WATCH") != nullptr;   // every coupled substep generates pairs and solves (A/B, tests)
    SolveParams last_contact_prm;   // its parameters
    // slot space of a partitioned rank = headroom x what it holds (mpm_dist_set_headroom, MPM_DIST_HEADROOM; 0 = the whole
    // scene's size, no shrink); grown at the migration that would overflow it (dist_resize)
    float dist_headroom = getenv("MPM_DIST_HEADROOM") ? std::max(0.f, (float)atof(getenv("MPM_DIST_HEADROOM"))) : 1.5f;
    // bands from the mesh: the drift (cells along x) between two migrations that the ghost bands are sized for, if the
    // zone allows that much (MPM_DIST_DRIFT).  Wider bands: fewer migrations, more ghost particles to advance.
    float dist_drift_target = getenv("MPM_DIST_DRIFT") ? std::max(.06f, (float)atof(getenv("MPM_DIST_DRIFT"))) : .5f;
    float dist_longest_edge = 0.f;        // cells, from the mesh handed to AddQRCloth
    // bands from the mesh are RE-TUNED at migrations (mpm_dist_retune): the drift budget follows the speed the ranks
    // measure, so that a migration is due every dist_target_interval substeps or so -- wide bands for a cloth that moves
    // along x, narrow ones (few ghosts) for one that does not.  MPM_DIST_RETUNE=0 keeps the bands of mpm_dist_init.
    bool dist_auto = false;               // the bands came from the mesh
    bool dist_retune = getenv("MPM_DIST_RETUNE") ? atoi(getenv("MPM_DIST_RETUNE")) != 0 : true;
    float dist_reach = 0.f, dist_hyst = 0.f, dist_delta_max = 0.f;   // cells: a face's reach, the hysteresis, the zone's limit
    float dist_target_interval = getenv("MPM_DIST_INTERVAL") ? std::max(2.f, (float)atof(getenv("MPM_DIST_INTERVAL"))) : 16.f;
    uint32_t dist_retunes = 0;
    // share of the ranks' common quiet-time estimate after which they migrate again (the estimate is ballistic, elastic
    // forces are not in it); MPM_MIG_SAFETY
    float mig_safety = getenv("MPM_MIG_SAFETY") ? std::min(1.f, std::max(.05f, (float)atof(getenv("MPM_MIG_SAFETY")))) : .5f;
    uint32_t dist_resizes = 0, dist_migrations = 0;
    // transport of the distributed contact solve when there is no native chain (mpm_dist_set_transport)
    mpm_exchange_fn dist_exchange = nullptr;
    mpm_allreduce_fn dist_allreduce = nullptr;
    void* dist_user = nullptr;
    size_t dist_zone_cap = 1024;
    std::string dump_dir = ".";
    // scratch for downloads
    void* d_stage = nullptr;
    size_t stage_bytes = 0;

    // Environment switches are read once per HANDLE, when the engine object is made (mpm_create): two engines of one
    // process can differ, and nothing is cached per process.
    // MPM_POISON=1 (tests): buffers that are not zero-initialised start as 0xFF bytes (NaN floats,
    // -1 ints), so that a read of something never written shows up on every box
    bool poison_fill = getenv("MPM_POISON") != nullptr;
    bool poison() const { return poison_fill; }
    // MPM_ANTICIPATE: horizon (substeps) of the re-sort's anticipatory binning (launch_rebuild)
    float anticipate_horizon = getenv("MPM_ANTICIPATE") ? (float)atof(getenv("MPM_ANTICIPATE")) : 32.f;
    // ... in cells, over that many substeps of the last known length (not in a partitioned domain, where ownership and
    // ghost bands are defined by the position itself)
    float anticipation() const { return dp.dist.on ? 0.f : anticipate_horizon * last_dt * dp.dxinv; }
    // MPM_CT_EAGER=1: the contact solve applies every accepted step with a kernel of its own (update_contact)
    bool ct_eager = getenv("MPM_CT_EAGER") != nullptr;
    // MPM_CT_RELAX: Jacobi relaxation of the contact solve instead of the reference's 0.3 (tests: overshoot on purpose)
    float ct_relax = getenv("MPM_CT_RELAX") ? (float)atof(getenv("MPM_CT_RELAX")) : 0.f;
    // MPM_CT_BATCH="first,next": Newton iterations enqueued per batch of the contact solve (measurements)
    int ct_batch[2] = {0, 0};
    bool ct_debug = getenv("MPM_CT_DEBUG") != nullptr;
    bool ct_force_dist = getenv("MPM_CT_FORCE_DIST") != nullptr;   // (tests, see update_contact)
    mpm_engine() {
        if (const char* t = getenv("MPM_CT_BATCH")) sscanf(t, "%d,%d", &ct_batch[0], &ct_batch[1]);
    }
    // tests (mpm_debug_fail_alloc): the n-th dalloc from now reports hipErrorOutOfMemory without asking the runtime
    int fail_alloc_countdown = 0;
    template <class T>
    int dalloc(T** out, size_t n, bool zero) {
        void* ptr = nullptr;
        const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
        if (fail_alloc_countdown > 0 && --fail_alloc_countdown == 0)
            return fail(MPM_ERR_NOMEM, "device allocation failed (injected by mpm_debug_fail_alloc)");
        HIP_TRY(hipMalloc(&ptr, bytes));
        allocs.push_back(ptr);
        alloc_bytes.push_back(bytes);
        if (zero) HIP_TRY(hipMemsetAsync(ptr, 0, bytes, stream));
        else if (poison()) HIP_TRY(hipMemsetAsync(ptr, 0xFF, bytes, stream));
        *out = static_cast<T*>(ptr);
        return 0;
    }
    // releases one dalloc'ed array (mpm_dist_init: the whole-scene sized arrays a partitioned rank gives back)
    template <class T>
    void dfree(T*& ptr) {
        if (!ptr) return;
        for (size_t k = 0; k < allocs.size(); ++k)
            if (allocs[k] == (void*)ptr) {
                (void)hipFree(allocs[k]);
                allocs.erase(allocs.begin() + (long)k);
                alloc_bytes.erase(alloc_bytes.begin() + (long)k);
                break;
            }
        ptr = nullptr;
    }
    size_t bytes_of(const void* ptr) const {
        for (size_t k = 0; k < allocs.size(); ++k)
            if (allocs[k] == ptr) return alloc_bytes[k];
        return 0;
    }
    int stage(size_t bytes) {
        if (bytes > stage_bytes) {
            if (d_stage) HIP_TRY(hipFree(d_stage));
            d_stage = nullptr;
            HIP_TRY(hipMalloc(&d_stage, bytes));
            if (poison()) HIP_TRY(hipMemsetAsync(d_stage, 0xFF, bytes, stream));
            stage_bytes = bytes;
        }
        return 0;
    }
};

// Blocking copies ORDERED ON THE ENGINE'S STREAM.  That stream is non-blocking: the legacy null
// stream behind plain hipMemcpy/hipMemset does not wait for it and is not waited for by it, so
// a plain hipMemcpy can overtake a queued hipMemsetAsync or kernel (seen as rare garbage in
// freshly finalised engines).  Nothing in the engine may use the synchronous calls.
#define H2D(e, dst, src, bytes)                                                                    \
    do {                                                                                           \
        HIP_TRY(hipMemcpyAsync((dst), (src), (bytes), hipMemcpyHostToDevice, (e)->stream));        \
        HIP_TRY(hipStreamSynchronize((e)->stream));                                                \
    } while (0)
#define D2H(e, dst, src, bytes)                                                                    \
    do {                                                                                           \
        HIP_TRY(hipMemcpyAsync((dst), (src), (bytes), hipMemcpyDeviceToHost, (e)->stream));        \
        HIP_TRY(hipStreamSynchronize((e)->stream));                                                \
    } while (0)

static int use(mpm_engine* e) {
    HIP_TRY(hipSetDevice(e->device));
    return 0;
}

// Fresh device arrays that replace something the engine holds: freed again unless the caller commits them ("all new
// arrays or none": mpm_set_bending, dist_resize).  Allocation itself is the engine's dalloc.
struct FreshArrays {
    mpm_engine* e;
    std::vector<void*> got;
    explicit FreshArrays(mpm_engine* e) : e(e) {}
    FreshArrays(const FreshArrays&) = delete;
    ~FreshArrays() { for (void* q : got) e->dfree(q); }
    template <class T>
    int alloc(T** out, size_t n, bool zero) {
        if (int rc = e->dalloc(out, n, zero)) return rc;
        got.push_back((void*)*out);
        return 0;
    }
    void commit() { got.clear(); }
};

// hipEvents of a measurement, destroyed however the function is left
struct Events {
    std::vector<hipEvent_t> ev;
    Events() = default;
    Events(const Events&) = delete;
    ~Events() { for (hipEvent_t x : ev) (void)hipEventDestroy(x); }
    int create(size_t n) {
        for (ev.reserve(n); ev.size() < n;) {
            hipEvent_t x;
            HIP_TRY(hipEventCreate(&x));
            ev.push_back(x);
        }
        return 0;
    }
    const hipEvent_t& operator[](size_t k) const { return ev[k]; }
};

// The getters of the caller's tables (pins, grid bodies, force fields, body contact materials): as many entries as fit,
// and the whole count (each getter checks its own arguments first)
template <class T>
static int copy_out(const std::vector<T>& set, T* out, size_t capacity, size_t* n_out) {
    std::copy(set.begin(), set.begin() + (long)std::min(capacity, set.size()), out);
    if (n_out) *n_out = set.size();
    return 0;
}

// The getters of a table with one record per cloth (or, the link limits, per link): `n` entries, `zero` where nothing was
// set
template <class T>
static int padded_out(std::vector<T> set, size_t n, const T& zero, T* out, size_t capacity, size_t* n_out) {
    REQUIRE(out || capacity == 0, "null output");
    set.resize(n, zero);
    return copy_out(set, out, capacity, n_out);
}

// ---- what the features' host headers need from mpm_engine.hip -------------------------------------------------------------
// (mpm_cloth_host.h, mpm_bodies_host.h, mpm_dist_host.h, mpm_chain_host.h: included by mpm_engine.hip, which defines these)
// the owed substeps and the held-back phase calls, run before a call looks at or changes the state
static int settle(mpm_engine* e, Ctl* fresh = nullptr);
// the conditional re-sort
static void launch_rebuild(mpm_engine* e, DP p, bool lean = false, float dt = 0.f);
static int recover_slab_overflow(mpm_engine* e, Ctl& c);
// the fixed-point scales of ParticleToGrid's tiles, from the total mass: again after every change of the masses
static int set_fixed_point_scales(mpm_engine* e);

#define READY_NO_SETTLE(e)                              \
    REQUIRE(e, "null handle");                          \
    REQUIRE((e)->finalized, "call mpm_finalize first"); \
    if (int rc__ = use(e)) return rc__
#define READY(e)         \
    READY_NO_SETTLE(e);  \
    if (int rc2__ = settle(e)) return rc2__

// ---- argument checks shared by pins, grid bodies and force fields ----------------------------------------------------------
static bool finite_n(const float* a, int n) {
    for (int k = 0; k < n; ++k)
        if (!std::isfinite(a[k])) return false;
    return true;
}
// R^T R = I and det R = 1, each entry within 1e-4 (float rotations that went through a few products)
static bool is_rotation(const float* R) {
    if (!finite_n(R, 9)) return false;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double d = 0.0;
            for (int k = 0; k < 3; ++k) d += (double)R[k * 3 + i] * (double)R[k * 3 + j];
            if (std::fabs(d - (i == j ? 1.0 : 0.0)) > 1e-4) return false;
        }
    const double det = (double)R[0] * ((double)R[4] * R[8] - (double)R[5] * R[7]) -
                       (double)R[1] * ((double)R[3] * R[8] - (double)R[5] * R[6]) +
                       (double)R[2] * ((double)R[3] * R[7] - (double)R[4] * R[6]);
    return std::fabs(det - 1.0) <= 1e-4;
}
// Which features are in force, for the lists of mpm_features.h.  The ONLY place outside a feature's own host code and the
// launch helpers that decides whether a feature is in force: one line per feature.
static FeatureState feature_state(const mpm_engine* e) {
    FeatureState s;
    s.on[F_PINS] = !e->pin.set.empty();
    s.on[F_MATERIALS] = e->multi_mat;
    s.on[F_GRID_BODIES] = !e->grid_bodies.empty();
    s.on[F_FORCE_FIELDS] = !e->force_fields.empty();
    s.on[F_BENDING] = e->bend.on(), s.max_dt[F_BENDING] = e->bend.max_dt;
    s.on[F_DAMPING] = e->damp.any(), s.max_dt[F_DAMPING] = e->damp.max_dt;
    s.on[F_WEAVE] = e->weave.on(), s.max_dt[F_WEAVE] = e->weave.max_dt;
    s.on[F_TEARING] = e->tear.on();
    s.on[F_LINKS] = e->links.on(), s.max_dt[F_LINKS] = e->links.max_dt;
    s.on[F_PRESSURE] = e->pressure.on();
    s.on[F_SHELL] = e->shell.on(), s.max_dt[F_SHELL] = e->shell.max_dt;
    s.on[F_ANCHORS] = e->anchors.on(), s.max_dt[F_ANCHORS] = e->anchors.max_dt;
    s.on[F_REST_SHAPE] = e->rest_set;
    return s;
}
// every feature of mpm_features.h is refused on a partitioned or multi-rank engine (out of scope);
// what_is: the feature's FeatureRow::what_is ("pins are", "bending stiffness is", ...), or a call's own ("mpm_tear_measure is")
static int single_engine_only(const mpm_engine* e, const char* what_is) {
    if (e->dp.dist.on || e->chain.comm || e->chain.direct || e->team.on)
        return fail(MPM_ERR_INVALID, std::string(what_is) + " not available on a partitioned or multi-rank engine");
    return 0;
}

