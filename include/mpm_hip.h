/*
 * mpm_hip.h -- C ABI of the MI355X-native cloth-MPM substep engine.
 *
 * This is the drop-in boundary for the hot path of g1n0st/drake's
 * multibody/gpu_mpm layer: every entry point below replaces one method of the
 * reference's GpuMpmState<float> / GpuMpmSolver<float> pair (the only scalar
 * type the reference instantiates, cuda_mpm_model.cu:347, cuda_mpm_solver.cu:623).
 * Citations are file:line under the reference tree.
 *
 * Conventions
 *   - plain pointers and sizes only; host buffers are caller-owned
 *   - every call returns 0 on success or a negative mpm_status; the message
 *     for the calling thread's last failure is mpm_last_error().  No call throws and no call
 *     terminates the process: every entry point ends in a catch-all that turns a C++ exception
 *     raised below it into MPM_ERR_NOMEM / MPM_ERR_INTERNAL (the reference's contract --
 *     settings.h:11-25: errors never kill the caller outside DEBUG builds)
 *   - one handle <-> one HIP device; calls on one handle must be serialised
 *     by the caller (the reference is single-threaded per state as well)
 *   - "slot order" is the reference's current particle order: [faces | verts]
 *     after mpm_finalize (cuda_mpm_model.cu:40-45), permuted by every
 *     mpm_rebuild_mapping(h, 1) exactly like RebuildMapping(state, true)
 *     (stable sort on the low min(3*domain_bits,16) key bits,
 *     cuda_mpm_solver.cu:47-68).  The engine's internal memory order is
 *     different (block/cell sorted 16-byte records) and never visible through this API.
 *   - vectors cross the boundary as packed float triples / row-major 3x3,
 *     exactly like the reference's Vec3<float>/Mat3<float> device buffers.
 */
#ifndef MPM_HIP_H_
#define MPM_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define MPM_API __attribute__((visibility("default")))
#else
#define MPM_API
#endif

typedef struct mpm_engine *mpm_handle_t;

typedef enum {
    MPM_OK = 0,
    MPM_ERR_INVALID = -1,     /* bad argument / call order                     */
    MPM_ERR_HIP = -2,         /* a HIP runtime call failed                     */
    MPM_ERR_DRIFT = -3,       /* a face particle was re-centred out of its block's tile (diverging state) */
    MPM_ERR_CAPACITY = -4,    /* internal table overflow                       */
    MPM_ERR_NO_DEVICE = -5,   /* no usable GPU: there is no CPU fallback       */
    MPM_ERR_DOMAIN = -6,      /* a particle left the grid (the reference: undefined behaviour) */
    MPM_ERR_RANGE = -7,       /* a ParticleToGrid node sum was not finite / out of the accumulators' range */
    MPM_ERR_HALO = -8,        /* partitioned domain: a particle left the zone shared with the neighbour rank */
    MPM_ERR_NOMEM = -9,       /* host or device memory exhausted (std::bad_alloc / hipErrorOutOfMemory)        */
    MPM_ERR_INTERNAL = -10    /* a C++ exception reached the C boundary and was caught there: a bug in the engine,
                                 reported instead of terminating the calling process                         */
} mpm_status;

/* Runtime form of the compile-time constants in settings.h:36-127. */
typedef struct {
    float youngs_modulus; /* settings.h:73  (4e5)                              */
    float poisson_ratio;  /* settings.h:77  (0.3)                              */
    float density;        /* settings.h:81  (2000)                             */
    float gamma;          /* settings.h:85  (0) shear/friction of the cloth    */
    float K;              /* settings.h:92  (1e5) normal penalty stiffness     */
    float V;              /* settings.h:99  (0.8) RPIC damping blend           */
    float c_F;            /* settings.h:103 (0)                                */
    float sdf_friction;   /* settings.h:110 (0.3)                              */
    float gravity;        /* settings.h:121 (-9.8)                             */
    float epsv;           /* settings.h:125 (1e-3) friction regularisation     */
    int32_t gravity_axis; /* settings.h:118 (2)                                */
    int32_t wall_cells;   /* settings.h:56  (3) G_BOUNDARY_CONDITION           */
} mpm_material_t;

/* Arrays that mpm_download_array can return (parity tests, visualisation,
 * checkpoints).  Particle arrays come back in slot order, packed like the
 * reference's device buffers; grid arrays are dense and indexed by the
 * reference's cell key (cuda_mpm_kernels.cuh:334-341). */
typedef enum {
    MPM_ARR_POSITIONS = 0,       /* float[3*np]   current_positions()          */
    MPM_ARR_VELOCITIES = 1,      /* float[3*np]   current_velocities()         */
    MPM_ARR_VOLUMES = 2,         /* float[np]     current_volumes()            */
    MPM_ARR_AFFINE = 3,          /* float[9*np]   current_affine_matrices()    */
    MPM_ARR_PIDS = 4,            /* int32[np]     current_pids()               */
    MPM_ARR_INDEX_MAPPINGS = 5,  /* int32[np]     index_mappings()             */
    MPM_ARR_SORT_KEYS = 6,       /* uint32[np]    current_sort_keys() evaluated on the
                                    current positions (what RebuildMapping computes)  */
    MPM_ARR_FORCES = 7,          /* float[3*np]   forces()                     */
    MPM_ARR_TAUS = 8,            /* float[9*np]   taus()                       */
    MPM_ARR_DEFORMATION_GRADIENTS = 9, /* float[9*nf] original face order      */
    MPM_ARR_DM_INVERSES = 10,    /* float[4*nf]   original face order          */
    MPM_ARR_INDICES = 11,        /* int32[3*nf]   indices() (offset by +nf)    */
    MPM_ARR_GRID_MASSES = 12,    /* float[cells]  grid_masses()                */
    MPM_ARR_GRID_MOMENTUM = 13,  /* float[3*cells] grid_momentum(): momentum after
                                    ParticleToGrid, velocity after UpdateGrid   */
    MPM_ARR_GRID_V_STAR = 14,    /* float[3*cells] grid_v_star()               */
    MPM_ARR_GRID_TOUCHED_FLAGS = 15, /* uint32[blocks] grid_touched_flags()    */
    MPM_ARR_GRID_TOUCHED_IDS = 16,   /* uint32[cnt] ascending block ids        */
    MPM_ARR_CONTACT_VEL = 17,    /* float[3*nk]   contact_vel()                */
    MPM_ARR_CONTACT_VEL0 = 18,   /* float[3*nk]   contact_vel0()               */
    MPM_ARR_GRID_DIR = 19,       /* float[3*cells] grid_Dir()                  */
    MPM_ARR_MASSES = 20          /* float[np]     the mass ParticleToGrid uses for each particle: vol * density
                                    rounded to float as ParticleToGrid rounds it (per-cloth density: see
                                    mpm_add_qr_cloth_with_material) */
} mpm_array_id;

/* Timed phases reported by mpm_profile_substeps. */
enum {
    MPM_PHASE_REBUILD = 0,
    MPM_PHASE_FEM = 1,     /* per-face kernel of CalcFemStateAndForce */
    MPM_PHASE_VFORCE = 2,  /* its per-vertex force gather, whenever that is a launch of its own (see mpm_profile_substeps) */
    MPM_PHASE_P2G = 3,
    MPM_PHASE_GRID = 4,
    MPM_PHASE_G2P = 5,
    MPM_PHASE_COUNT = 6
};

typedef struct {
    uint64_t substeps;        /* substeps executed so far                      */
    uint64_t rebuilds;        /* internal block/cell re-sorts performed        */
    uint32_t home_blocks;     /* 4^3 blocks that currently own particles       */
    uint32_t active_blocks;   /* blocks whose nodes are updated each substep   */
    uint32_t touched_blocks;  /* reference-exact touched count of last P2G     */
    uint32_t error_flags;     /* sticky device error bits (0 = none)           */
    uint32_t active_faces;    /* particles this engine works on: all of them, or (partitioned   */
    uint32_t active_vertices; /* domain) the ones it owns plus its ghost copies                 */
    uint32_t face_slots;      /* particle slots allocated: the scene's counts, or -- after mpm_dist_init, which   */
    uint32_t vertex_slots;    /* shrinks the rank to its share -- 1.5 x what the rank held then, plus head room     */
    uint64_t particle_bytes;  /* device bytes of all arrays indexed by particle slot                              */
    uint64_t scene_index_bytes; /* device bytes indexed by ORIGINAL particle id (id -> slot map, slot-order
                                   bookkeeping, topology tables of Finalize): whole-scene sized on every rank;
                                   a partitioned engine keeps only the maps, 13 bytes per particle of the scene */
    uint64_t resort_checks;   /* times the kernels of the conditional re-sort were launched, Finalize's first sort
                                 included (mpm_run_substeps and complete phase-by-phase substeps leave them out while
                                 the quiet time below lasts, then send them with every 4th substep)                   */
    float quiet_time_s;       /* the last re-sort's estimate of how long no particle can leave its block's tile when
                                 all of them move ballistically (velocity + gravity); 0 = not estimated                */
    float since_resort_s;     /* simulated time since that re-sort                                                     */
} mpm_stats_t;

MPM_API const char *mpm_last_error(void);
MPM_API int mpm_default_material(mpm_material_t *out);

/* ---- GpuMpmState<float> -------------------------------------------------- */

/* `GpuMpmState() = default` + the grid constants of settings.h:48-59 made
 * runtime: the grid is (2^domain_bits)^3 cells of size 2^-domain_bits.
 * `device` is the HIP device ordinal.  `material` may be NULL (defaults). */
MPM_API int mpm_create(int domain_bits, const mpm_material_t *material, int device, mpm_handle_t *out);

/* GpuMpmState::AddQRCloth (cuda_mpm_model.cu:16-33).  pos/vel: float[3*n_verts];
 * indices: int32[3*n_faces] local to this cloth.  May be called repeatedly. */
MPM_API int mpm_add_qr_cloth(mpm_handle_t h, const float *pos, const float *vel, size_t n_verts,
                             const int32_t *indices, size_t n_faces);

/* GpuMpmState::Finalize (cuda_mpm_model.cu:36-122): allocates every device
 * buffer, uploads the particles and runs the FEM initialisation kernel. */
MPM_API int mpm_finalize(mpm_handle_t h);

/* GpuMpmState::Destroy (cuda_mpm_model.cu:124-242); also frees the handle. */
MPM_API int mpm_destroy(mpm_handle_t h);

/* n_verts() / n_faces() / n_particles() (cuda_mpm_model.cuh:43-45). */
MPM_API int mpm_counts(mpm_handle_t h, size_t *n_verts, size_t *n_faces, size_t *n_particles);

/* grid_touched_cnt_host() (cuda_mpm_model.cuh:95-100); synchronises. */
MPM_API int mpm_grid_touched_cnt(mpm_handle_t h, uint32_t *out);

/* GpuMpmState::DumpCpuState (cuda_mpm_model.cu:244-265): vertex positions in
 * original vertex order (float[3*n_verts]) and triangle indices local to the
 * vertex array (int32[3*n_faces]).  Either pointer may be NULL. */
MPM_API int mpm_dump_cpu_state(mpm_handle_t h, float *pos_out, int32_t *indices_out);

/* ReallocateContacts is implicit in mpm_copy_contact_pairs. */

/* GpuMpmState::ReallocateExternelBodies (cuda_mpm_model.cu:319-338): sizes and
 * zeroes the per-body impulse accumulators. */
MPM_API int mpm_reallocate_external_bodies(mpm_handle_t h, size_t n_bodies);

/* GpuMpmState::ExternelBodyForceToHost (cuda_mpm_model.cu:340-345):
 * tau_out / f_out: float[3*n_bodies] accumulated impulses (F_Bq_W_tau, F_Bq_W_f). */
MPM_API int mpm_external_body_force_to_host(mpm_handle_t h, float *tau_out, float *f_out);

/* ---- rigid feedback wire format (consumers of the accumulators above) ----- */

/* DeformableDriver::FinalizeExternalContactForces (multibody/plant/deformable_driver.h:210-219):
 * ExternelBodyForceToHost, then impulse / dt -> force for every body.  `dt` is the PLANT step
 * (the accumulators collect the impulses of all its substeps).  tau_out / f_out: float[3*n_bodies],
 * torque about the body origin p_WB handed in with the contact pairs, and force, in the world frame. */
MPM_API int mpm_finalize_external_contact_forces(mpm_handle_t h, float dt, float *tau_out, float *f_out);

/* SpatialForce::Shift (multibody/math/spatial_force.h:91-93, 151-155) for n forces:
 * tau_out[i] = tau[i] - offset[i] x f[i]; f is unchanged.  Host arithmetic, needs no GPU. */
MPM_API int mpm_spatial_force_shift(size_t n, const float *tau, const float *f, const float *offset, float *tau_out);

/* What MultibodyPlant::AddAppliedExternalSpatialForces does with external_forces_host()
 * (multibody/plant/multibody_plant.cc:2385-2407): p_BoBq_W = R_WB * p_BoBq_B,
 * F_BBo_W = SpatialForce(tau, f).Shift(-p_BoBq_W), i.e. tau_Bo = tau + p_BoBq_W x f.
 * R_WB: float[9*n] row major; the rest float[3*n].  Host arithmetic, needs no GPU. */
MPM_API int mpm_external_forces_at_body_origin(size_t n_bodies, const float *R_WB, const float *p_BoBq_B,
                                               const float *tau, const float *f, float *tau_Bo_out);

/* ---- GpuMpmSolver<float> ------------------------------------------------- */

/* GpuMpmSolver::RebuildMapping (cuda_mpm_solver.cu:17-70).  Must be called
 * once per substep before mpm_particle_to_grid, as every reference caller does
 * (deformable_driver.h:244, cuda_mpm_test.cc:66).  sort != 0 re-orders the
 * slot order like the reference's stable 16-bit radix sort. */
MPM_API int mpm_rebuild_mapping(mpm_handle_t h, int sort);

/* GpuMpmSolver::CalcFemStateAndForce (cuda_mpm_solver.cu:72-84). */
MPM_API int mpm_calc_fem_state_and_force(mpm_handle_t h, float dt);

/* GpuMpmSolver::ParticleToGrid (cuda_mpm_solver.cu:86-105). */
MPM_API int mpm_particle_to_grid(mpm_handle_t h, float dt);

/* GpuMpmSolver::UpdateGrid (cuda_mpm_solver.cu:107-151).  mpm_bc in {-1,0,1,2,3} are the
 * reference's scenes (update_grid_kernel<T, BC>, cuda_mpm_kernels.cuh:673-774); MPM_BC_TABLE
 * uses the colliders set with mpm_set_grid_colliders, MPM_BC_BODIES (below) the rigid bodies set with
 * mpm_set_grid_bodies.  The same values are accepted wherever an entry point takes mpm_bc. */
#define MPM_BC_TABLE 4
MPM_API int mpm_update_grid(mpm_handle_t h, int mpm_bc);

/* Runtime form of the analytic colliders that the reference hard-codes per scene in
 * update_grid_kernel (cuda_mpm_kernels.cuh:660-789).  For a node at x = (idx + 0.5) dx (:661-665)
 * the FIRST collider of the list with phi(x) < 0 decides (the reference's else/break chains):
 *   MPM_GC_FIXED             v <- v + (v_c - v)                                   (:778-781)
 *   MPM_GC_SLIP_APPROACHING  only if n.(v_c - v) > 0 (scene 0, :684-690), then
 *   MPM_GC_SLIP              v += mu (v_c - v) + (1 - mu) n (n.(v_c - v))          (:783-786)
 * with n = grad(phi) and mu = friction (SDF_FRICTION, settings.h:110; a negative value selects the
 * engine's material.sdf_friction).  Shapes: sphere (centre p, radius), half-space (inside where
 * n.(x - p) < 0, n a unit vector).  At most 16 colliders. */
enum { MPM_GC_SPHERE = 0, MPM_GC_HALF_SPACE = 1 };
enum { MPM_GC_FIXED = 0, MPM_GC_SLIP_APPROACHING = 1, MPM_GC_SLIP = 2 };
typedef struct mpm_grid_collider {
    int32_t shape;
    int32_t mode;
    float p[3];
    float n[3];
    float radius;
    float v[3];        /* collider velocity (0 in every reference scene) */
    float friction;
} mpm_grid_collider_t;
MPM_API int mpm_set_grid_colliders(mpm_handle_t h, size_t n, const mpm_grid_collider_t *colliders);
/* The table that reproduces scene mpm_bc in {-1,0,1,2,3} (what mpm_update_grid(h, mpm_bc) runs). */
MPM_API int mpm_grid_collider_preset(int mpm_bc, float sdf_friction, mpm_grid_collider_t *out, size_t capacity,
                                     size_t *n_out);

/* GpuMpmSolver::GridToParticle (cuda_mpm_solver.cu:153-161). */
MPM_API int mpm_grid_to_particle(mpm_handle_t h, float dt);

/* GpuMpmSolver::GpuSync (cuda_mpm_solver.cu:163-166); also surfaces the sticky
 * device error flags, checked in this order: MPM_ERR_DRIFT, MPM_ERR_DOMAIN,
 * MPM_ERR_HALO (partitioned domain), MPM_ERR_RANGE (a ParticleToGrid node sum
 * was not finite, or left the fixed-point range of a deterministic engine) and
 * MPM_ERR_CAPACITY (a table or the slab pool overflowed).  A failure of the
 * HIP runtime while it runs owed substeps or synchronises is MPM_ERR_HIP
 * (MPM_ERR_NOMEM, MPM_ERR_INTERNAL as for every call). */
MPM_API int mpm_sync(mpm_handle_t h);

/* GpuMpmSolver::GpuSync() as the reference declares and calls it -- no state argument, a
 * cudaDeviceSynchronize() (cuda_mpm_solver.cu:164-166, cuda_mpm_test.cc:73): every engine the calling
 * thread's current HIP device holds is brought up to date (substeps that mpm_run_substeps deferred are run),
 * then the whole device is synchronised.  Like the reference's call it reports nothing about the state of a
 * simulation: the sticky errors of an engine (MPM_ERR_DRIFT, _CAPACITY, ...) stay with that engine's own
 * mpm_sync / mpm_get_stats, only a failure of the HIP runtime is an error here.  The engine list is walked under
 * the lock mpm_create / mpm_destroy take; the handles' own rule applies besides: no other thread may be inside
 * another call on one of them. */
MPM_API int mpm_device_synchronize(void);

/* Active blocks whose x block coordinate lies in [bx_lo, bx_hi]: what mpm_halo_pack would pack for that zone right
 * now (the set changes with re-sorts only).  For sizing exchange buffers after mpm_dist_init / mpm_finalize: the
 * native chain sends a fixed capacity per substep (a RCCL send needs its size when it is enqueued), so that capacity
 * should be a small multiple of this count, agreed between the neighbours, not a guess. */
MPM_API int mpm_halo_zone_blocks(mpm_handle_t h, int bx_lo, int bx_hi, uint32_t *count_out);

/* Tests: the frame of a contact with unit normal u (rows of J: two tangents, then u) exactly as the contact
 * kernels build it -- the same inline function, compiled for the host (math_tools.cuh:599-638 with axis_index 2,
 * a clone of RotationMatrix::MakeFromOneUnitVector; pinned on the reference's test vectors of
 * math/test/rotation_matrix_test.cc:1215-1252 in tests/test_contact_frame.py).  No device is touched. */
MPM_API int mpm_contact_frame(const float u[3], float J[9]);

/* bench.py, the contact leg's roofline: the four kernels of one backtracking Newton iteration of the solve that
 * mpm_update_contact has just finished (contact gradients / Hessians per cell, direction per node, line-search
 * energies, decision), each launched `reps` times back to back and timed with HIP events on the engine's stream:
 * kernel_ms[4] = duration per launch of (k_ct_tile, k_ct_node_dir, k_ct_ls, k_ct_decide).  Grid velocities are
 * left alone; call it before the next mpm_update_contact. */
MPM_API int mpm_profile_contact_iteration(mpm_handle_t h, int reps, float kernel_ms[4]);

/* Blocking copies between caller-owned host memory and device memory, ordered on the engine's stream (a plain
 * hipMemcpy on the null stream is not ordered with it).  For transports that stage the engine's exchange buffers
 * through the host (mpm_dist_set_transport): they must not bring a second HIP runtime into the process. */
MPM_API int mpm_memcpy_d2h(mpm_handle_t h, void *dst_host, const void *src_device, size_t bytes);
MPM_API int mpm_memcpy_h2d(mpm_handle_t h, void *dst_device, const void *src_host, size_t bytes);

/* Tests: substeps that mpm_run_substeps has enqueued but that found a re-sort pending and are still owed
 * (run by the next call that synchronises).  Waits for the stream; does NOT run them. */
MPM_API int mpm_debug_owed_substeps(mpm_handle_t h, uint32_t *out);

/* Bitwise reproducibility from run to run (off by default; the environment variable
 * MPM_DETERMINISTIC=1 turns it on at mpm_create).  A substep never uses float atomics, but the
 * engine's re-sort orders the particles inside a cell by the arrival of integer atomics; with
 * this switch every re-sort additionally sorts each cell's particles by their previous slot
 * (one more kernel per substep, ~2 us when idle, ~15 us per re-sort at 1M particles), and
 * ParticleToGrid accumulates its node sums in 64-bit fixed point (integer sums: exact whatever the
 * order in which the waves arrive) instead of in double precision (~1 us per substep at 1M
 * particles; the double sums are exact too unless the contributions to one node span more than
 * 2^29 in magnitude, in which case their last bit, 2^-53 of the sum, depends on the order). */
MPM_API int mpm_set_deterministic(mpm_handle_t h, int on);

/* The arithmetic of CalcFemStateAndForce's 19 divisions and 10 square roots per face (the QR / polar / SVD steps of
 * cuda_mpm_kernels.cuh:72-181 through math_tools.cuh:456-597).
 *   on = 0 (default): correctly rounded, as the reference's expressions read.  One substep then agrees with a plain-C
 *     restatement of the reference at north_star's "float state within 1e-5 relative" wherever float arithmetic can
 *     deliver that (tests/test_fast_math_gpu.py; tests/helpers.py: NOISE_FLOOR, floor_decides).
 *   on = 1: the hardware's 1-ulp reciprocal / reciprocal square root followed by one Newton step (results within
 *     ~0.6 ulp): 2.4 us per substep less at 1M particles (k_fem 910 -> 630 vector instructions per face); the
 *     velocities of one substep then differ from the strict path's by about the float rounding noise of that substep
 *     (1.4 x the distance between a float and a double evaluation; 1.0 - 1.7e-5 of max|v| on the parity scenes).
 *     The reference itself is built with -use_fast_math (tools/skylark/cuda.bzl:66-80), i.e. with CUDA's
 *     approximate division and square root: this switch is the closer analogue of what the reference RUNS, the default
 *     of what its source SAYS.
 * Also MPM_FAST_MATH=1 in the environment at mpm_create.  May be changed between substeps. */
MPM_API int mpm_set_fast_math(mpm_handle_t h, int on);
MPM_API int mpm_get_fast_math(mpm_handle_t h, int *on_out);

/* GpuMpmSolver::SyncParticleStateToCpu (cuda_mpm_solver.cu:185-191):
 * pos_out: float[3*n_particles] in slot order (the reference fills
 * positions_host()). */
MPM_API int mpm_sync_particle_state_to_cpu(mpm_handle_t h, float *pos_out);

/* GpuMpmSolver::Dump (cuda_mpm_solver.cu:168-183): Wavefront OBJ. */
MPM_API int mpm_dump_obj(mpm_handle_t h, const char *filename);

/* GpuMpmSolver::CopyContactPairs (cuda_mpm_solver.cu:193-212) taking the
 * MpmParticleContactPairs SoA (cpu_mpm_model.h:73-114): particle slot index,
 * rigid body index, signed distance (<0), normal, contact position, rigid
 * point velocity, body origin p_WB. */
MPM_API int mpm_copy_contact_pairs(mpm_handle_t h, size_t n_contacts, const uint32_t *particle_in_contact_index,
                                   const uint32_t *non_mpm_id, const float *penetration_distance,
                                   const float *normal, const float *particle_in_contact_position,
                                   const float *rigid_v, const float *rigid_p_WB);

/* Device-side replacement of DeformableDriver::CalcMpmContactPairs (deformable_driver.h:120-194)
 * followed by CopyContactPairs, for rigid bodies with analytic signed distance fields: no particle
 * positions travel to the host.  For every particle slot s (ascending) and collider j (ascending)
 * with phi_j(x_s) < 0 one contact is produced with exactly the fields of MpmParticleContactPairs
 * (cpu_mpm_model.h:73-114; deformable_driver.h:181-187): particle_in_contact_index = s,
 * non_mpm_id = body, penetration_distance = phi, normal = -grad(phi)/|grad(phi)|,
 * position = x_s, rigid_v = v + w x (x_s - p_WB), rigid_p_WB = p_WB.
 *   kind 0 half-space: inside is z_B <= 0 (Drake's HalfSpace), plane through p_WB, normal = R_WB[:,2]
 *   kind 1 sphere:     radius dims[0], centre p_WB
 *   kind 2 box:        half extents dims[0..2] in the body frame
 *   kind 3 capsule:    radius dims[0], half length dims[1] along z_B
 *   kind 4 cylinder:   radius dims[0], half length dims[1] along z_B (Drake's Cylinder(radius, length): (radius, length/2));
 *                      Drake's conventions (distance_to_point_callback.cc:206-299, 401-489): inside, the nearest feature is
 *                      the barrel on a tie with a cap; a point on the axis takes the radial direction +x_B
 *   kind 5 ellipsoid:  semi-axes dims[0..2] along x_B, y_B, z_B (Drake's Ellipsoid(a, b, c): (a, b, c)); the exact signed
 *                      distance (the reference's GJK/EPA answer is good to ~1e-6), gradient normalize(N / a^2) at the
 *                      nearest point N
 * Kinds 4 and 5 need every dimension they use finite and > 0 (MPM_ERR_INVALID otherwise, before anything is enqueued).
 * The pairs are left in the engine as if mpm_copy_contact_pairs had been called;
 * mpm_download_contact_pairs returns them (any pointer may be NULL). */
enum {
    MPM_COLLIDER_HALF_SPACE = 0,
    MPM_COLLIDER_SPHERE = 1,
    MPM_COLLIDER_BOX = 2,
    MPM_COLLIDER_CAPSULE = 3,
    MPM_COLLIDER_CYLINDER = 4,
    MPM_COLLIDER_ELLIPSOID = 5
};
typedef struct mpm_collider {
    int32_t kind;
    uint32_t body;      /* index into the external-body accumulators */
    float p_WB[3];      /* body origin in the world */
    float R_WB[9];      /* rotation body -> world, row major */
    float dims[3];
    float v[3], w[3];   /* spatial velocity of the body frame, world */
} mpm_collider_t;
MPM_API int mpm_generate_contact_pairs(mpm_handle_t h, size_t n_colliders, const mpm_collider_t *colliders,
                                       size_t *n_contacts_out);
/* QueryObject::ComputeSignedDistanceToPoint (query_object.h) for ONE collider of any kind, on the device: the signed
 * distance phi and the unit world gradient of phi at n world points x_W (float[3n]), everywhere -- outside, inside and
 * on the surface -- computed by the distance function of mpm_generate_contact_pairs.  phi_out: float[n],
 * grad_W_out: float[3n]; caller-owned host arrays.  A synchronisation point. */
MPM_API int mpm_collider_signed_distance(mpm_handle_t h, const mpm_collider_t *c, size_t n, const float *x_W,
                                         float *phi_out, float *grad_W_out);

/* ---- Mesh colliders (an extension) ----
 * A rigid body made of triangles -- Drake's Mesh or Convex, whose ComputeSignedDistanceToPoint the reference's driver
 * never sees (query_object.h: those shapes are ignored) -- as a signed-distance lattice held by the engine.  A scene with
 * mesh colliders therefore makes contact pairs the reference would not make.
 *
 * mpm_sdf_shape_from_mesh builds the lattice of one mesh on the device and returns its shape id in *shape_out.  verts:
 * float[3 n_verts] in the body frame B (the caller bakes in X_BG and the Mesh's scale); tris: int32[3 n_tris] vertex
 * indices.  The lattice is axis-aligned in B with spacing `cell` and covers the mesh's bounding box plus pad_cells cells
 * on every side: lo = min - pad_cells cell, n_a = ceil((max_a - min_a) / cell) + 2 pad_cells + 1 nodes per axis, node
 * (i, j, k) at lo + (i, j, k) cell, values float, x fastest.  A node's value is the distance to the nearest triangle,
 * negative where the generalised winding number w (the sum of the triangles' signed solid angles over 4 pi) has
 * |w| > 0.5: the sign does not depend on the triangles' orientation and survives small cracks.  Refused with
 * MPM_ERR_INVALID before anything is allocated or enqueued: a vertex index out of range, a non-finite vertex, n_tris == 0,
 * a cell that is not finite and > 0, pad_cells < 2, more than 2^24 lattice nodes or more than 2^21 triangles.  The shape
 * is the engine's until mpm_destroy.  A synchronisation point (a one-time build: O(nodes x triangles), split into
 * launches over node bricks and triangle ranges so that none runs long; the result does not depend on the split).
 * mpm_sdf_shape_info: the lattice's nodes per axis, lo and cell (any pointer may be NULL); mpm_sdf_shape_download: its
 * n[0] n[1] n[2] values into a caller-owned float array. */
MPM_API int mpm_sdf_shape_from_mesh(mpm_handle_t h, const float *verts, size_t n_verts, const int32_t *tris, size_t n_tris,
                                    float cell, int pad_cells, uint32_t *shape_out);
MPM_API int mpm_sdf_shape_info(mpm_handle_t h, uint32_t shape, int32_t n[3], float lo[3], float *cell);
MPM_API int mpm_sdf_shape_download(mpm_handle_t h, uint32_t shape, float *values);
/* A mesh collider: a shape posed as body `body` (p_WB, R_WB row-major as in mpm_collider_t) with the body's spatial
 * velocity (v, w).  Its signed distance at a world point x, in float:
 *   x_B = R_WB^T (x - p_WB); q = x_B clamped to the lattice box [lo, lo + (n - 1) cell] per axis;
 *   t_a = (q_a - lo_a) * inv in float, inv = 1 / cell rounded to float once (a product, not a division);
 *   the cell of q: i_a = min(floor(t_a), n_a - 2), fraction f_a = min(t_a - i_a, 1);
 *   phi = trilinear(q) + |x_B - q|, the trilinear interpolation of the cell's eight corner values (x, then y, then z);
 *   gradient: outside the box (|x_B - q| > 0) normalize(x_B - q), inside the analytic gradient of the trilinear cell at q,
 *   normalised; when its squared length (value per cell inside, length outside) is <= 1e-30: +z_B; rotated to the world
 *   with R_WB.
 * A pair is a particle with phi < 0; its fields are those of mpm_collider_t's pairs: dist = phi, normal = -gradient,
 * rigid_v = v + w x (x - p_WB), p_WB. */
typedef struct mpm_sdf_collider {
    uint32_t shape;
    uint32_t body;
    float p_WB[3];
    float R_WB[9];
    float v[3];
    float w[3];
} mpm_sdf_collider_t;
/* The engine's mesh colliders, until the next call (n = 0 clears them; at most 1024, MPM_ERR_INVALID beyond).  Pair generation (mpm_generate_contact_pairs,
 * mpm_run_coupled_substeps, mpm_world_coupled_substeps) tests them AFTER the call's analytic colliders: pairs in
 * ascending (slot, collider) order, mesh collider m having index n_analytic + m, and "colliders" there means the analytic
 * ones plus these (a call with no analytic collider but mesh colliders is not contact-free).  Rigid poses are fixed within
 * a step: set them once per step, then run its substeps.  Stream-ordered: generations enqueued after this call see the
 * new set.  An unknown shape id is refused here; a body out of range at the generating call, before anything is
 * enqueued, as for mpm_collider_t. */
MPM_API int mpm_set_sdf_colliders(mpm_handle_t h, size_t n, const mpm_sdf_collider_t *colliders);
/* Contact material of a rigid body: the three parameters of the contact model that the solving calls take as scalars
 * (friction_mu, stiffness, damping of mpm_update_contact and mpm_coupled_params_t), per body.  materials[b] belongs to
 * rigid body b: non_mpm_id of an uploaded pair, `body` of mpm_collider_t and mpm_sdf_collider_t.  Field by field, a
 * value < 0 means "what the solving call passes"; bodies b >= n inherit all three.  Every contact's parameters are a
 * SELECT between its body's entry and the call's scalars, never arithmetic: bit for bit one or the other.  Values >= 0
 * are all legal (stiffness = 0: the body exerts nothing; damping = 0; friction_mu = 0).  The engine does not combine
 * these with properties of the cloth: where both sides have some (Drake's CalcContactFrictionFromSurfaceProperties,
 * 2 mu_A mu_B / (mu_A + mu_B)), the caller combines them and passes the result.
 * mpm_set_body_contact_materials: the engine's table until the next call (n = 0 clears it: every contact takes the
 * call's scalars again, through the kernel instances and with the bits of an engine of this library that never had a
 * table).  Independent of
 * mpm_reallocate_external_bodies.  MPM_ERR_INVALID, with the table unchanged and nothing enqueued or allocated, for a
 * field that is not finite, n > 65536, or materials == NULL with n > 0.  Stream-ordered like mpm_set_sdf_colliders
 * (and a synchronisation point: the call waits for its upload on the engine's stream): solves enqueued after the call --
 * mpm_update_contact, mpm_run_coupled_substeps, mpm_world_coupled_substeps, mpm_profile_contact_iteration -- read the new
 * table, also a solve that reuses the previous solve's set-up.  The
 * caller's array may be freed on return.  Body ids are global in a partitioned world: mpm_world_coupled_substeps refuses
 * (MPM_ERR_INVALID, nothing enqueued) local handles whose tables differ.
 * mpm_get_body_contact_materials: the table as given; min(n, capacity) entries into out (NULL with capacity 0), n into
 * *n_out. */
typedef struct { float friction_mu, stiffness, damping; } mpm_contact_material_t;
MPM_API int mpm_set_body_contact_materials(mpm_handle_t h, size_t n, const mpm_contact_material_t *materials);
MPM_API int mpm_get_body_contact_materials(mpm_handle_t h, mpm_contact_material_t *out, size_t capacity, size_t *n_out);
/* mpm_collider_signed_distance for one mesh collider: phi and the unit world gradient at n world points, by the pair
 * generator's own function.  A synchronisation point. */
MPM_API int mpm_sdf_collider_signed_distance(mpm_handle_t h, const mpm_sdf_collider_t *c, size_t n, const float *x_W,
                                             float *phi_out, float *grad_W_out);
/* n_contacts_out may be NULL: the call then waits for nothing -- the pairs are counted on the device and STAY counted
 * there; mpm_update_contact's launches have fixed grids and read the count on the device (the reference's driver reads
 * every position back, loops over the particles on the host and uploads the pairs, per substep:
 * deformable_driver.h:120-194, cuda_mpm_solver.cu:185-212).  mpm_update_contact reports the count afterwards
 * (mpm_contact_stats_t::contacts); mpm_get_contact_pair_count reads it back on request (a synchronisation point), as do
 * mpm_download_contact_pairs and a non-NULL n_contacts_out.  Up to 16 colliders travel as a kernel argument (no upload);
 * more through a device array that is refreshed only when the colliders have changed. */
MPM_API int mpm_get_contact_pair_count(mpm_handle_t h, size_t *n_contacts_out);
/* What the last mpm_update_contact worked on, without touching the device: contacts, grid nodes reached by a contact
 * stencil, and whether its set-up was the previous solve's, reused (a settled scene whose pair list repeats: no sort, no
 * per-cell runs, no node list -- verified on the device entry by entry).  Any pointer may be NULL. */
MPM_API int mpm_last_contact_counts(mpm_handle_t h, uint32_t *contacts_out, uint32_t *nodes_out, int *setup_reused_out);
/* Tests: {mpm_update_contact calls that solved, of them on a reused set-up, solves refused on the device because a guess of
 * the host's was wrong (repeated with the full set-up), pair generations / solves repeated after a buffer overflow,
 * substeps of mpm_run_coupled_substeps that were enqueued contact-free (no particle in any collider when the substep before
 * ended), of them skipped on the device and repeated as coupled substeps}. */
MPM_API int mpm_debug_contact_counters(mpm_handle_t h, uint64_t out6[6]);
/* Tests of the invariant that no kernel of the solve indexes a per-pair array with a count it has not clamped to the
 * capacity that sized the array (the reference sizes its launches from a host count, cuda_mpm_solver.cu:222-232; here the
 * count of device-made pairs never leaves the device).  Overwrites the count mpm_generate_contact_pairs left on the device
 * (count >= 0) and / or shifts the number of the pair generation that wrote it (stamp_delta != 0: "a count some other
 * generation left", i.e. a stale one).  The next mpm_update_contact must refuse: MPM_ERR_CAPACITY for a count outside
 * [0, capacity], MPM_ERR_INTERNAL for a stale one -- nothing indexed, nothing solved; pairs made again afterwards solve as
 * if nothing had happened.  Needs pairs counted on the device (n_contacts_out == NULL). */
MPM_API int mpm_debug_contact_count(mpm_handle_t h, int count, int stamp_delta);
/* Tests of the contact watch alone (the kernel behind a contact-free substep of mpm_run_coupled_substeps, which decides
 * whether the next substep may go without pair generation and solve): one launch of it over the current particle state
 * -- vertices where they are, faces at the centroid of their corners, formed by the kernel -- against the given
 * colliders and the engine's mesh colliders, ungated.  *hit_out: 1 when some active particle may be within the watch's
 * margin (a thousandth of a cell) of the inside of a collider, else 0.  Validates like mpm_generate_contact_pairs; leaves
 * the pairs in the engine and the analytic colliders of the last generation as they are (the device table of the mesh
 * colliders is brought up to date with the engine's set, as a generation would do).  Needs a finalized engine (the first
 * re-sort has numbered the active particles).  A synchronisation point. */
MPM_API int mpm_debug_contact_watch(mpm_handle_t h, size_t n_colliders, const mpm_collider_t *colliders, int *hit_out);
MPM_API int mpm_download_contact_pairs(mpm_handle_t h, uint32_t *particle_in_contact_index, uint32_t *non_mpm_id,
                                       float *penetration_distance, float *normal, float *position, float *rigid_v,
                                       float *rigid_p_WB);

/* GpuMpmSolver::UpdateContact (cuda_mpm_solver.cu:214-621).  iterations_out,
 * residual_out may be NULL.  frame/substep/dump only name the optional JSON
 * statistics file (written to dump_dir set by mpm_set_dump_dir, default ".").
 * max_newton_iterations <= 0 selects the reference's 2000. */
MPM_API int mpm_update_contact(mpm_handle_t h, int frame, int substep, float dt, float friction_mu, float stiffness,
                               float damping, int dump, int exact_line_search, int max_newton_iterations,
                               int *iterations_out, float *residual_out);
MPM_API int mpm_set_dump_dir(mpm_handle_t h, const char *dir);

/* The numbers the reference prints and dumps per UpdateContact call (cuda_mpm_solver.cu:577-612:
 * iteration count, residual, line-search count, energy), plus the step and energies of the LAST
 * Newton iteration so that a single iteration (max_newton_iterations = 1) can be compared:
 * alpha = accepted step, energy = E(alpha) as the line search evaluated it, E0 = E(0),
 * norm_dir_sq / dofs = sum |Dir|^2 before relaxation and the DoF count (cuda_mpm_solver.cu:567-570). */
typedef struct {
    int32_t iterations;
    int32_t line_search_evals;   /* summed over the iterations */
    uint32_t contacts;
    uint32_t nodes;              /* grid nodes reached by a contact stencil */
    float residual;
    float alpha;
    float energy;
    float E0;
    float norm_dir_sq;
    float dofs;
} mpm_contact_stats_t;
MPM_API int mpm_get_contact_stats(mpm_handle_t h, mpm_contact_stats_t *out);

/* The decisions of the last mpm_update_contact, one row per Newton iteration -- what the reference's host loop decides per
 * iteration (cuda_mpm_solver.cu:472-528 backtracking, :383-471 exact search, :567-570 stopping test) and dumps as JSON
 * for the exact search (:587-612).  Row = MPM_CONTACT_LOG_FLOATS floats:
 *   [0] residual sqrt(sum |Dir|^2) / DoFs   [1] line-search evaluations   [2] E(alpha)   [3] accepted alpha   [4] E(0)
 *   [5] sum |Dir|^2 (before relaxation)     [6] DoFs                      [7] 0
 * At most 2048 iterations are kept.  rows_out may be NULL (count only). */
#define MPM_CONTACT_LOG_FLOATS 8
MPM_API int mpm_download_contact_log(mpm_handle_t h, float *rows_out, size_t capacity_rows, size_t *n_rows_out);

/* ---- conveniences on top of the reference interface ---------------------- */

/* The five solver calls of one contact-free substep (cuda_mpm_test.cc:66-72,
 * deformable_driver.h:244-258 without the contact part), without host syncs. */
MPM_API int mpm_substep(mpm_handle_t h, float dt, int mpm_bc);
MPM_API int mpm_run_substeps(mpm_handle_t h, int n, float dt, int mpm_bc);

/* The same for COUPLED substeps: the body of DeformableDriver::CalcAbstractStates' loop
 * (multibody/plant/deformable_driver.h:240-258) n times in one call, for rigid bodies with analytic signed distance
 * fields (mpm_collider_t, see mpm_generate_contact_pairs): RebuildMapping, CalcFemStateAndForce, ParticleToGrid,
 * UpdateGrid(mpm_bc), contact pairs on the device, UpdateContact(dt, mu, stiffness, damping, exact), GridToParticle.
 * The results are those of the seven calls (the tests compare them bit for bit); the host waits once per substep, for
 * the word that says the solve has converged.  mpm_reallocate_external_bodies must have been called (the per-body
 * impulses accumulate over the n substeps, as over the substeps of one plant step: deformable_driver.h:196-219).
 * While nothing touches a collider the call goes without pair generation and solve: after a substep without pairs a watch
 * kernel asks whether the NEXT substep would have any (a pair is a particle with phi < 0 where the substep starts: exact),
 * and the substeps that follow are enqueued contact-free, each checked the same way; the ones that turn out to have pairs
 * skip themselves on the device and are run again as coupled substeps.  Their results report 0 contacts and iterations.
 * results: n entries or NULL. */
typedef struct {
    float dt;
    int32_t mpm_bc;
    float friction_mu, stiffness, damping;
    int32_t exact_line_search;
    int32_t max_newton_iterations;   /* <= 0: the reference's 2000 */
} mpm_coupled_params_t;
typedef struct {
    int32_t iterations;
    uint32_t contacts, nodes;
    float residual;
    int32_t setup_reused;
} mpm_coupled_result_t;
MPM_API int mpm_run_coupled_substeps(mpm_handle_t h, int n, const mpm_coupled_params_t *params, size_t n_colliders,
                                     const mpm_collider_t *colliders, mpm_coupled_result_t *results);
/* (partitioned domains: see mpm_team_prepare below) */
MPM_API int mpm_world_coupled_substeps(mpm_handle_t *handles, int n_local, int n, const mpm_coupled_params_t *params,
                                       size_t n_colliders, const mpm_collider_t *colliders, mpm_coupled_result_t *const *results);

/* ---- Fixed constraints: cloth vertices pinned to rigid bodies (an extension) ----
 * DeformableModel::AddFixedConstraint (deformable_model.h:227-230) for the MPM cloth.
 * A pin is (vertex, body, p_BQ): `vertex` indexes the vertex numbering of mpm_add_qr_cloth / mpm_dump_cpu_state (global
 * over all cloths in call order; particle id n_faces + vertex), p_BQ is the attachment point in the body frame.
 * A body motion is set per body: the pose (p_WB, R_WB row-major, body -> world) at the start of the next substep and a
 * constant spatial velocity (v, w), world frame.  Setting it restarts that body's clock: t = 0.
 * At the end of every GridToParticle that runs -- mpm_grid_to_particle, mpm_substep, mpm_run_substeps (owed substeps
 * included), mpm_run_coupled_substeps and the contact-free substeps it enqueues behind a watch -- the clock first advances
 * by the substep's dt (after the k-th substep t = sum of the dt), then every pinned vertex gets, with p(t) = p_WB + t v and
 * R(t) = Rodrigues(t w) R_WB:
 *   x = p(t) + R(t) p_BQ;   v_Q = v + w x (x - p(t));   C = [w]x  (the exact velocity gradient of the rigid motion;
 *   GridToParticle's RPIC blend maps a skew C to itself).
 * A substep that skips itself (it is run again later) neither moves a pin nor advances a clock.
 * Reaction: with m the particle's ParticleToGrid mass and v_g2p the velocity GridToParticle wrote for it, the constraint
 * gives the cloth the impulse m (v_Q - v_g2p); body `body` receives force impulse l = m (v_g2p - v_Q) and torque
 * (x - p_WB) x l about the p_WB of its motion, in the accumulators of the contact impulses (64-bit fixed point: the sums
 * do not depend on the order) read by mpm_external_body_force_to_host and mpm_finalize_external_contact_forces.  A pin
 * whose body is >= the mpm_reallocate_external_bodies count moves its vertex and adds no impulse.
 * Pinned vertices still take part in CalcFemStateAndForce, ParticleToGrid and contact-pair generation like any other
 * vertex: a selection shape that is also a collision geometry of the same body produces contacts with the pinned
 * vertices.  A target that leaves its block's tile asks for a re-sort as an advected particle does; one outside the grid
 * is reported as MPM_ERR_DOMAIN.
 * Refused with MPM_ERR_INVALID before anything is enqueued, the state untouched: a call before mpm_finalize, a vertex
 * >= n_verts, a vertex twice in one mpm_set_pins, a non-finite p_BQ, pose or velocity, an R_WB that is not a rotation
 * (|R^T R - I| and |det R - 1| within 1e-4), a body twice in one mpm_set_body_motions, and any partitioned or multi-rank
 * engine (mpm_dist_init, mpm_chain_*, mpm_team_*: out of scope) -- the pin calls on such an engine, and mpm_dist_init,
 * the halo, chain and team substeps on an engine with pins.  A substep entry point called while some pin's body has no
 * motion is refused the same way.  With no pins nothing is launched.  Stream-ordered: substeps enqueued after a call see
 * its pins and motions. */
typedef struct mpm_pin {
    uint32_t vertex;
    uint32_t body;
    float p_BQ[3];
} mpm_pin_t;
typedef struct mpm_body_motion {
    uint32_t body;
    float p_WB[3];
    float R_WB[9];
    float v[3], w[3];
} mpm_body_motion_t;
/* Replaces the pin set (n = 0 clears it; pins may then be NULL). */
MPM_API int mpm_set_pins(mpm_handle_t h, size_t n, const mpm_pin_t *pins);
/* Sets the motion of n bodies (once per plant step: the body poses of CalcAbstractStates). */
MPM_API int mpm_set_body_motions(mpm_handle_t h, size_t n, const mpm_body_motion_t *motions);
/* AddFixedConstraint's selection: every vertex whose current position has phi <= 0 for the analytic shape (kinds 0-5;
 * phi by the function of mpm_collider_signed_distance, the shape posed by its own p_WB / R_WB) is pinned to `body`
 * with p_BQ = R_WB^T (x - p_WB) for the body pose given here.  The new pins are appended to the set; a vertex already
 * pinned keeps its pin and is not counted.  *n_added (may be NULL): the pins added.  No new vertex inside:
 * MPM_ERR_INVALID, nothing added.  A synchronisation point. */
MPM_API int mpm_pins_inside_collider(mpm_handle_t h, const mpm_collider_t *shape, uint32_t body, const float p_WB[3],
                                     const float R_WB[9], size_t *n_added);
/* The pin set in order: min(n, capacity) pins into out (may be NULL when capacity is 0), n into *n_out. */
MPM_API int mpm_get_pins(mpm_handle_t h, mpm_pin_t *out, size_t capacity, size_t *n_out);

/* ---- Per-cloth materials (an extension) ----
 * DeformableModel::RegisterDeformableBody takes a DeformableBodyConfig per body (deformable_model.h:161-163); this is
 * that choice for the MPM cloth.  The per-cloth fields are E, nu, rho, gamma, K and c_F, with the meanings of the
 * same fields of mpm_material_t.  Everything else stays engine-wide, taken from the material given to mpm_create:
 * the RPIC blend V (read by GridToParticle), gravity and its axis, epsv, sdf_friction and the wall cells.
 * An engine that receives at least one mpm_add_qr_cloth_with_material call becomes multi-material at mpm_finalize;
 * its cloths added with plain mpm_add_qr_cloth (before or after) get the engine's material, as does a NULL `m`.
 * An engine that never calls it runs exactly as before.
 * In a multi-material engine a particle's ParticleToGrid mass is the float product vol * rho of its cloth, the same
 * float a single-material engine with that density forms; MPM_ARR_MASSES returns it on every engine.  MPM_ARR_VOLUMES
 * still returns volumes (within one float ulp: mass / rho) and mpm_upload_particle_state still takes volumes.
 * Refused with MPM_ERR_INVALID, nothing recorded: a call after mpm_finalize, a non-finite field, E <= 0, nu outside
 * [0, 0.5), rho <= 0, gamma, K or c_F below 0, and more than 256 cloths in a multi-material engine (a plain
 * mpm_add_qr_cloth that would be the 257th included).  Partitioned and multi-rank engines are out of scope: a
 * multi-material engine refuses mpm_dist_init, mpm_chain_*, mpm_team_* and the halo, chain, team and world substeps
 * with MPM_ERR_INVALID.  Materials cannot change after mpm_finalize. */
typedef struct mpm_cloth_material {
    float youngs_modulus, poisson_ratio, density, gamma, K, c_F;   /* meanings as in mpm_material_t */
} mpm_cloth_material_t;
/* GpuMpmState::AddQRCloth with a material of its own (m NULL: the engine's material). */
MPM_API int mpm_add_qr_cloth_with_material(mpm_handle_t h, const float *pos, const float *vel, size_t n_verts,
                                           const int32_t *indices, size_t n_faces, const mpm_cloth_material_t *m);
/* Cloth `cloth` in call order (plain mpm_add_qr_cloth calls count too): its vertex range (vertex numbering of
 * mpm_dump_cpu_state), its face range (original face order) and its material.  Any output may be NULL.  Valid before
 * and after mpm_finalize. */
MPM_API int mpm_get_cloth_info(mpm_handle_t h, size_t cloth, size_t *first_vertex, size_t *n_verts,
                               size_t *first_face, size_t *n_faces, mpm_cloth_material_t *m);
/* The number of cloths added so far. */
MPM_API int mpm_cloth_count(mpm_handle_t h, size_t *n_out);

/* ---- Rigid bodies in the grid update (an extension) ----
 * The boundary condition of UpdateGrid for posed, moving rigid bodies of every kind the contact path knows, with the
 * reaction on the bodies: what mpm_set_grid_colliders does for an unposed sphere and a half-space, for the six analytic
 * kinds of mpm_collider_t and the mesh lattices of mpm_sdf_shape_from_mesh, at the cost of the grid update instead of the
 * contact solve.  mpm_bc = MPM_BC_BODIES selects the table set with mpm_set_grid_bodies wherever an entry point takes
 * mpm_bc: mpm_update_grid, mpm_substep, mpm_run_substeps (owed and replayed substeps included),
 * mpm_run_coupled_substeps, mpm_profile_substeps.  With an empty table it behaves as mpm_bc = -1.
 * The domain walls act first, as always.  Then, for a node with mass at x = (idx + 0.5) dx, the FIRST body of the table
 * that contains the node decides:
 *   membership and normal are the pair generator's (mpm_generate_contact_pairs), so that both coupling paths agree about
 *     where a body's surface is: an analytic body contains x when mpm_collider_t's membership holds (phi(x) < 0 for
 *     kinds 0-4, sum (x_B,i / a_i)^2 < 1 for the ellipsoid), a mesh body when the interpolant of mpm_sdf_collider_t gives
 *     phi(x) < 0; n is the unit world gradient of phi that mpm_collider_signed_distance /
 *     mpm_sdf_collider_signed_distance return at x (the ellipsoid's exact nearest-point gradient, evaluated for member
 *     nodes only);
 *   the body's velocity at the node is the rigid velocity field v_c(x) = v + w x (x - p_WB);
 *   the three modes of mpm_grid_collider_t apply with v_c(x) as the collider velocity:
 *     MPM_GC_FIXED             v <- v_c(x)   (v + (v_c - v), :778-781, written without the rounding residue of v)
 *     MPM_GC_SLIP_APPROACHING  only if n.(v_c - v) > 0, then
 *     MPM_GC_SLIP              v += mu (v_c - v) + (1 - mu) n (n.(v_c - v)), the product (n.(v_c - v)) (1 - mu) formed in
 *                              double as in the reference (:783-786).
 * Reaction: for a node of mass m decided by a body, with v_in the velocity after the walls and v_out the velocity
 * written, body `shape.body` receives the force impulse l = -m (v_out - v_in) and the torque impulse (x - p_WB) x l, in
 * the accumulators of the contact impulses (64-bit fixed point, the contact impulses' scale: the sums do not depend on the
 * order) read by mpm_external_body_force_to_host and mpm_finalize_external_contact_forces.  A body index >= the
 * mpm_reallocate_external_bodies count acts on the cloth and accumulates nothing.  A substep that skips itself adds
 * nothing; its replay adds once.  A contribution outside the fixed-point range raises MPM_ERR_RANGE at the next
 * mpm_sync, as a contact impulse does.
 * Poses are fixed between two calls of mpm_set_grid_bodies: set the table once per plant step, then run its substeps.
 * The call needs mpm_finalize, is ordered on the engine's stream and is a synchronisation point; substeps that
 * mpm_run_substeps still owes are run with the table they were enqueued with before the new one takes effect.
 * Refused with MPM_ERR_INVALID before anything is enqueued, the previous table staying in force: n > 16; for an analytic
 * body a kind outside 0-5 or dimensions mpm_collider_t refuses; a sdf_shape that is neither MPM_GB_NO_MESH nor a shape
 * of this engine; a mode outside 0-2; a friction that is not finite; a non-finite p_WB, v or w; an R_WB that is not a
 * rotation (|R^T R - I| and |det R - 1| within 1e-4); and any partitioned or multi-rank engine (mpm_dist_init,
 * mpm_chain_*, mpm_team_*: shared blocks are updated by two ranks there and would count their impulses twice) -- this
 * call on such an engine, and mpm_dist_init, the halo, chain, team and world substeps on an engine with a non-empty
 * table.  mpm_update_grid_from_sums and mpm_substep_end refuse MPM_BC_BODIES with a non-empty table. */
#define MPM_BC_BODIES 5                 /* mpm_bc value: walls + the table of mpm_set_grid_bodies */
#define MPM_GB_NO_MESH 0xFFFFFFFFu
typedef struct mpm_grid_body {
    mpm_collider_t shape;   /* kind 0-5, body, p_WB, R_WB, dims, v, w: meanings and validity rules of mpm_collider_t */
    uint32_t sdf_shape;     /* MPM_GB_NO_MESH, or a shape id of mpm_sdf_shape_from_mesh: then kind and dims are ignored */
    int32_t mode;           /* MPM_GC_FIXED, MPM_GC_SLIP_APPROACHING, MPM_GC_SLIP */
    float friction;         /* < 0: the engine's material.sdf_friction, as in mpm_grid_collider_t */
} mpm_grid_body_t;
/* Replaces the table (n <= 16; n = 0 clears it, bodies may then be NULL). */
MPM_API int mpm_set_grid_bodies(mpm_handle_t h, size_t n, const mpm_grid_body_t *bodies);
/* The table as given: min(n, capacity) entries into out (may be NULL when capacity is 0), n into *n_out. */
MPM_API int mpm_get_grid_bodies(mpm_handle_t h, mpm_grid_body_t *out, size_t capacity, size_t *n_out);

/* ---- External force fields on the cloth (an extension) ----
 * Body loads other than the material's one gravity on one axis: off-axis gravity, springs towards a point, the
 * centrifugal term of a rotating frame, air drag towards a wind, drag along the cloth's normal.  A table of at most
 * MPM_MAX_FORCE_FIELDS fields.  Each field has an affine vector field u(x) = u0 + G (x - x0), G row-major 3 x 3, and,
 * with MPM_FF_REGION, acts only on particles with lo <= x <= hi (closed, per axis, tested on the particle's float
 * position).  ALL COEFFICIENTS ARE PER UNIT MASS: a particle's acceleration is the sum, in table order, over the fields
 * whose region contains it, of
 *   MPM_FF_ACCEL        u(x)                                  face and vertex particles
 *   MPM_FF_DRAG         -gamma (v - u(x))                     face and vertex particles; gamma in 1/s, u the wind velocity
 *   MPM_FF_NORMAL_DRAG  -gamma s n, s = (v - u(x)) . n        face particles only; with MPM_FF_QUADRATIC -gamma s |s| n
 *                                                             (gamma then in 1/m)
 * with n = d / |d|, d = F[:,2] the face's director (its sign cancels; a field contributes nothing where |d|^2 < 1e-30),
 * 1 / |d| formed with a correctly rounded square root and division whatever mpm_set_fast_math says.  The force on a
 * particle is m a with m the mass ParticleToGrid forms (volume x density, per-cloth densities included); a caller
 * with a coefficient c per unit VOLUME (a force density c (u - v), N/m^3 per m/s) passes gamma = c / rho.
 * Evaluation is explicit, inside ParticleToGrid, on the state it reads: m a dt joins the particle's momentum; a face
 * particle's velocity is the mean of its corners' that CalcFemStateAndForce wrote.  It works with pins, per-cloth
 * materials, grid bodies, deterministic mode, fast math and the coupled path.
 * Stability: every substep entry point that takes a dt (mpm_particle_to_grid, mpm_substep_begin, mpm_substep,
 * mpm_run_substeps, mpm_run_coupled_substeps, mpm_profile_substeps) returns MPM_ERR_INVALID, before anything is
 * enqueued, when dt * (sum of gamma over the MPM_FF_DRAG and linear MPM_FF_NORMAL_DRAG fields) > 1: an explicit drag
 * beyond that reverses the relative velocity.  Quadratic fields cannot be bounded this way (their rate is gamma |s|):
 * keeping dt gamma |s| well below 1 is the caller's responsibility.
 * mpm_set_force_fields needs mpm_finalize, is ordered on the engine's stream and is a synchronisation point; substeps
 * that mpm_run_substeps still owes are run with the table they were enqueued with before the new one takes effect.
 * Time-dependent fields: set the table between batches.  While a table is set the engine does not use the re-sort's
 * quiet-time estimate (which assumes gravity alone) to omit re-sort check launches.
 * Refused with MPM_ERR_INVALID, the previous table staying in force: n > 8; an unknown kind or unknown flags; a number
 * that is not finite; gamma < 0; lo > hi on any axis (checked whether or not MPM_FF_REGION is set); any partitioned or
 * multi-rank engine -- this call on such an engine, and mpm_dist_init, the halo, chain, team and world substeps on an
 * engine with a non-empty table. */
#define MPM_MAX_FORCE_FIELDS 8
#define MPM_FF_ACCEL 0
#define MPM_FF_DRAG 1
#define MPM_FF_NORMAL_DRAG 2
#define MPM_FF_QUADRATIC 1u             /* flags: MPM_FF_NORMAL_DRAG is quadratic in the normal speed */
#define MPM_FF_REGION 2u                /* flags: the field acts inside lo <= x <= hi only */
typedef struct mpm_force_field {
    int32_t kind;           /* MPM_FF_ACCEL, MPM_FF_DRAG, MPM_FF_NORMAL_DRAG */
    uint32_t flags;         /* MPM_FF_QUADRATIC | MPM_FF_REGION */
    float gamma;            /* drag rate per unit mass, >= 0 (ignored by MPM_FF_ACCEL) */
    float u0[3];            /* u(x) = u0 + G (x - x0) */
    float G[9];             /* row-major */
    float x0[3];
    float lo[3], hi[3];     /* the region (MPM_FF_REGION); lo <= hi always */
} mpm_force_field_t;
/* Replaces the table (n <= 8; n = 0 clears it, fields may then be NULL). */
MPM_API int mpm_set_force_fields(mpm_handle_t h, size_t n, const mpm_force_field_t *fields);
/* The table as given: min(n, capacity) entries into out (may be NULL when capacity is 0), n into *n_out. */
MPM_API int mpm_get_force_fields(mpm_handle_t h, mpm_force_field_t *out, size_t capacity, size_t *n_out);
/* The acceleration of n particles under a table, on the host (no handle, no device): the inline function
 * ParticleToGrid calls, compiled for the host.  x, v, acc_out: n x 3 floats; director: n x 3 floats (F[:,2] of face
 * particles), or NULL for vertex particles.  The table is validated as by mpm_set_force_fields. */
MPM_API int mpm_force_field_acceleration(const mpm_force_field_t *fields, size_t n_fields, size_t n, const float *x,
                                         const float *v, const float *director, float *acc_out);

/* ---- Bending stiffness of the cloth, per cloth (an extension) ----
 * The membrane model resists stretch, shear and change of the director, not folding: an isometric fold costs nothing.
 * This adds the quadratic hinge energy of Bergou et al. 2006 / Wardetzky et al. 2007 for a rest shape that is flat per
 * hinge (the positions given to mpm_add_qr_cloth*; rest angles zero).  Every interior edge x0 x1 shared by exactly two
 * faces of one cloth is a hinge (x0, x1 | x2, x3), x2 opposite the edge in face A, x3 in face B.  With a0, a1 the rest
 * angles of face A at x0, x1, b0, b1 those of face B and A_A, A_B the rest areas,
 *   K = (cot a1 + cot b1, cot a0 + cot b0, -(cot a0 + cot a1), -(cot b0 + cot b1)),   c = 3 / (A_A + A_B),
 *   E = 1/2 k sum_h c_h |sum_j K_hj x_j|^2 = 1/2 x^T (k Q) x,   f = -k Q x   on the vertex particles.
 * Q is constant, symmetric, sparse (13 entries per row on a regular valence-6 mesh), its rows sum to zero: the force is
 * linear in the positions, zero on every affine image of the rest shape, and its total and total torque vanish.
 * Boundary edges and edges with more than two faces form no hinge.  k is a flexural rigidity (N m); the discrete energy
 * of a right-triangle grid bent onto a cylinder of radius R is about 3 x 1/2 k A / R^2 (the model's mesh-dependent
 * factor: calibrate k against the mesh in use).
 * The force joins the vertex forces of CalcFemStateAndForce (MPM_ARR_FORCES includes it; its kernel runs behind the
 * vertex-force kernel and counts under MPM_PHASE_VFORCE).  It works with pins, per-cloth materials, grid bodies, force
 * fields, deterministic mode, fast math and the coupled path, and is the same bits whatever the particle order.
 * mpm_set_bending needs mpm_finalize, is ordered on the engine's stream and is a synchronisation point; substeps that
 * mpm_run_substeps still owes are run first, with the stiffness they were enqueued with.  stiffness[c] >= 0 is cloth
 * c's k; n_cloths must be mpm_cloth_count, or 0.  All zeros or n_cloths = 0 switches the feature off: the engine then
 * launches exactly what it launches without this call.  While it is on the engine does not use the re-sort's quiet-time
 * estimate to omit re-sort check launches, and every batched substep launches the vertex-force kernel.
 * Stability: the entry points that take a dt and check the force fields' (see above) also return MPM_ERR_INVALID,
 * before anything is enqueued, for a dt above mpm_bending_max_stable_dt = 2 / sqrt(max_i (1 / m_i) sum_j |k Q_ij|), m_i
 * the vertex particle's mass as of mpm_set_bending: Gershgorin's bound on the lumped system, on which symplectic Euler
 * needs dt omega <= 2.  It is conservative for MPM (the grid shares a vertex's impulse with the face particles around
 * it): a guard, not a guarantee.  +inf while the feature is off.
 * Refused with MPM_ERR_INVALID, nothing changed: a stiffness that is negative or not finite; a wrong count; a call
 * before mpm_finalize; a face with a hinge whose rest area is zero or whose rest cotangent is not finite, in a cloth
 * with k > 0 (the message names the face); any partitioned or multi-rank engine -- this call on such an engine, and
 * mpm_dist_init, the halo, chain, team and world substeps on an engine with bending on. */
MPM_API int mpm_set_bending(mpm_handle_t h, size_t n_cloths, const float *stiffness);
/* The stiffness in force: min(mpm_cloth_count, capacity) values into out (zeros while off), the cloth count into *n_out. */
MPM_API int mpm_get_bending(mpm_handle_t h, float *out, size_t capacity, size_t *n_out);
/* -k Q x on the current positions: f_out[3 * n_verts], in the vertex numbering of mpm_dump_cpu_state (zeros for the
 * vertices of cloths without bending).  The device function of the substep's kernel; changes no state. */
MPM_API int mpm_bending_forces(mpm_handle_t h, float *f_out);
MPM_API int mpm_bending_max_stable_dt(mpm_handle_t h, float *dt_out);
/* Q of one cloth on the host (no handle, no device), in double from the float rest positions pos[3 * n_verts] and the
 * triangles indices[3 * n_faces], as CSR: ascending columns, the diagonal included, every pair of vertices that shares
 * a hinge present.  row_offsets[n_verts + 1] (may be NULL); min(nnz, capacity) entries into cols / vals (may be NULL
 * when capacity is 0); nnz into *nnz_out: call once with capacity 0 for the size.  MPM_ERR_INVALID, naming the face,
 * when a face with a hinge has zero rest area or a cotangent that is not finite. */
MPM_API int mpm_bending_matrix(const float *pos, size_t n_verts, const int32_t *indices, size_t n_faces, size_t *row_offsets,
                               int32_t *cols, double *vals, size_t capacity, size_t *nnz_out);

/* ---- Stiffness-proportional damping of the cloth, per cloth (an extension) ----
 * The stiffness half of a Rayleigh pair (Drake's DeformableBodyConfig::stiffness_damping_coefficient), as a material
 * damper: per cloth two coefficients in seconds, both >= 0.
 *   membrane  Kelvin-Voigt on the in-plane Green strain.  Per face, with F2 = [x1 - x0, x2 - x0] Dm^-1 the in-plane
 *             columns of F and dF2 the same of the corner velocities: Edot = 1/2 (F2^T dF2 + dF2^T F2),
 *             S = beta (2 mu Edot + lambda tr(Edot) I) with the cloth's Lame parameters, P = F2 S, corner records
 *             G = vol P grad_N, vertex force -sum G.  Linear in v; zero for every rigid velocity field whatever the
 *             deformation; total force and torque vanish; power -sum f.v = sum vol S:Edot >= 0.  The director column
 *             of F (the gamma, K and c_F terms) is not damped.
 *   bending   f = -beta k Q v, the hinge operator of mpm_set_bending on the velocities; it acts only on a cloth whose
 *             bending stiffness k is > 0 (a beta on a cloth with k = 0 is accepted and does nothing), and follows a
 *             later mpm_set_bending.
 * The forces join the vertex forces of CalcFemStateAndForce (MPM_ARR_FORCES includes them): the membrane kernel runs
 * directly behind the face kernel and adds its records to the elastic ones (it counts under MPM_PHASE_FEM), the bending
 * one behind the bending kernel (MPM_PHASE_VFORCE).  It works with pins, per-cloth materials, grid bodies, force
 * fields, bending, fast math, deterministic mode and the coupled path.
 * mpm_set_damping needs mpm_finalize, is ordered on the engine's stream and is a synchronisation point; substeps that
 * mpm_run_substeps still owes are run first, with the old coefficients.  n_cloths must be mpm_cloth_count, or 0.  All
 * zeros or n_cloths = 0 switches the feature off: the engine then launches exactly what it launches without this call.
 * While it is on the engine does not use the re-sort's quiet-time estimate to omit re-sort check launches.
 * Stability: explicit viscous forces need dt rho(M^-1 D) <= 2.  The entry points that check
 * mpm_bending_max_stable_dt also return MPM_ERR_INVALID, before anything is enqueued, for a dt above
 *   mpm_damping_max_stable_dt = 2 / max_i (1 / m_i) [ sum_{faces f around i} beta_m vol_f (2 mu + 2 lambda) |g_i| (|g_0| + |g_1| + |g_2|)
 *                                                     + beta_b sum_j |k Q_ij| ],
 * g_j the columns of the face's grad_N, m_i the vertex particle's mass as of the call, 2 mu + 2 lambda the largest
 * eigenvalue of Edot -> 2 mu Edot + lambda tr(Edot) I: Gershgorin's bound at the REST shape.  A cloth stretched by a
 * factor s lowers the true limit by about s^2 (F2 enters twice); on the other hand the grid shares a vertex's impulse
 * with the face particles around it.  It is a guard, not a guarantee, and how conservative it is has not been
 * measured.  +inf while the feature is off.
 * Refused with MPM_ERR_INVALID, nothing changed: a coefficient that is negative or not finite; a wrong count; a call
 * before mpm_finalize; any partitioned or multi-rank engine -- this call on such an engine, and mpm_dist_init, the
 * halo, chain, team and world substeps on an engine with damping on. */
typedef struct mpm_cloth_damping {
    float membrane, bending;   /* seconds, >= 0 */
} mpm_cloth_damping_t;
MPM_API int mpm_set_damping(mpm_handle_t h, size_t n_cloths, const mpm_cloth_damping_t *d);
/* The coefficients in force: min(mpm_cloth_count, capacity) entries into out (zeros while off), the cloth count into *n_out. */
MPM_API int mpm_get_damping(mpm_handle_t h, mpm_cloth_damping_t *out, size_t capacity, size_t *n_out);
/* The membrane + bending damping force on the current positions and velocities: f_out[3 * n_verts], in the vertex
 * numbering of mpm_dump_cpu_state (zeros for the vertices of undamped cloths).  The device functions of the substep's
 * kernels; a vertex's face records are summed on the host in ascending face id, as the vertex-force kernel sums them.
 * Changes no state. */
MPM_API int mpm_damping_forces(mpm_handle_t h, float *f_out);
MPM_API int mpm_damping_max_stable_dt(mpm_handle_t h, float *dt_out);
/* The membrane kernel's face function on the host (no handle, no device), face by face: dminv3[3 n] = (Dm0, Dm1, Dm3)
 * of Dm^-1 = [Dm0 Dm1; 0 Dm3], vol[n], mu[n], lambda[n], beta[n], x9 / v9[9 n] the corners' positions and velocities
 * ([corner][component]); rec9_out[9 n] the corner records G ([corner][component]; the force on a corner is -G). */
MPM_API int mpm_damping_face_records(size_t n_faces, const float *dminv3, const float *vol, const float *mu,
                                     const float *lambda, const float *beta, const float *x9, const float *v9,
                                     float *rec9_out);

/* ---- Woven cloth: orthotropic warp / weft / shear stiffness per cloth (an extension) ----
 * The membrane of the face kernel is isotropic: one E, one nu per cloth.  Woven fabric has warp and weft moduli that
 * differ by factors, and a shear modulus orders of magnitude below both.  The weave is an ADDED orthotropic St. Venant-
 * Kirchhoff energy on the in-plane Green strain, resolved along per-face material axes; the isotropic model stays as
 * the fabric's matrix (lower the cloth's E and let the weave carry the yarn directions).
 * Per face with corners 0, 1, 2, rest Dm^-1 = [Dm0 Dm1; 0 Dm3] and rest volume vol (area x thickness): the rest frame
 * is e1 along the rest edge 0 -> 1, e2 the in-plane perpendicular towards corner 2; the warp is the unit vector
 * a = (c, s) in that frame, the weft b = (-s, c), and
 *   F2  = [x1 - x0, x2 - x0] Dm^-1,  E = 1/2 (F2^T F2 - I),  Eaa = a^T E a,  Ebb = b^T E b,  Eab = a^T E b
 *   Psi = 1/2 ka Eaa^2 + 1/2 kb Ebb^2 + kab Eaa Ebb + 2 G Eab^2                           (per rest volume)
 *   Saa = ka Eaa + kab Ebb,  Sbb = kb Ebb + kab Eaa,  Sab = 2 G Eab,  S = Saa a a^T + Sbb b b^T + Sab (a b^T + b a^T)
 *   P = F2 S,  corner records G_rec = vol P grad_N,  vertex force -sum G_rec.
 * Stateless, rotation invariant, with an energy; total force and torque vanish.  The constants per cloth are in Pa like
 * the cloth's E: E_warp, E_weft >= 0, G >= 0, nu the weft contraction per unit warp extension.  With
 * D = 1 - nu^2 E_weft / E_warp:  ka = E_warp / D, kb = E_weft / D, kab = nu E_weft / D, formed in double and rounded once
 * to float.  D must be > 0; E_warp = 0 requires nu = 0 (then ka = kab = 0, kb = E_weft).  A cloth whose four constants
 * are zero has no weave: its faces write nothing.
 * Axes: warp_dir is a rest-space direction per cloth; face_dirs (NULL, or 3 floats per face in the face numbering of
 * mpm_dump_cpu_state) gives a direction per face, for panels cut on the bias; a face whose entry is (0, 0, 0) falls
 * back to its cloth's warp_dir.  Once, at the call, on the host in double from the rest positions: the direction is
 * projected onto the face's rest plane and normalised, and (c, s), its components on (e1, e2), are rounded to float.
 * The kernel does not renormalise.  A projection shorter than 1e-3 |d| (a yarn that stands on the face), or a zero d,
 * on a face of a cloth WITH weave is refused with MPM_ERR_INVALID; the message names the face.
 * The force joins the vertex forces of CalcFemStateAndForce (MPM_ARR_FORCES includes it): its kernel runs directly
 * behind the face kernel and BEFORE the membrane damping kernel, and adds its records to the elastic ones (it counts
 * under MPM_PHASE_FEM).  It works with pins, per-cloth materials, grid bodies, force fields, bending, damping, links,
 * pressure, shell bending, anchors, fast math, deterministic mode and the coupled path.
 * mpm_set_weave needs mpm_finalize, is ordered on the engine's stream and is a synchronisation point; substeps that
 * mpm_run_substeps still owes are run first, with the old table.  n_cloths must be mpm_cloth_count, or 0.  All-zero
 * constants or n_cloths = 0 switches the feature off: the engine then launches exactly what it launches without this
 * call.  While it is on the engine does not use the re-sort's quiet-time estimate to omit re-sort check launches.
 * Stability: the entry points that check mpm_bending_max_stable_dt also return MPM_ERR_INVALID, before anything is
 * enqueued, for a dt above
 *   mpm_weave_max_stable_dt = 2 / sqrt( max_i (1 / m_i) sum_{faces f around i} vol_f kmax_f |g_i| (|g_0| + |g_1| + |g_2|) ),
 * g_j the columns of the face's grad_N, m_i the vertex particle's mass as of the call, kmax the larger of 2G and the
 * larger eigenvalue of [[ka, kab], [kab, kb]]: Gershgorin's bound at the REST shape.  It is a guard, not a guarantee
 * (a stretched cloth is stiffer: F2 enters twice, and the geometric stiffness F2 -> F2 S is not in it), and how
 * conservative it is has not been measured.  +inf while the feature is off.
 * Refused with MPM_ERR_INVALID, nothing changed: a constant that is negative or not finite; D <= 0; E_warp = 0 with
 * nu != 0; a wrong count; a call before mpm_finalize; a perpendicular or zero direction (above); any partitioned or
 * multi-rank engine -- this call on such an engine, and mpm_dist_init, the halo, chain, team and world substeps on an
 * engine with the weave on. */
typedef struct mpm_cloth_weave {
    float E_warp, E_weft, nu, G;   /* Pa, Pa, -, Pa */
    float warp_dir[3];             /* rest-space direction of the warp; its length does not matter */
} mpm_cloth_weave_t;
MPM_API int mpm_set_weave(mpm_handle_t h, size_t n_cloths, const mpm_cloth_weave_t *w, const float *face_dirs);
/* The constants in force: min(mpm_cloth_count, capacity) entries into out (zeros while off), the cloth count into *n_out. */
MPM_API int mpm_get_weave(mpm_handle_t h, mpm_cloth_weave_t *out, size_t capacity, size_t *n_out);
/* The axis table in force: cs_out[2 * n_faces] = (c, s) per face in the face numbering of mpm_dump_cpu_state; (0, 0)
 * on the faces of a cloth without weave and everywhere while the feature is off. */
MPM_API int mpm_weave_axes(mpm_handle_t h, float *cs_out);
/* The weave's force on the current positions: f_out[3 * n_verts], in the vertex numbering of mpm_dump_cpu_state (zeros
 * for the vertices of cloths without weave); rec_out (NULL, or [9 * n_faces]): every face's corner records G_rec
 * ([corner][component]; the force on a corner is -G_rec).  The device function of the substep's kernel; a vertex's
 * records are summed on the host in ascending face id, as the vertex-force kernel sums them.  Changes no state. */
MPM_API int mpm_weave_forces(mpm_handle_t h, float *f_out, float *rec_out);
/* out[3 * n_faces] = Eaa, Ebb, Eab per face, the floats the kernel forms (zeros on a cloth without weave). */
MPM_API int mpm_weave_strain(mpm_handle_t h, float *out);
/* Sum over the cloth's faces of the float vol Psi the kernel's face function forms, added in double in face order in a
 * fixed tree, without atomics: the same bits whatever the particle order and the determinism mode.  min(cloth count,
 * capacity) entries into per_cloth, the cloth count into *n_out, the sum of the rows in cloth order into *total (each
 * may be NULL).  Zeros while the feature is off. */
MPM_API int mpm_weave_energy(mpm_handle_t h, double *per_cloth, size_t capacity, size_t *n_out, double *total);
MPM_API int mpm_weave_max_stable_dt(mpm_handle_t h, float *dt_out);
/* The kernel's face function on the host (no handle, no device), face by face: dminv3[3 n] = (Dm0, Dm1, Dm3) of
 * Dm^-1 = [Dm0 Dm1; 0 Dm3], vol[n], coef4[4 n] = (ka, kb, kab, 2G), cs2[2 n] = (c, s), x9[9 n] the corners' positions
 * ([corner][component]); rec9_out[9 n] the corner records, strain3_out[3 n] = Eaa, Ebb, Eab, energy_out[n] = vol Psi
 * (each output may be NULL). */
MPM_API int mpm_weave_face_records(size_t n, const float *dminv3, const float *vol, const float *coef4, const float *cs2,
                                   const float *x9, float *rec9_out, float *strain3_out, float *energy_out);
/* The axis function of mpm_set_weave on the host (no handle, no device): rest_x9[9 n] the faces' rest corners, dir3[3 n]
 * a direction per face; cs2_out[2 n] = (c, s).  A face whose direction is zero, not finite or within the 1e-3 cone of
 * its normal gets (0, 0); *first_bad_out (may be NULL) is the first such face, or -1, and the call returns
 * MPM_ERR_INVALID if there is one. */
MPM_API int mpm_weave_face_axes(size_t n, const float *rest_x9, const float *dir3, float *cs2_out, int32_t *first_bad_out);

/* ---- Tearing cloth: faces fail beyond a stretch limit, per cloth (an extension) ----
 * Every other cloth feature is elastic or viscous; this one lets the cloth open.  Per cloth one number, stretch_limit:
 * 0 (the cloth never tears) or a finite value > 1, the largest principal in-plane stretch a face survives.  Per face
 * with rest Dm^-1 = [Dm0 Dm1; 0 Dm3] and the corner positions the face kernel has just used:
 *   F2 = [x1 - x0, x2 - x0] Dm^-1,  C = F2^T F2,  m = 1/2 (C00 + C11),  q = (1/2 (C00 - C11))^2 + C01^2,
 *   lambda1 = m + sqrt(q) (the square of the largest stretch);  the face FAILS when lambda1 > L = (float)(limit^2),
 * L formed in double and rounded once, the comparison evaluated without the square root: h = L - m,
 * fails = (h < 0) || (q > h h).  Host and device run one function and agree to the bit on m, q and the verdict.
 * State: one byte per face, all zero when the feature is first switched on.  It is monotone: a substep only ever sets
 * it (a face that failed stays failed when the load goes away, and when mpm_set_tearing changes or removes the
 * limits); mpm_set_torn_faces alone clears it.
 * A torn face, from the substep in which it fails: its corner records and its normal-column stress factor are
 * overwritten with zeros at the end of the face pass, so it exerts no membrane force, no weave force
 * (mpm_set_weave), no membrane damping force (mpm_set_damping) and no stress in ParticleToGrid.  Its face particle
 * KEEPS its mass, its centroid position and velocity and the update of its deformation gradient: it still carries
 * momentum through the grid and meets colliders.  Decisions within a substep are made face by face on the positions of
 * the substep's start (Jacobi); the result does not depend on the particle order or on deterministic mode; a substep
 * that skips itself marks nothing.
 * It works with per-cloth materials, the weave, membrane damping, links, anchors, pins, force fields, grid bodies,
 * contact, fast math, deterministic mode and every substep path.  It does NOT compose with hinges or pressure: a
 * cloth with a tear limit or a torn face may not have bending stiffness > 0 (mpm_set_bending), shell bending
 * stiffness > 0 (mpm_set_shell_bending) or a pressure mode other than off (mpm_set_pressure) -- whichever call comes
 * second returns MPM_ERR_INVALID and names the other; a cloth without limit and without torn faces in the same
 * engine keeps them all -- unless mpm_set_tear_coupling (below) lifts the refusal for shell bending or for gas mode.
 * mpm_weave_forces, mpm_weave_energy and mpm_damping_forces keep reporting what those features alone would give on
 * every face, torn or not.  mpm_measure and mpm_face_strain: a torn face adds nothing to the three strain energies and
 * is left out of the stretch extremes (mpm_face_strain reports its s1, s2, r22 and 0 for its energy); its mass, momenta
 * and kinetic energies stay.
 * mpm_set_tearing needs mpm_finalize, is ordered on the engine's stream and is a synchronisation point; substeps that
 * mpm_run_substeps still owes are run first, with the old limits.  n_cloths must be mpm_cloth_count.  A table of zeros
 * switches the limits off; if no face is torn either, the tables are freed and the engine launches exactly what it
 * launches without this call.  While the tables exist the engine does not use the re-sort's quiet-time estimate.
 * Refused with MPM_ERR_INVALID, nothing changed: a limit that is not 0 and not a finite number > 1 (NaN included); a
 * wrong count; a call before mpm_finalize; the combinations above; any partitioned or multi-rank engine -- these calls
 * on such an engine, and mpm_dist_init, the halo, chain, team and world substeps on an engine whose tables exist.
 * The cost of the substep's kernel on a GPU has not been measured. */
typedef struct mpm_cloth_tear {
    float stretch_limit;   /* 0: never tears; else finite and > 1 */
    float reserved[3];     /* not read */
} mpm_cloth_tear_t;
MPM_API int mpm_set_tearing(mpm_handle_t h, size_t n_cloths, const mpm_cloth_tear_t *t);
/* The limits in force: min(mpm_cloth_count, capacity) entries into out (zeros while off), the cloth count into *n_out. */
MPM_API int mpm_get_tearing(mpm_handle_t h, mpm_cloth_tear_t *out, size_t capacity, size_t *n_out);
/* Scissors and restore: torn[n_faces], one byte per face in the face numbering of mpm_dump_cpu_state; non-zero marks
 * the face torn, zero restores it.  Replaces every flag.  Allowed while every limit is 0 (a pre-cut cloth that does
 * not tear further); an all-zero array with all limits 0 frees the tables.  A synchronisation point like
 * mpm_set_tearing. */
MPM_API int mpm_set_torn_faces(mpm_handle_t h, const uint8_t *torn);
/* The flags (torn_out[n_faces], may be NULL) and the number of torn faces per cloth, counted on the device in face
 * order: min(cloth count, capacity) entries into count_per_cloth, the cloth count into *n_out.  Zeros while off. */
MPM_API int mpm_tear_state(mpm_handle_t h, uint8_t *torn_out, uint32_t *count_per_cloth, size_t capacity, size_t *n_out);
/* The substep's face function on the current positions, state untouched: mq_out[2 * n_faces] = (m, q) per face,
 * would_fail_out[n_faces] = the verdict against the face's cloth's limit (0 on a cloth without limit); either may be
 * NULL.  Torn faces are evaluated like the others. */
MPM_API int mpm_tear_measure(mpm_handle_t h, float *mq_out, uint8_t *would_fail_out);
/* The kernel's face function on the host (no handle, no device), face by face: dminv3[3 n] = (Dm0, Dm1, Dm3), x9[9 n]
 * the corners' positions ([corner][component]), L[n] the squared limit as a float; mq_out[2 n] = (m, q),
 * fails_out[n] = (h < 0) || (q > h h) as it stands (the caller decides what L = 0 means); either output may be NULL. */
MPM_API int mpm_tear_face(size_t n, const float *dminv3, const float *x9, const float *L, float *mq_out, uint8_t *fails_out);

/* ---- Tearing composed with shell bending and gas: cut hinges, vented cloths (a mode of the engine) ----
 * Paper and foil bend, keep creases and rip; a balloon bursts.  By default a cloth that may tear can have neither
 * shell bending nor pressure (above).  mpm_set_tear_coupling switches on, per engine, the rule for where they meet:
 *   MPM_TEAR_CUTS_HINGES  shell bending (mpm_set_shell_bending, creases included) on a cloth that tears: a hinge one of
 *                         whose two faces is torn is CUT -- it carries no moment: its four corner records are +0, its psi
 *                         0, its energy term 0, mpm_shell_state counts it as inactive; it does not yield and keeps its
 *                         psibar (mpm_set_creases), so a hinge restored by mpm_set_torn_faces acts again with the psibar
 *                         it had.
 *   MPM_TEAR_VENTS_GAS    gas mode (MPM_PRESSURE_GAS) on a cloth that tears: a cloth with at least one torn face is
 *                         VENTED -- its gauge is +0.0f, its energy 0, capped 0, every pressure force an exact zero; its
 *                         volume is still reported.
 * Neither is stored: both are functions of the tear flags, evaluated in every substep and in every query
 * (mpm_shell_forces, mpm_shell_state, mpm_crease_measure, mpm_pressure_forces, mpm_pressure_state), so scissors and
 * restore work as they are and a restored cloth re-inflates by the gas law on its current volume.  The tearing kernel
 * runs last of the face kernels, the hinge and pressure kernels behind it: a face that fails in a substep cuts its hinges
 * and vents its cloth IN THAT SAME SUBSTEP, whatever the particle order and the determinism mode; a substep that skips
 * itself changes nothing.
 * NOT MODELLED: a leak rate and partial venting (one torn face empties the cloth at once; pv does not change).  Still
 * refused, whatever the mask, with the messages above: quadratic bending k > 0 (mpm_set_bending; its matrix is
 * assembled per vertex row and a hinge cannot be taken out of it -- MPM_SHELL_REST_FLAT is the same model's
 * continuation) and MPM_PRESSURE_CONSTANT on a cloth that tears.  mpm_shell_max_stable_dt is unchanged and stays a bound:
 * a row's Gershgorin sum only loses non-negative terms when hinges are cut.
 * The default is 0: every call, message and launch is that of an engine without this call, and so it is with a bit set
 * while no cloth holds the combination.  mpm_set_tear_coupling needs mpm_finalize and runs the substeps that
 * mpm_run_substeps still owes first, with the mode they were enqueued with.  Refused with MPM_ERR_INVALID, nothing
 * changed: a call before mpm_finalize; an unknown bit; a partitioned or multi-rank engine; clearing a bit while some
 * cloth holds the combination that bit permits -- a tear limit or a torn face (counted on the device) together with
 * shell k > 0 (MPM_TEAR_CUTS_HINGES) or gas mode (MPM_TEAR_VENTS_GAS); the message names the cloth and both calls. */
#define MPM_TEAR_CUTS_HINGES 1u   /* shell bending on a cloth that tears: a hinge with a torn face carries no moment */
#define MPM_TEAR_VENTS_GAS   2u   /* gas pressure on a cloth that tears: a cloth with a torn face has gauge 0 */
MPM_API int mpm_set_tear_coupling(mpm_handle_t h, uint32_t mask);
MPM_API int mpm_get_tear_coupling(mpm_handle_t h, uint32_t *mask_out);
/* per hinge of mpm_shell_hinges: 1 where the hinge is cut on the current flags (cut_out, one byte for EVERY hinge of the
 * table, may be NULL); counts per cloth: min(cloth count, capacity) entries into cut_per_cloth, the cloth count into
 * *n_out.  Zeros while MPM_TEAR_CUTS_HINGES is not set.  Changes no state. */
MPM_API int mpm_shell_cut_hinges(mpm_handle_t h, uint8_t *cut_out, uint32_t *cut_per_cloth, size_t capacity, size_t *n_out);
/* per cloth: 1 where the cloth is vented on the current flags; min(cloth count, capacity) entries, the cloth count into
 * *n_out.  Zeros while MPM_TEAR_VENTS_GAS is not set.  Changes no state. */
MPM_API int mpm_pressure_vented(mpm_handle_t h, uint8_t *vented_per_cloth, size_t capacity, size_t *n_out);
/* host only: faces A and B of every hinge of mpm_mesh_hinges, same order, cloth-local ids: min(n, capacity) pairs into
 * faces2 (may be NULL when capacity is 0), the hinge count into *n_out.  MPM_ERR_INVALID for an id out of range. */
MPM_API int mpm_mesh_hinge_faces(const int32_t *indices, size_t n_faces, size_t n_verts, int32_t *faces2, size_t capacity,
                                 size_t *n_out);

/* ---- Rest shape apart from the initial pose: pre-strained and re-shaped cloth (an extension) ----
 * mpm_finalize takes the pose the cloths were added in as their stress-free shape.  mpm_set_rest_shape computes the rest
 * state again from other vertex positions rest_pos[3 n_verts] (the vertex numbering of mpm_dump_cpu_state, over all
 * cloths), on the particle order the engine has reached: a membrane stretched onto a frame, a garment whose flat pattern
 * differs from the pose it starts in, cloth that shrinks or grows between batches of substeps, a restart from a deformed
 * pose.  NULL restores the positions as added.
 * After the call the rest state is, bit for bit, the one mpm_finalize would have computed had the cloths been added at
 * rest_pos: Dm^-1 per face (MPM_ARR_DM_INVERSES), the face's static volume, every particle's volume -- a face's is
 * |e0 x e1| / 8 dx, a vertex's the float sum of its faces' in ascending face id -- and, in a multi-material engine, its
 * mass = volume x its cloth's density.
 * THE MASS RULE: mass follows the rest shape.  The engine has one number per face for the volume of the elastic energy
 * and the volume of the mass; a cloth pre-stretched onto a frame therefore has the mass of its rest shape (as the real
 * one has), and the fixed-point scales of ParticleToGrid are derived again from the new total.
 * Left alone: positions, velocities, C, F, torn flags and the particle order.  F's in-plane columns are rewritten by
 * the next CalcFemStateAndForce from the deformed edges and the new Dm^-1; F's normal column stays the pose's.  The
 * reports (mpm_measure, mpm_face_strain) read F as the last CalcFemStateAndForce wrote it: between this call and the
 * next substep they still show the strain against the OLD rest shape (the masses are the new ones at once).
 * Features set AFTERWARDS derive from the rest shape, not from the pose: the cotangent weights of mpm_set_bending, the
 * default shape of mpm_set_shell_bending (its own rest_pos still overrides per cloth), the winding check of a gas
 * pressure, the axes of mpm_set_weave (mpm_weave_axes), and every stability limit, which reads the new Dm^-1, volumes
 * and masses.
 * THE ORDERING RULE: the call needs mpm_finalize; substeps that mpm_run_substeps still owes are run first, with the old
 * rest state; it is ordered on the engine's stream and is a synchronisation point.  Time-dependent rest shapes are set
 * between batches, like time-dependent force fields.
 * Refused with MPM_ERR_INVALID, the previous rest state staying in force to the bit (the first three are decided on the
 * host, in double, before anything is enqueued):
 *   - a coordinate that is not finite;
 *   - a face whose first rest edge e0 = x1 - x0 or whose rest area |e0 x e1| is zero (mpm_rest_shape_check names the
 *     first; there is no conditioning threshold, as mpm_finalize has none);
 *   - a partitioned or multi-rank engine; and mpm_dist_init, the chain, team and world set-up and substeps on an engine
 *     whose rest shape is set (NULL clears that; the halo substeps of a single engine run on whatever rest state it holds);
 *   - a table in force whose host side holds values derived from the rest positions, Dm^-1, the volumes or the masses:
 *     mpm_set_bending (weights, limit), mpm_set_shell_bending (cbar, psibar, limit), mpm_set_weave (axes, limit),
 *     mpm_set_damping (row sums, masses, limit), mpm_set_pressure (with a cloth not off: the rest volume's sign),
 *     mpm_set_links (limit from the masses; its break limits go with it), mpm_set_anchors (limit from the masses),
 *     mpm_set_pins (the bodies' impulse sums are kept in the fixed-point scale of the total mass).  The caller clears
 *     such a table, sets the rest shape and sets the table again.
 *   Per-cloth materials, mpm_set_force_fields, mpm_set_tearing / mpm_set_torn_faces, grid colliders and bodies and
 *   contact materials hold nothing of the kind and are accepted. */
MPM_API int mpm_set_rest_shape(mpm_handle_t h, const float *rest_pos /* [3 n_verts], vertex numbering of mpm_dump_cpu_state; NULL = the positions as added */);
/* The rest shape in force into rest_pos_out[3 n_verts] (may be NULL): the positions as added until mpm_set_rest_shape;
 * *is_set_out (may be NULL) = 1 while a rest shape given by the caller is in force.  Needs mpm_finalize; no device work. */
MPM_API int mpm_get_rest_shape(mpm_handle_t h, float *rest_pos_out /* [3 n_verts] */, int *is_set_out);
/* Host only, no handle, no device: what mpm_set_rest_shape checks.  *first_bad_face_out (may be NULL) = the first face
 * whose first edge or area, formed in double from the float positions, is zero or not finite, or -1; MPM_ERR_INVALID if
 * there is one, if an index is out of range or if a coordinate is not finite. */
MPM_API int mpm_rest_shape_check(const float *rest_pos, size_t n_verts, const int32_t *indices, size_t n_faces, int32_t *first_bad_face_out);

/* ---- Links between cloth vertices: seams, springs and tension-only cords (an extension) ----
 * Every mpm_add_qr_cloth* call makes an island; pins are hard constraints to rigid bodies only.  A link joins two
 * distinct cloth vertices a, b -- of one cloth or of two -- by a damped spring: panels sewn into a garment, a sheet laced
 * to another, a banner hung by cords, a tether that stops a flap at a length.  Ids are in the vertex numbering of
 * mpm_dump_cpu_state, over all cloths.  With d = x_b - x_a and w = v_b - v_a, in float, the force on a is
 *   seam   (rest_length L == 0)  f_j = fma(k, d_j, c w_j): linear and isotropic, no square root, no singular configuration
 *   spring (L > 0)               l2 = fma(d2, d2, fma(d1, d1, d0 d0)), l = sqrt(l2), s = fma(w2, d2, fma(w1, d1, w0 d0)) / l,
 *                                t = fma(c, s, k (l - L)), g = t / l, f_j = g d_j; nothing where l2 < 1e-30
 *   MPM_LINK_TENSION_ONLY        nothing unless l > L (a cord): the elastic and the damping part are gated together
 * and the force on b is its negative -- bit for bit: every intermediate is even or odd in (d, w), the square root and
 * both divisions are correctly rounded whatever mpm_set_fast_math says, no product is contracted.  A vertex's links are
 * added in link order by one lane, without atomics: the result is the same bits whatever the particle order, and the
 * links' total force is zero within the rounding of those additions.  Duplicate pairs are allowed; each is a link of
 * its own.  Elastic energy of a link that acts: 1/2 k (l - L)^2.  A seam of n stitches that should act as one spring of
 * stiffness K takes k = K / n per link.
 * The force joins the vertex forces of CalcFemStateAndForce (MPM_ARR_FORCES includes it; its kernel runs behind the
 * vertex-force, bending and bending-damping kernels and counts under MPM_PHASE_VFORCE).  It works with pins, per-cloth
 * materials, grid bodies, force fields, bending, damping, deterministic mode, fast math and the coupled path.
 * mpm_set_links replaces the table (n = 0 clears it, links may then be NULL); it needs mpm_finalize, is ordered on the
 * engine's stream and is a synchronisation point; substeps that mpm_run_substeps still owes are run first, with the
 * table they were enqueued with.  With an empty table the engine launches exactly what it launches without this call.
 * While links are set the engine does not use the re-sort's quiet-time estimate to omit re-sort check launches, and
 * every batched substep launches the vertex-force kernel.
 * Stability: symplectic Euler on a damped oscillator, v' = v + dt (-W x - G v), x' = x + dt v', is stable iff
 * W dt^2 + 2 G dt <= 4.  With Gershgorin's bounds on the lumped system, W = max_i (2 / m_i) sum_j k_ij and
 * G = max_i (2 / m_i) sum_j c_ij over vertex i's links, m_i the vertex particle's mass as of mpm_set_links,
 * mpm_links_max_stable_dt is the positive root of that quadratic (2 / G where W = 0), and the entry points that check
 * mpm_bending_max_stable_dt also return MPM_ERR_INVALID, before anything is enqueued, for a dt above it.  A guard, not a
 * guarantee: a compressed spring with L > 0 has a transverse (geometric) stiffness k (L - l) / l that the bound does
 * not cover, and the grid shares a vertex's impulse with the faces around it.  +inf while the table is empty.
 * Refused with MPM_ERR_INVALID, the previous table staying in force and nothing enqueued: a call before mpm_finalize; a
 * or b >= the vertex count; a == b; a stiffness, rest_length or damping that is negative or not finite; unknown flags; a
 * table that does not fit 2^31 records; any partitioned or multi-rank engine -- this call on such an engine, and
 * mpm_dist_init, the halo, chain, team and world substeps on an engine with links. */
#define MPM_LINK_TENSION_ONLY 1u   /* acts only while length > rest_length (a cord) */
typedef struct mpm_link {
    uint32_t a, b;       /* the two vertices, distinct */
    float stiffness;     /* k, N/m,   >= 0 */
    float rest_length;   /* L, m,     >= 0; 0 is a seam */
    float damping;       /* c, N s/m, >= 0 */
    uint32_t flags;      /* MPM_LINK_TENSION_ONLY */
} mpm_link_t;
MPM_API int mpm_set_links(mpm_handle_t h, size_t n, const mpm_link_t *links);
/* The table as given: min(n, capacity) entries into out (may be NULL when capacity is 0), n into *n_out. */
MPM_API int mpm_get_links(mpm_handle_t h, mpm_link_t *out, size_t capacity, size_t *n_out);
/* The links' force on the current positions and velocities: f_out[3 * n_verts], in the vertex numbering of
 * mpm_dump_cpu_state (zeros for vertices without a link).  The device function of the substep's kernel; changes no state. */
MPM_API int mpm_link_forces(mpm_handle_t h, float *f_out);
/* Sum of 1/2 k (l - L)^2 over the links that act (the gates above, decided on the float differences), every term formed
 * in double from the float positions on the device, the terms added in link order, without atomics: the same bits
 * whatever the particle order.  length_out (n links, may be NULL): every link's length, acting or not, formed in double and rounded to float once.  This
 * energy is not part of mpm_measure's record.  Changes no state. */
MPM_API int mpm_link_energy(mpm_handle_t h, double *energy_out, float *length_out);
MPM_API int mpm_links_max_stable_dt(mpm_handle_t h, float *dt_out);
/* The force of one link on its end a, on the host (no handle, no device): the inline function the link kernel calls,
 * compiled for the host.  xa, xb, va, vb, f_on_a: 3 floats each.  The link is not validated (a and b are not read). */
MPM_API int mpm_link_force(const mpm_link_t *link, const float xa[3], const float xb[3], const float va[3], const float vb[3],
                           float f_on_a[3]);

/* ---- Breakable links: seams rip and cords snap beyond a length (an extension) ----
 * Tearing lets the fabric open; this lets what holds it together fail.  Each link i of the table in force may carry a
 * break_length b_i: 0 (the link never breaks) or a finite value > rest_length (for a seam: > 0).  The host forms
 * B2_i = (float)((double)b_i (double)b_i), rounded once.  With d = x_b - x_a in float and the l2 of the link's force law,
 *   l2 = fma(d2, d2, fma(d1, d1, d0 d0)),  the link BREAKS when l2 > B2_i
 * -- no square root; false for a NaN position; even in d, and formed once per link, not per end.  Host and device run one
 * function and agree to the bit on l2 and the verdict.  l2 is within 6 x 2^-24 l2 of the exact value on the float
 * positions.
 * State: one byte per link in link order, all zero when limits or flags are first set.  It is monotone: a substep only
 * ever sets it (a link that broke stays broken when the load goes away, and when mpm_set_link_limits changes or removes
 * the limits); mpm_set_broken_links alone clears it.  mpm_set_links replaces the table, and the limits and flags go with
 * the table they belonged to: the new table starts with no limits and no flags.
 * A broken link does not act, from the substep in which it breaks: the elastic and the damping part, every kind of link
 * (seam, spring, tension-only), both ends.  Decisions within a substep are made link by link on the positions of the
 * substep's start, the positions the link kernel reads (Jacobi); the result does not depend on the other links'
 * decisions, the particle order or deterministic mode; a substep that skips itself marks nothing.  The kernel runs
 * immediately in front of the link kernel, one lane per link, and counts under MPM_PHASE_VFORCE.
 * mpm_link_forces and mpm_link_energy report what the substep applies: a broken link adds nothing to the forces, its
 * energy term is 0, length_out still reports its length.  mpm_get_links keeps returning the table as given.
 * mpm_links_max_stable_dt does NOT change when links break: it is formed over the whole table, and breaking only removes
 * non-negative terms from its row sums, so it stays a valid, more conservative, guard.
 * It works with everything links work with: tearing, pins, anchors, both bending models, pressure, damping, the weave,
 * force fields, grid bodies, contact, fast math, deterministic mode and every non-partitioned substep path.  Anchors
 * (mpm_set_anchors) do not break yet.
 * Both setters need mpm_finalize, are ordered on the engine's stream and are synchronisation points; substeps that
 * mpm_run_substeps still owes are run first, with the old limits.  The tables exist while some limit is > 0 or some flag
 * is set; otherwise they are freed and the engine launches exactly what it launches without these calls.
 * Refused with MPM_ERR_INVALID, nothing changed: a call before mpm_finalize; n different from the link count (0 allowed
 * for the limits); a limit that is negative, NaN, infinite, non-zero and <= rest_length, or whose square is not a finite
 * float (or is 0 for a non-zero limit) -- the message names the link; a null array with n > 0; any partitioned or
 * multi-rank engine.
 * The cost of the substep's kernel on an MI355X: 5.2 us per substep at 168,200 links with limits on and none broken; a
 * substep in which many links break has not been measured. */
/* n == the link count: one break_length per link; n == 0 (break_length may be NULL): all limits off */
MPM_API int mpm_set_link_limits(mpm_handle_t h, size_t n, const float *break_length);
/* The limits in force: min(link count, capacity) entries into out (zeros while off), the link count into *n_out. */
MPM_API int mpm_get_link_limits(mpm_handle_t h, float *out, size_t capacity, size_t *n_out);
/* Scissors and restore: broken[n], n the link count, one byte per link in link order; non-zero breaks the link, zero
 * restores it.  Replaces every flag.  Allowed while every limit is 0 (a cord cut by hand); an all-zero array with all
 * limits 0 frees the tables. */
MPM_API int mpm_set_broken_links(mpm_handle_t h, size_t n, const uint8_t *broken);
/* The flags (broken_out[link count], may be NULL) and the number of broken links (count_out, may be NULL), counted on the
 * device in link order in a fixed tree.  Zeros while the tables do not exist. */
MPM_API int mpm_link_break_state(mpm_handle_t h, uint8_t *broken_out, uint32_t *count_out);
/* The substep's link function on the current positions, state untouched: l2_out[link count], would_break_out[link count]
 * = the verdict against the link's limit (0 for a link without a limit, and while the tables do not exist); either may be
 * NULL.  Broken links are evaluated like the others. */
MPM_API int mpm_link_break_measure(mpm_handle_t h, float *l2_out, uint8_t *would_break_out);
/* The kernel's link function on the host (no handle, no device), link by link: xa3[3 n], xb3[3 n] the ends' positions,
 * B2[n] the squared limit as a float; l2_out[n], breaks_out[n] = (l2 > B2) as it stands (the caller decides what B2 = 0
 * means); either output may be NULL. */
MPM_API int mpm_link_breaks(size_t n, const float *xa3, const float *xb3, const float *B2, float *l2_out, uint8_t *breaks_out);

/* ---- Anchors: springs and cords from cloth vertices to rigid bodies (an extension) ----
 * A pin holds a vertex to a body rigidly; a link joins two cloth vertices compliantly.  An anchor is the compliant
 * attachment to a body: a banner hung from a moving pole by cords, a parachute's lines to its payload, a tarp lashed to a
 * truck bed, a sheet in a compliant clip, a tether that stops a flap at a length.  The body feels the tension.
 * The attachment point.  Let t be the body's clock as it stands when CalcFemStateAndForce runs, that is at the start of
 * the substep -- the clock of the pins, which mpm_set_body_motions restarts and which advances at the end of every
 * GridToParticle that runs.  With p(t) = p_WB + t v and R(t) = Rodrigues(t w) R_WB,
 *   y = p(t) + R(t) p_BQ;   v_Q = v + w x (y - p(t)),
 * formed in double as the pins' kernel forms them and rounded to float once each (y32, v_Q32).
 * The force on the vertex is the law of a link (above), evaluated by the same inline function with d = y32 - x and
 * w = v_Q32 - v_vertex: L == 0 is a zero-length spring (the seam law), L > 0 a spring, MPM_ANCHOR_TENSION_ONLY a cord;
 * the 1e-30 gate, the correctly rounded square root and divisions and the disabled contraction are those of a link.  A
 * vertex's anchors are added in anchor order by one lane, without atomics: vertex forces are the same bits whatever the
 * particle order.  The force joins the vertex forces of CalcFemStateAndForce behind the shell-bending kernels
 * (MPM_ARR_FORCES includes it; its time counts under MPM_PHASE_VFORCE).
 * The reaction.  With dt the substep's length, body `body` receives the force impulse l = -(double)f (double)dt and the
 * torque impulse (y32 - p_WB) x l about the p_WB of its motion as set -- the convention of pins, so that one body's
 * accumulator means one thing --, in the accumulators of the contact impulses (64-bit fixed point: the sums do not depend
 * on the order; an overflow raises the range error as it does for pins) read by mpm_external_body_force_to_host and
 * mpm_finalize_external_contact_forces.  An anchor whose body is >= the mpm_reallocate_external_bodies count acts on the
 * vertex and adds no impulse.
 * Exactly once.  A substep that skips itself and is run again adds neither force nor impulse.  Every
 * CalcFemStateAndForce that does run adds the impulse: a caller of the phase-by-phase mpm_calc_fem_state_and_force who
 * calls it twice for one substep has added it twice.
 * Clocks.  An engine with anchors and no pins advances the clocks at the end of every GridToParticle that runs, exactly
 * as one with pins does; an engine with both advances them once.
 * While anchors are set the engine does not use the re-sort's quiet-time estimate to omit re-sort check launches, and
 * every batched substep launches the vertex-force kernel.  With an empty table the engine launches exactly what it
 * launches without this call.
 * mpm_set_anchors replaces the table (n = 0 clears it, anchors may then be NULL); it needs mpm_finalize, is ordered on
 * the engine's stream and is a synchronisation point; substeps that mpm_run_substeps still owes are run first, with the
 * table they were enqueued with.  Duplicate (vertex, body) pairs are allowed; each is an anchor of its own: n anchors
 * meant to act as one spring of stiffness K take K / n each.  A pinned vertex may also carry anchors.
 * Motions may be set after anchors; a substep entry point (mpm_calc_fem_state_and_force included) called while some
 * anchor's body has no motion is refused as it is for pins, and so are mpm_anchor_forces and mpm_anchor_state.
 * Stability: the body's end is prescribed, so the factor is 1 where a link has 2: W = max_i (1 / m_i) sum k and
 * G = max_i (1 / m_i) sum c over vertex i's anchors, m_i the vertex particle's mass as of mpm_set_anchors;
 * mpm_anchors_max_stable_dt is the positive root of W dt^2 + 2 G dt = 4 (+inf while the table is empty), and the entry
 * points that check mpm_links_max_stable_dt also return MPM_ERR_INVALID, before anything is enqueued, for a dt above it.
 * This is a separate guard, not a guarantee: a vertex with links and anchors passes each guard on its own, and the bound
 * does not cover the geometric stiffness of a compressed spring.
 * It works with pins, per-cloth materials, grid bodies, force fields, bending, damping, links, pressure, shell bending,
 * deterministic mode, fast math and the coupled path.
 * Refused with MPM_ERR_INVALID, the previous table staying in force and nothing enqueued: a call before mpm_finalize; a
 * vertex >= the vertex count; a non-finite p_BQ; a stiffness, rest_length or damping that is negative or not finite;
 * unknown flags; a table that does not fit 2^31 records; any partitioned or multi-rank engine -- this call on such an
 * engine, and mpm_dist_init, the halo, chain, team and world substeps on an engine with anchors. */
#define MPM_ANCHOR_TENSION_ONLY 1u        /* acts only while length > rest_length (a cord) */
typedef struct mpm_anchor {
    uint32_t vertex;      /* vertex numbering of mpm_dump_cpu_state, over all cloths */
    uint32_t body;        /* as mpm_pin_t::body: motion of that body, accumulator of that body */
    float p_BQ[3];        /* attachment point in the body frame */
    float stiffness;      /* k, N/m,   >= 0 */
    float rest_length;    /* L, m,     >= 0; 0: a zero-length spring (the seam law) */
    float damping;        /* c, N s/m, >= 0 */
    uint32_t flags;       /* MPM_ANCHOR_TENSION_ONLY */
} mpm_anchor_t;           /* 36 bytes */
MPM_API int mpm_set_anchors(mpm_handle_t h, size_t n, const mpm_anchor_t *anchors);
/* The table as given: min(n, capacity) entries into out (may be NULL when capacity is 0), n into *n_out. */
MPM_API int mpm_get_anchors(mpm_handle_t h, mpm_anchor_t *out, size_t capacity, size_t *n_out);
/* The anchors' force on the current state at the bodies' current clocks: f_out[3 * n_verts], in the vertex numbering of
 * mpm_dump_cpu_state (zeros for vertices without an anchor).  The device function of the substep's kernel; changes no
 * state and adds no impulse. */
MPM_API int mpm_anchor_forces(mpm_handle_t h, float *f_out);
/* On the current state at the bodies' current clocks; any output may be NULL; changes no state.
 * energy_out: the sum of 1/2 k (l - L)^2 over the anchors that act (the link's gates, decided on the float differences),
 * every term formed in double from the floats y32 and x, added in anchor order without atomics.  length_out (n): every
 * anchor's length, acting or not, formed in double and rounded to float once.  point_out (3 n): every anchor's y32.
 * impulse_quantum_out: one double, the quantum of the bodies' accumulators -- every impulse is rounded to a multiple of
 * it before it is added, which states the rounding of a reaction sum.  This energy is not part of mpm_measure's record. */
MPM_API int mpm_anchor_state(mpm_handle_t h, double *energy_out, float *length_out, float *point_out, double *impulse_quantum_out);
MPM_API int mpm_anchors_max_stable_dt(mpm_handle_t h, float *dt_out);
/* The attachment point on the host (no handle, no device): the pose function of the pins' and anchors' kernels and the
 * two formulas above, compiled for the host, at clock t.  y, v_Q: 3 floats each, either may be NULL.  The motion is not
 * validated.  sin and cos are each platform's own, so host and device agree within one float ulp of the components'
 * scale, not to the bit.  The force of an anchor on its vertex is mpm_link_force with xb = y, vb = v_Q. */
MPM_API int mpm_anchor_point(const mpm_body_motion_t *motion, double t, const float p_BQ[3], float y[3], float v_Q[3]);

/* ---- Enclosed-volume pressure per cloth: inflatable cloths (an extension) ----
 * Every other force on the cloth is local: none knows that a cloth can enclose something, so a ball, a cushion, an
 * airbag or a balloon in a gripper has no load that keeps it from collapsing.  mpm_set_pressure gives every cloth a
 * gauge pressure g that pushes each face along its winding normal (a force field, mpm_set_force_fields, pushes along a
 * fixed direction and cannot depend on a volume).  One mpm_cloth_pressure_t per cloth, in the order of the
 * mpm_add_qr_cloth* calls:
 *   MPM_PRESSURE_OFF       nothing (the other fields are not read beyond the finiteness check)
 *   MPM_PRESSURE_CONSTANT  g = p: any finite value, either sign; the mesh may be open -- a follower load of p per unit
 *                          of CURRENT area along each face's winding normal
 *   MPM_PRESSURE_GAS       an isothermal gas in a closed cloth: pv > 0 (the product p V of the enclosed gas),
 *                          p_ambient >= 0, p_max > p_ambient.  With V the cloth's current signed volume,
 *                          g = min(pv / V, p_max) - p_ambient where V > 0, and g = p_max - p_ambient otherwise, formed
 *                          in double and rounded to float once: never a NaN or an infinity.  A collapsed or inverted
 *                          cloth gets the capped pressure, and mpm_pressure_state says so.
 * Volume: V = 1/6 sum_faces x_a . (x_b x x_c), every term formed in double from the float positions, summed in id order
 * in a fixed tree.  Force on vertex i: every face around it, rotated cyclically to read (i, b, c), in ascending face id,
 *   f_i = (g / 6) sum (x_b - x_i) x (x_c - x_i)
 * in float, every operation written out, no contraction, the one multiplication by g / 6 last.  Differences only: the
 * force is translation invariant to the bit.  On an interior vertex of a closed, consistently wound mesh it is exactly
 * g dV/dx_i, so the force is conservative: E = -p V (constant), E = -pv ln V + p_ambient V (gas, while not capped).
 * Orientation: positive g pushes along the winding normal; gas mode requires V > 0 on the rest shape (reverse the winding
 * otherwise).  One lane per vertex adds its faces in a fixed order, without atomics: V, g and the forces are the same
 * bits whatever the particle order.
 * The force joins the vertex forces of CalcFemStateAndForce (MPM_ARR_FORCES includes it; its kernels run behind the
 * vertex-force, bending, bending-damping and link kernels and count under MPM_PHASE_VFORCE; the volume is reduced on the
 * device inside the substep, a batch of mpm_run_substeps stays device resident).  It works with pins, per-cloth
 * materials, grid bodies, force fields, bending, damping, links, deterministic mode, fast math and the coupled path.
 * NO dt GUARD: the gas's stiffness (pv / V^2) grad V grad V^T + a geometric term depends on the state and is unbounded
 * as V -> 0 below the cap; a limit computed at the rest shape would promise something it cannot keep.  Watch V and g
 * through mpm_pressure_state and choose dt accordingly.
 * mpm_set_pressure replaces the table (n_cloths = 0 turns pressure off, the table may then be NULL; otherwise n_cloths
 * must equal mpm_cloth_count); it needs mpm_finalize, is ordered on the engine's stream and is a synchronisation point;
 * substeps that mpm_run_substeps still owes are run first, with the table they were enqueued with.  With pressure off
 * the engine launches exactly what it launches without this call.  While pressure is set the engine does not use the
 * re-sort's quiet-time estimate, and every batched substep launches the vertex-force kernel.
 * Refused with MPM_ERR_INVALID, the previous table staying in force and nothing enqueued: a call before mpm_finalize; a
 * wrong n_cloths; a number that is not finite; an unknown mode; gas parameters outside the ranges above; gas on a mesh
 * that is not closed and consistently wound (the message names the cloth and the first offending edge, vertex ids in
 * the numbering of mpm_dump_cpu_state); gas on a rest volume <= 0; a table that does not fit 2^31 records; any
 * partitioned or multi-rank engine -- this call on such an engine, and mpm_dist_init, the halo, chain, team and world
 * substeps on an engine with pressure; a mode other than off on a cloth with a tear limit or a torn face
 * (mpm_set_tearing), unless mpm_set_tear_coupling with MPM_TEAR_VENTS_GAS permits gas mode there. */
#define MPM_PRESSURE_OFF 0u
#define MPM_PRESSURE_CONSTANT 1u
#define MPM_PRESSURE_GAS 2u
typedef struct mpm_cloth_pressure {
    uint32_t mode;     /* MPM_PRESSURE_* */
    float p;           /* constant: the gauge pressure, Pa */
    float pv;          /* gas: p V of the enclosed gas, J, > 0 */
    float p_ambient;   /* gas: Pa, >= 0 */
    float p_max;       /* gas: the cap on the absolute pressure, Pa, > p_ambient */
} mpm_cloth_pressure_t;
typedef struct mpm_cloth_pressure_state {
    double volume;     /* V, signed; reported for every cloth, pressurised or not, closed or not */
    double energy;     /* -p V (constant), -pv ln V + p_ambient V (gas); 0 for an unpressurised cloth and while capped */
    float gauge;       /* g; 0 for an unpressurised cloth */
    uint32_t capped;   /* gas: V <= 0 or pv / V >= p_max */
} mpm_cloth_pressure_state_t;
MPM_API int mpm_set_pressure(mpm_handle_t h, size_t n_cloths, const mpm_cloth_pressure_t *per_cloth);
/* The table as given: min(n, capacity) entries into out (may be NULL when capacity is 0), the cloth count into *n_out.
 * Zeros (MPM_PRESSURE_OFF) while pressure is off. */
MPM_API int mpm_get_pressure(mpm_handle_t h, mpm_cloth_pressure_t *out, size_t capacity, size_t *n_out);
/* The pressure force on the current positions: f_out[3 * n_verts], in the vertex numbering of mpm_dump_cpu_state (zeros
 * for the vertices of unpressurised cloths).  V and g are formed anew from the current positions, never taken from
 * what the last substep left.  The device function of the substep's kernel; changes no state. */
MPM_API int mpm_pressure_forces(mpm_handle_t h, float *f_out);
/* Volume, energy, gauge pressure and cap of every cloth on the current positions: min(n, capacity) entries into out,
 * the cloth count into *n_out.  Needs mpm_finalize; works with pressure off (volumes alone); refused on a partitioned
 * or multi-rank engine (the volume would need a rank-ordered sum across the cut).  Changes no state. */
MPM_API int mpm_pressure_state(mpm_handle_t h, mpm_cloth_pressure_state_t *out, size_t capacity, size_t *n_out);
/* Host only (no handle, no device): the check mpm_set_pressure applies to a cloth in gas mode.  indices: 3 * n_faces
 * vertex ids in [0, n_verts).  Returns 1 when every directed edge a -> b of the faces occurs exactly once and its
 * reverse b -> a exactly once (closed and consistently wound), 0 otherwise with the first offending directed edge, in
 * face order, in edge_out (may be NULL); MPM_ERR_INVALID for an id out of range. */
MPM_API int mpm_mesh_is_closed(const int32_t *indices, size_t n_faces, size_t n_verts, int32_t edge_out[2]);
/* Host only: the inline row function the pressure kernel calls, compiled for the host.  x_own: the vertex, x_b, x_c:
 * 3 * n floats, entry e's corners b and c; f_out = (g / 6) sum_e (x_b - x_own) x (x_c - x_own), added in order. */
MPM_API int mpm_pressure_vertex_force(float g, const float x_own[3], size_t n, const float *x_b, const float *x_c,
                                      float f_out[3]);

/* ---- Shell bending about a curved rest shape: the hinge-angle model (an extension) ----
 * mpm_set_bending's quadratic model is defined for a rest shape that is flat per hinge: it pulls a ball, a sleeve or a
 * pre-formed cup towards a flat sheet and its energy is not zero on the shape the caller built.  mpm_set_shell_bending
 * bends about the rest shape's own dihedral angles (discrete shells), in the variable psi = 2 sin(theta / 2).
 * Hinges are exactly those of mpm_set_bending: every edge shared by exactly two faces of one cloth; boundary edges and
 * edges with more than two faces form none.  A hinge is (x0, x1 | x2, x3): x0 -> x1 is the edge as face A, the face
 * with the lower id, runs it; x2 is opposite the edge in face A, x3 in face B.  The hinges of the cloths with k > 0 are
 * numbered in ascending (cloth, min(v0, v1), max(v0, v1)).  All quantities are differences against x0:
 *   e = x1 - x0,  a = x2 - x0,  b = x3 - x0,   nA = e x a,  nB = b x e             (parallel on a flat hinge)
 *   nAh = nA / |nA|,  nBh = nB / |nB|,  sigma = +1 where e . (nA x nB) >= 0, else -1
 *   psi  = sigma |nAh - nBh| = 2 sin(theta / 2),   theta the signed dihedral angle, 0 on a flat hinge
 *   dpsi = 1/2 |nAh + nBh|   = cos(theta / 2)
 *   E_h  = 1/2 k cbar (psi - psibar)^2,   cbar = 3 |ebar|^2 / (Abar_A + Abar_B)   (rest edge length and rest areas)
 *   f_j  = -k cbar (psi - psibar) dpsi G_j,   G_j = grad_{x_j} theta,   G2 = -|e| nA / |nA|^2,  G3 = -|e| nB / |nB|^2,
 *          G1 = -(wA G2 + wB G3),  G0 = -((1 - wA) G2 + (1 - wB) G3),   wA = a . e / |e|^2,  wB = b . e / |e|^2
 * in float, every operation written out, no contraction, no trigonometric function; the square roots and divisions are
 * correctly rounded whatever mpm_set_fast_math says.  Differences only: the force is translation invariant to the bit.
 * k is in N m and means what mpm_set_bending's k means: with psibar = 0 the energy of a hinge whose two triangles move
 * rigidly equals the quadratic model's, so this model is its rotation-invariant continuation to curved rest shapes.
 * It is bounded (no infinite force).  ITS WEAKNESS: dpsi -> 0 as |theta| -> pi, so a hinge folded flat onto itself
 * feels no restoring force, and psi jumps from 2 to -2 there: the energy is discontinuous for psibar != 0 while the
 * force is continuous.
 * The rest shape: per cloth, MPM_SHELL_REST_SHAPE takes psibar and cbar from rest_pos (3 * n_verts floats in the vertex
 * numbering of mpm_dump_cpu_state; only the cloth's own vertices are read) where rest_pos is given, else from the mesh
 * as added; MPM_SHELL_REST_FLAT sets psibar = 0 and takes cbar from the mesh as added.  psibar is not computed on the
 * host: the call runs the hinge function on the device once on the rest positions and keeps the psi it wrote, so on
 * those positions psi - psibar is an exact zero and every vertex force is +-0: the rest shape is an exact equilibrium.
 * cbar is formed in double on the host and k cbar rounded to float once.  A hinge acts only while |e|^2, |nA|^2 and
 * |nB|^2 are all >= 1e-30; otherwise its records are exact zeros and it counts as inactive: never a NaN or an infinity.
 * The force joins the vertex forces of CalcFemStateAndForce (MPM_ARR_FORCES includes it): two kernels behind the
 * vertex-force, bending, link and pressure kernels, counted under MPM_PHASE_VFORCE -- one lane per hinge writes the four
 * corner records, one lane per vertex adds its records in ascending hinge id, no atomics: records, psi and forces are
 * the same bits whatever the particle order.  A cloth may have mpm_set_bending and this on: the forces add.
 * Stiffness-proportional damping of these hinges is mpm_set_shell_damping (below); mpm_set_damping's bending part acts
 * on the quadratic model only.  It works with pins, per-cloth materials, grid bodies, force fields, bending, damping, links, pressure,
 * deterministic mode, fast math and the coupled path.
 * STABILITY GUARD: the substep entry points that check mpm_bending_max_stable_dt refuse, before anything is enqueued,
 *   dt > mpm_shell_max_stable_dt = 2 / sqrt(max_i (1 / m_i) sum_{h contains i} k cbar dpsibar^2 |Gbar_hi| sum_j |Gbar_hj|)
 * (Gershgorin on the Gauss-Newton part of the stiffness).  It is a guard AT THE REST SHAPE: it does not cover the
 * geometric stiffness of a deformed hinge, nor the larger |G| of a hinge whose triangles have collapsed.  How
 * conservative it is has not been measured.  +inf while the feature is off.  mpm_set_shell_damping's beta TIGHTENS this
 * guard (below).
 * mpm_set_shell_bending replaces the table (all-zero stiffness or n_cloths = 0 switches the feature off, the table may
 * then be NULL; otherwise n_cloths must equal mpm_cloth_count); it needs mpm_finalize, is ordered on the engine's stream
 * and is a synchronisation point; substeps that mpm_run_substeps still owes are run first, with the table they were
 * enqueued with.  With the feature off the engine launches exactly what it launches without this call.  While it is on
 * the engine does not use the re-sort's quiet-time estimate, and every batched substep launches the vertex-force kernel.
 * Refused with MPM_ERR_INVALID, the previous table staying in force and nothing enqueued: a call before mpm_finalize; a
 * wrong n_cloths; a negative or non-finite stiffness; an unknown rest; a non-finite rest_pos; a zero rest area or a zero
 * rest edge at a hinge of a cloth with k > 0 (the message names the face); any partitioned or multi-rank engine -- this
 * call on such an engine, and mpm_dist_init, the halo, chain, team and world substeps on an engine with it on; k > 0 on
 * a cloth with a tear limit or a torn face (mpm_set_tearing), unless mpm_set_tear_coupling with MPM_TEAR_CUTS_HINGES
 * permits it. */
#define MPM_SHELL_REST_SHAPE 0u   /* psibar from rest_pos where given, else from the mesh as added */
#define MPM_SHELL_REST_FLAT 1u    /* psibar = 0 */
typedef struct mpm_cloth_shell {
    float stiffness;   /* k in N m, >= 0; 0: the cloth has no hinge */
    uint32_t rest;     /* MPM_SHELL_REST_* */
} mpm_cloth_shell_t;
MPM_API int mpm_set_shell_bending(mpm_handle_t h, size_t n_cloths, const mpm_cloth_shell_t *per_cloth,
                                  const float *rest_pos /* [3 n_verts] or NULL */);
/* The table as given: min(n, capacity) entries into out (may be NULL when capacity is 0), the cloth count into *n_out.
 * Zeros while the feature is off. */
MPM_API int mpm_get_shell_bending(mpm_handle_t h, mpm_cloth_shell_t *out, size_t capacity, size_t *n_out);
/* The hinge table in force (the hinges of the cloths with k > 0, in hinge order): min(n, capacity) hinges into ids4
 * (4 vertex ids x0, x1, x2, x3 each, in the numbering of mpm_dump_cpu_state), kc (float(k cbar)) and psibar (what the
 * device wrote on the rest positions; 0 for MPM_SHELL_REST_FLAT); the hinge count into *n_out.  The outputs may be
 * NULL when capacity is 0. */
MPM_API int mpm_shell_hinges(mpm_handle_t h, int32_t *ids4, float *kc, float *psibar, size_t capacity, size_t *n_out);
/* The shell force on the current positions: f_out[3 * n_verts], in the vertex numbering of mpm_dump_cpu_state (zeros for
 * the vertices of cloths without it).  The device functions of the substep's kernels; changes no state. */
MPM_API int mpm_shell_forces(mpm_handle_t h, float *f_out);
/* On the current positions: energy_per_cloth[mpm_cloth_count] = sum of the hinges' float terms 1/2 kc (psi - psibar)^2,
 * as the hinge kernel forms them, added in double in hinge order (a fixed order, no atomics: the same bits whatever
 * the particle order); psi_out (one per hinge of mpm_shell_hinges, may be NULL): the hinge's psi, 0 for an inactive
 * one; inactive_out (may be NULL): how many hinges do not act.  This energy is not part of mpm_measure's record.
 * Changes no state. */
MPM_API int mpm_shell_state(mpm_handle_t h, double *energy_per_cloth, float *psi_out, uint32_t *inactive_out);
MPM_API int mpm_shell_max_stable_dt(mpm_handle_t h, float *dt_out);
/* Host only (no handle, no device): the hinges of a mesh as mpm_set_shell_bending finds them for one cloth.  indices:
 * 3 * n_faces vertex ids in [0, n_verts).  min(n, capacity) hinges into ids4 (x0, x1, x2, x3 each; may be NULL when
 * capacity is 0), the hinge count into *n_out.  MPM_ERR_INVALID for an id out of range. */
MPM_API int mpm_mesh_hinges(const int32_t *indices, size_t n_faces, size_t n_verts, int32_t *ids4, size_t capacity,
                            size_t *n_out);
/* Host only: the inline function the hinge kernel calls, compiled for the host.  x12: x0, x1, x2, x3; kc = float(k
 * cbar); rec12_out: the four corner records f_0 .. f_3; psi_out (may be NULL): the hinge's psi.  Returns 1 where the
 * hinge acts, 0 where it does not (exact zeros), a negative code on a null argument. */
MPM_API int mpm_shell_hinge(const float x12[12], float kc, float psibar, float rec12_out[12], float *psi_out);

/* ---- Hinge damping: stiffness-proportional damping of the shell hinges, per cloth (state of shell bending) ----
 * A tube, a rolled sheet or a creased fold set in motion rings until the transfer scheme happens to eat the motion:
 * mpm_set_damping covers the membrane and the quadratic hinge model, links and anchors carry their own damping, and this
 * call is the damper of the shell hinges.  Per hinge of a cloth with beta > 0 (seconds), with e, a, b, nA, nB, wA, wB,
 * dpsi and G_j of the shell block above, gA = |e| / |nA|^2, gB = |e| / |nB|^2, and the corner velocities as differences
 * against corner 0, w_j = v_j - v_0 (Galilean invariant to the bit):
 *   thetadot = sum_j G_j . v_j = -(gA nA . (w2 - wA w1) + gB nB . (w3 - wB w1))
 *   psidot   = dpsi thetadot
 *   m_d      = -(bkc psidot) dpsi,    bkc = float(beta k cbar), formed in double on the host and rounded once
 *   f_j      = (m_el + m_d) G_j,      m_el = -(k cbar (psi - psibar)) dpsi the elastic moment above
 * This is -beta times the Gauss-Newton stiffness k cbar dpsi^2 G G^T applied to the velocities: the matrix the guard
 * bounds, and the stiffness half of a Rayleigh pair, as mpm_set_damping is.  It is linear in v, an exact zero for a common
 * velocity, zero up to rounding for a rigid rotation, dissipative (-sum_j f_j . v_j = bkc psidot^2 >= 0), bounded where
 * the elastic force is bounded and gone where dpsi -> 0, like the elastic moment.  In float, every operation written out,
 * no contraction, the same function on host and device (mpm_shell_hinge_damped).  A hinge whose bkc is 0 (a cloth with
 * beta = 0 on a damped engine) gives the undamped hinge's bits.
 * NOT MODELLED: no mass-proportional part; the damping moment does not enter the crease yield rule (mpm_set_creases
 * yields on the elastic moment alone); the geometric stiffness is not damped.
 * It is STATE OF SHELL BENDING, not a feature of its own: it needs shell bending on, mpm_set_shell_bending replaces the
 * hinge table and the damping table goes with the table it belonged to (mpm_get_shell_damping then returns zeros), and
 * whatever holds for an engine with shell bending holds for it -- partitioned and multi-rank engines refuse it, the rest
 * shape cannot be replaced under it.  It adds no launch: while some cloth has beta > 0 the hinge kernel's damped instance
 * runs in the undamped one's place and also reads the four corner velocities.  A cut hinge (mpm_set_tear_coupling) carries
 * no moment and is not damped.  MPM_ARR_FORCES includes the damping force; mpm_shell_forces and mpm_shell_state keep
 * reporting the elastic part alone.
 * STABILITY GUARD: beta TIGHTENS mpm_shell_max_stable_dt.  With W the rate of the elastic guard above (dt <= 2 / sqrt(W))
 * and G the same maximum with every row's sum times its cloth's beta, the limit becomes that of symplectic Euler on a
 * damped oscillator, the positive root of W dt^2 + 2 G dt = 4 (as mpm_links_max_stable_dt), rounded down; the refusal is
 * worded as the shell guard's.  While no cloth has beta > 0 it is the elastic limit to the bit.  Like the elastic guard it
 * holds AT THE REST SHAPE and is not a guarantee.  How conservative it is has not been measured.
 * mpm_set_shell_damping replaces the table (all-zero beta or n_cloths = 0 switches it off and frees the tables, the table
 * may then be NULL; otherwise n_cloths must equal mpm_cloth_count); it needs mpm_finalize and shell bending in force, runs
 * the substeps mpm_run_substeps still owes first, and is a synchronisation point.  Off means off: the engine then launches
 * exactly what it launched before the call.  beta > 0 on a cloth without hinges is accepted and does nothing.
 * Refused with MPM_ERR_INVALID, nothing enqueued, the previous table staying in force: a call before mpm_finalize; shell
 * bending off; a wrong n_cloths; a negative or non-finite beta; a non-zero reserved; a beta k cbar that is no finite
 * float; any partitioned or multi-rank engine. */
typedef struct mpm_cloth_shell_damping {
    float beta;       /* seconds, >= 0; 0: the cloth's hinges are not damped */
    float reserved;   /* must be 0 */
} mpm_cloth_shell_damping_t;
MPM_API int mpm_set_shell_damping(mpm_handle_t h, size_t n_cloths, const mpm_cloth_shell_damping_t *per_cloth);
/* The table as given: min(n, capacity) entries into out (may be NULL when capacity is 0), the cloth count into *n_out.
 * Zeros while the damper is off. */
MPM_API int mpm_get_shell_damping(mpm_handle_t h, mpm_cloth_shell_damping_t *out, size_t capacity, size_t *n_out);
/* The damping part alone on the current positions and velocities: f_out[3 * n_verts], in the vertex numbering of
 * mpm_dump_cpu_state (zeros while the damper is off).  The device functions of the substep's kernels; changes no state. */
MPM_API int mpm_shell_damping_forces(mpm_handle_t h, float *f_out);
/* On the current positions and velocities: power_per_cloth[mpm_cloth_count] = sum of the hinges' float terms
 * (bkc psidot) psidot, the dissipated power, as the hinge kernel forms them, added in double in hinge order (a fixed
 * order, no atomics); psidot_out (one per hinge of mpm_shell_hinges, may be NULL): the hinge's psidot, 0 for a hinge that
 * does not act -- reported whether or not the hinge's cloth is damped.  Changes no state. */
MPM_API int mpm_shell_damping_state(mpm_handle_t h, double *power_per_cloth, float *psidot_out);
/* Host only: the inline function the damped hinge kernel calls, compiled for the host.  x12, v12: positions and
 * velocities of x0, x1, x2, x3; kc = float(k cbar); bkc = float(beta k cbar); rec12_out: the four corner records of the
 * elastic and the damping moment together; psi_out, psidot_out (may be NULL).  Returns 1 where the hinge acts, 0 where it
 * does not (exact zeros, whatever the velocities), a negative code on a null argument. */
MPM_API int mpm_shell_hinge_damped(const float x12[12], const float v12[12], float kc, float psibar, float bkc,
                                   float rec12_out[12], float *psi_out, float *psidot_out);

/* ---- Creases: plastic shell hinges that keep a fold (an extension of shell bending) ----
 * Shell bending is elastic: a sheet folded in half springs back flat.  With creases a hinge's rest value psibar, the
 * number the hinge kernel reads, evolves on the device under a yield rule, so paper, foil, pressed fabric and pleats
 * keep their folds.  Per cloth: y = float(2 sin(yield_angle / 2)), eta = hardening, P = float(2 sin(max_angle / 2))
 * (max_angle 0 means pi, P = 2), formed in double and rounded once.  In every substep, BEFORE the hinge force, per hinge
 * of a cloth with y > 0, with psi and dpsi of the shell block above on the positions of the substep's start:
 *   d = psi - psibar,  ad = |d|,  t = ad dpsi;   the hinge yields where it acts and t > y (never on a NaN); then
 *   dy = y / dpsi,  dn = dy + eta (ad - dy),  psibar' = min(max(psi - copysign(dn, d), -P), P);   else psibar' = psibar
 * in float, every operation written out, no contraction, the division correctly rounded.  The rule acts on the
 * generalised moment conjugate to theta, k cbar (psi - psibar) dpsi, not on psi - psibar alone: dpsi -> 0 as |theta| ->
 * pi, so a hinge folded flat onto itself, where psi jumps between +2 and -2, carries no moment and does not yield -- a
 * sheet folded in half does not flip its crease when theta wobbles across pi.  It is a return mapping: from the substep
 * in which a hinge yields its moment is at most k cbar (y + eta (t - y)), up to rounding; psibar moves towards psi and
 * never past it.  eta is the post-yield tangent over the elastic one; 0 is perfectly plastic.  psibar stays in [-P, P].
 * NOT MODELLED: no rate dependence, no softening, no coupling between neighbouring hinges, and the psi discontinuity at
 * |theta| = pi that the shell model documents stays.  Creases in mpm_set_bending's quadratic model are not provided.
 * On the device: one kernel of one lane per hinge immediately in front of the hinge kernel, counted under
 * MPM_PHASE_VFORCE, launched only while the crease tables exist: while some cloth has yield_angle > 0 or some hinge's
 * psibar differs from its rest value.  Otherwise the engine launches exactly what it launches without these calls.
 * Decisions are taken hinge by hinge (Jacobi), one writer per hinge, no atomics: the same bits whatever the particle
 * order, deterministic mode or substep path; a substep that skips itself changes nothing.
 * Reports: mpm_shell_hinges keeps reporting the REST psibar; mpm_shell_forces and mpm_shell_state use the psibar in
 * force, so they show the creased forces and the elastic energy 1/2 k cbar (psi - psibar)^2.  mpm_shell_max_stable_dt
 * does not change: its Gauss-Newton term does not contain psibar.
 * mpm_set_shell_bending replaces the hinge table, and the crease parameters and state go with the table they belonged
 * to (as link limits go with mpm_set_links): set them again afterwards.
 * Every setter needs mpm_finalize and shell bending on, runs the substeps mpm_run_substeps still owes first (with the
 * old values), is ordered on the engine's stream and is a synchronisation point.  Refused with MPM_ERR_INVALID, nothing
 * changed, the message naming the cloth or hinge: a call before mpm_finalize; shell bending off; a wrong count;
 * yield_angle neither 0 nor in (0, pi) (or so small that y rounds to 0), or NaN; hardening outside [0, 1); max_angle
 * neither 0 nor in (0, pi]; a P below the rest |psibar| of a hinge of the cloth; mpm_set_crease_state with a non-finite
 * value or |psibar| above its hinge's P; a null array with n > 0; any partitioned or multi-rank engine. */
typedef struct mpm_cloth_crease {
    float yield_angle;   /* rad; 0: the cloth's hinges are elastic; else in (0, pi) */
    float hardening;     /* eta in [0, 1); 0: perfectly plastic */
    float max_angle;     /* rad; 0: pi; else in (0, pi]: psibar stays within 2 sin(max_angle / 2) */
    float reserved;      /* not read */
} mpm_cloth_crease_t;
/* n_cloths is 0 (the table may be NULL) or mpm_cloth_count.  All zeros switches yielding off and KEEPS the creases made
 * so far (mpm_set_crease_state(h, NULL) removes them). */
MPM_API int mpm_set_creases(mpm_handle_t h, size_t n_cloths, const mpm_cloth_crease_t *per_cloth);
/* The table as given: min(mpm_cloth_count, capacity) entries into out (zeros while off), the cloth count into *n_out. */
MPM_API int mpm_get_creases(mpm_handle_t h, mpm_cloth_crease_t *out, size_t capacity, size_t *n_out);
/* Scissors and restore: psibar[n_hinges] (hinge order of mpm_shell_hinges) replaces every hinge's psibar, so it can
 * pre-crease a cloth; NULL irons the cloth: every hinge returns to its rest psibar to the bit.  Allowed while every
 * yield_angle is 0. */
MPM_API int mpm_set_crease_state(mpm_handle_t h, const float *psibar);
/* The psibar in force per hinge (psibar_out[n_hinges], may be NULL) and per cloth the number of hinges whose psibar
 * differs from the rest value in bits: min(cloth count, capacity) entries into creased_per_cloth, the cloth count into
 * *n_out.  Zeros while off. */
MPM_API int mpm_crease_state(mpm_handle_t h, float *psibar_out, uint32_t *creased_per_cloth, size_t capacity, size_t *n_out);
/* The substep's hinge function on the current positions, state untouched: psi, dpsi and the psibar the next substep
 * would leave, per hinge; each may be NULL. */
MPM_API int mpm_crease_measure(mpm_handle_t h, float *psi_out, float *dpsi_out, float *psibar_next_out);
/* The kernel's two inline functions on the host (no handle, no device), hinge by hinge: x12[12 n] = x0, x1, x2, x3;
 * psibar, y, eta, P [n]; psi_out, dpsi_out, psibar_out [n] and yields_out [n] may each be NULL. */
MPM_API int mpm_crease_hinge(size_t n, const float *x12, const float *psibar, const float *y, const float *eta, const float *P,
                             float *psi_out, float *dpsi_out, float *psibar_out, uint8_t *yields_out);

/* ---- Energy, momentum and strain report per cloth (an extension) ----
 * What System::CalcKineticEnergy / CalcPotentialEnergy answer for a Drake plant, and what a caller choosing dt or
 * calibrating a stiffness needs: one device-side reduction instead of seven downloads and a host restatement of the
 * constitutive model.  All arithmetic is in double, from the engine's float records:
 *   m       the float MPM_ARR_MASSES returns for the particle.
 *   vertex  x, v and C are the particle's own records.
 *   face    x and v are the means of its three corner vertices' current x and v -- the state the next
 *           CalcFemStateAndForce gives it; the face particle's own x / v record is stale inside and after the batched
 *           substeps and is not used.  C is its own record.
 *   D       dx^2 / 4, the second moment of the quadratic B-spline: 1/2 m D |C|_F^2 and m D (C21-C12, C02-C20, C10-C01)
 *           are the kinetic energy and the angular momentum of the particle's affine velocity field on the grid.
 *   strain  d1, d2 = (x_b - x_a, x_c - x_a) Dm^-1 from the CURRENT corner positions, d3 the stored normal column F[:,2].
 *           a11 = d1.d1, a12 = d1.d2, a22 = d2.d2, J = sqrt(max(a11 a22 - a12^2, 0)), T = a11 + a22,
 *           s1 +- s2 = sqrt(max(T +- 2 J, 0)) (the singular values of [d1 d2]); with n = d1 x d2, r22 = d3.n / |n|; a
 *           face with |n| = 0 takes r22 = 0 and contributes no normal or shear energy.
 *   energy  psi_in = mu ((s1-1)^2 + (s2-1)^2) + 1/2 lambda (J-1)^2,  psi_n = K/3 (1-r22)^3 if r22 < 1, else 0,
 *           psi_s = 1/2 gamma max(|d3|^2 - r22^2, 0), with the floats mu, lambda, K, gamma the FEM kernel uses for the
 *           face's cloth, times the face's rest volume V.  This is the published energy of Jiang et al. 2017, whose
 *           gradient the FEM stress is for gamma = 0.  For gamma != 0 the report STATES this energy; no claim is made
 *           that the stress the engine applies (the reference's) is its gradient.
 *   bending E = -1/4 sum_i sum_{j != i} c_ij |x_j - x_i|^2 with c_ij the float coefficients of the table the bending
 *           kernel reads (= 1/2 x^T k Q x: Q is symmetric with zero row sums), per cloth; 0 while bending is off.
 *   The potentials of force fields (mpm_set_force_fields) are NOT reported: most of them (drag, wind) have none.
 *   The elastic energy of the links (mpm_set_links) is NOT in this record either, whose layout is unchanged: links join
 *   cloths, so it belongs to no row; mpm_link_energy reports it.
 *   The energy of the weave (mpm_set_weave) is NOT in this record either, whose layout is unchanged: elastic_in_plane is
 *   the isotropic membrane's alone; mpm_weave_energy reports the weave's, per cloth.
 * gravity_potential is -sum m g x[gravity_axis] with g = mpm_material_t::gravity (signed) -- zero at the world origin.
 * The sums are formed in ORIGINAL id order in a fixed tree, without floating-point atomics: a row is the same bits
 * whatever the particle order (slot order, arrival order inside a cell, deterministic mode on or off). */
typedef struct mpm_cloth_measure {
    double mass;                        /* sum m                                          */
    double mass_position[3];            /* sum m x        (centre of mass = this / mass)  */
    double momentum[3];                 /* sum m v                                        */
    double angular_momentum[3];         /* sum m x cross v, about the world origin        */
    double affine_angular_momentum[3];  /* sum m D (C21-C12, C02-C20, C10-C01)            */
    double kinetic;                     /* sum 1/2 m |v|^2                                */
    double kinetic_affine;              /* sum 1/2 m D |C|_F^2                            */
    double gravity_potential;           /* -sum m g x[gravity_axis], g = material.gravity */
    double elastic_in_plane, elastic_normal, elastic_shear;   /* sum over faces of V psi_* */
    double bending;                     /* 1/2 x^T (k Q) x of the cloth, 0 while off      */
    float stretch_max, stretch_min;     /* max s1, min s2 over the faces                  */
    float normal_min;                   /* min r22 over the faces                         */
    float speed_max;                    /* max |v| over the VERTEX particles              */
    uint32_t faces, vertices;           /* particles counted                              */
} mpm_cloth_measure_t;                  /* 184 bytes */
/* One row per cloth, in cloth order: min(mpm_cloth_count, capacity) rows into per_cloth (may be NULL when capacity is
 * 0), the cloth count into *n_cloths_out, and into *total the sum of ALL the cloths' rows in cloth order, formed in
 * double -- its extremes the max / min over the rows, its counts the sums of theirs.  Either output may be NULL.  A cloth
 * with nothing counted reports stretch_max = speed_max = 0 and stretch_min = normal_min = +inf.
 * Needs mpm_finalize (MPM_ERR_INVALID before).  Ordered on the engine's stream and a synchronisation point; substeps
 * that mpm_run_substeps still owes are run first.  At most three kernel launches.  Changes no state, no counter of
 * mpm_stats_t and no sticky error.
 * A partitioned engine (mpm_dist_init) counts the particles the rank OWNS and skips the others: the ranks' rows add up
 * to the scene's, and a multi-rank caller adds them itself. */
MPM_API int mpm_measure(mpm_handle_t h, mpm_cloth_measure_t *per_cloth, size_t capacity, size_t *n_cloths_out,
                        mpm_cloth_measure_t *total);
/* The faces' terms of the report, per face: out[4 * n_faces] = (s1, s2, r22, V (psi_in + psi_n + psi_s)) as floats,
 * in original face order.  Same calling rules as mpm_measure; refused (MPM_ERR_INVALID, nothing enqueued) on a
 * partitioned or multi-rank engine. */
MPM_API int mpm_face_strain(mpm_handle_t h, float *out);
/* The energy density on the host (no handle, no device): the inline function of the report's kernels, compiled for
 * the host.  F: n row-major 3x3 deformation gradients (columns d1, d2, d3); out[6 * n] = s1, s2, r22, psi_in, psi_n,
 * psi_s in double.  The Lame parameters are formed from m in float, as mpm_finalize forms them. */
MPM_API int mpm_cloth_energy_density(const mpm_cloth_material_t *m, size_t n, const float *F, double *out);

/* Runs n substeps with HIP events around every kernel group on the engine's
 * stream and returns the mean milliseconds per substep of each phase
 * (phase_ms[MPM_PHASE_COUNT]) and of the whole substep.  The launches are those of mpm_run_substeps, but every substep
 * carries its re-sort launches and none skips itself.  MPM_PHASE_VFORCE is the vertex-force kernel (and the bending,
 * link, pressure, shell-bending and anchor kernels behind it) wherever the engine launches it -- a mesh with a vertex of
 * more than eight faces, an engine with bending stiffness, links, pressure, shell bending or anchors --; on every other engine ParticleToGrid sums the vertex forces itself and the phase is empty. */
MPM_API int mpm_profile_substeps(mpm_handle_t h, int n, float dt, int mpm_bc, float *phase_ms, float *total_ms);

/* ---- multi-GPU: one engine per GPU, domains tiled along x ------------------
 * Each rank runs its own engine on its own local grid; neighbouring ranks' grids overlap in a
 * few block layers next to the cut.  Per substep, between mpm_particle_to_grid and the grid
 * update:  mpm_grid_gather -> mpm_halo_pack (one buffer per neighbour) -> exchange the buffers
 * (RCCL send/recv on the same stream, done by the caller) -> mpm_halo_add for every received
 * buffer -> mpm_update_grid_from_sums.  Nothing here synchronises with the host.
 * The reference has no multi-GPU path (settings.h:40 G_DEVICE_COUNT = 1); this is new surface. */

/* Raw node sums (mass, momentum) of all active blocks, without the update. */
MPM_API int mpm_grid_gather(mpm_handle_t h);
/* Size in bytes of a halo buffer for `capacity_blocks` blocks. */
MPM_API size_t mpm_halo_buffer_bytes(size_t capacity_blocks);
/* Packs the sums of the active blocks whose x block coordinate is in [bx_lo, bx_hi] into
 * dev_buf (device memory), relabelled by shift_bx blocks (the neighbour's local coordinates). */
MPM_API int mpm_halo_pack(mpm_handle_t h, int bx_lo, int bx_hi, int shift_bx, void *dev_buf, size_t capacity_blocks);
/* Adds a neighbour's packed sums to the local ones (blocks that are not active here are skipped). */
MPM_API int mpm_halo_add(mpm_handle_t h, const void *dev_buf, size_t capacity_blocks);
/* UpdateGrid (cuda_mpm_solver.cu:107-151) on sums that already include the neighbours'. */
MPM_API int mpm_update_grid_from_sums(mpm_handle_t h, int mpm_bc);
/* The two halves of a multi-GPU substep: RebuildMapping + CalcFemStateAndForce + ParticleToGrid +
 * mpm_grid_gather, and mpm_update_grid_from_sums + GridToParticle. */
MPM_API int mpm_substep_begin(mpm_handle_t h, float dt);
MPM_API int mpm_substep_end(mpm_handle_t h, float dt, int mpm_bc);
/* The same with the halo kernels folded in (one host call either side of the exchange):
 * begin + mpm_halo_pack for each of the n_zones <= 2 (bx_lo[i], bx_hi[i], shift_bx[i]) -> send_bufs[i];
 * mpm_halo_add for each of the n_bufs received buffers + end. */
MPM_API int mpm_substep_begin_halo(mpm_handle_t h, float dt, int n_zones, const int *bx_lo, const int *bx_hi,
                                   const int *shift_bx, void *const *send_bufs, size_t capacity_blocks);
/* The same chain driven by the library itself: RCCL point-to-point on the engine's stream (no
 * event between pack, transfer and add; a cross-stream dependency costs ~20 us on this stack) and
 * one host call for a batch of substeps.  Rank 0 makes the id (mpm_chain_unique_id), the caller
 * distributes its 128 bytes by any means, every rank calls mpm_chain_init with its own handle.
 * Rank r's local frame is shifted by r * pitch_blocks blocks along x; cut_lo / cut_hi are the local
 * x block indices of the left / right cut planes, zone_blocks the halo depth either side of a cut.
 * periodic != 0 closes the chain into a ring (rank world-1's right neighbour is rank 0): used to
 * exercise the transport with a single rank, whose neighbours are then itself.  id == NULL: the geometry only, without
 * an RCCL communicator (for the direct transport below). */
MPM_API int mpm_chain_unique_id(char id_out[128]);
MPM_API int mpm_chain_init(mpm_handle_t h, const char id[128], int rank, int world, int cut_lo_block, int cut_hi_block,
                           int pitch_blocks, int zone_blocks, size_t capacity_blocks, int periodic);
MPM_API int mpm_chain_substeps(mpm_handle_t h, int n_substeps, float dt, int mpm_bc);
/* Partitioned domain (mpm_dist_init + mpm_chain_init with pitch_blocks = 0): mpm_chain_substeps also
 * swaps migration records with the neighbours every `every` substeps (mpm_dist_migrate_pack / _apply);
 * every = 0: when the ranks' common quiet-time estimate says so (mpm_dist_migration_quiet_time). */
MPM_API int mpm_chain_enable_migration(mpm_handle_t h, int every, size_t capacity_particles);
MPM_API int mpm_chain_destroy(mpm_handle_t h);
/* DIRECT halo exchange (round 5; the reference has no multi-GPU path, settings.h:40): instead of RCCL send / recv -- a
 * kernel of its own plus a staging copy, ~21 us of every chain substep on this stack -- the kernel that gathers a rank's
 * zone sums stores them straight into the NEIGHBOUR's receive buffer (device memory of the peer, mapped through a HIP IPC
 * handle; xGMI on one node), a one-thread kernel raises a sequence flag over there, and a one-wave kernel on the
 * receiving side waits for it (bounded: MPM_HALO_TIMEOUT_S, default 5 s, then MPM_ERR_HALO) before the grid update reads
 * the sums.  Receive buffers alternate between two parities, so nobody overwrites what a neighbour may still read.
 *   mpm_chain_init(h, NULL, rank, world, ...)     the geometry alone (no RCCL communicator; or with an id: RCCL stays
 *                                                 available for the rare exchanges -- migration, the contact solve)
 *   mpm_chain_direct_prepare(h, handle_out)       allocates this rank's receive buffers, returns their IPC handle
 *   (the caller hands every rank its neighbours' 64 bytes, by any means)
 *   mpm_chain_direct_connect(h, left, right)      maps the neighbours' buffers (NULL where there is no neighbour; a rank
 *                                                 that is its own neighbour -- a ring of one -- needs no handle);
 *                                                 both NULL on a rank that HAS neighbours: the direct path is switched
 *                                                 off again (what a caller does on every rank when one of them could
 *                                                 not map its neighbour: all ranks must use the same transport)
 * mpm_chain_substeps then uses the direct path for the per-substep halo.  Validated on one GPU only (two processes
 * sharing it; the ring of one): the protocol, the indexing and the time-out -- NOT the ordering of peer stores across
 * two devices, which this build has never run on. */
MPM_API int mpm_chain_direct_prepare(mpm_handle_t h, char handle_out[64]);
MPM_API int mpm_chain_direct_connect(mpm_handle_t h, const char left_handle[64], const char right_handle[64]);
/* Round 6: the region must be FINE-GRAINED device memory -- mpm_chain_direct_prepare returns MPM_ERR_HIP when the runtime
 * refuses it (a coarse-grained region would let stale lines of the receiver's L2 shadow a peer's stores: wrong sums, no
 * error flag), and the caller then keeps every rank on RCCL; MPM_DIRECT_COARSE_OK=1 accepts plain device memory for
 * rehearsals on ONE device.  The pack counts its entries in this device's memory and the count travels with the signal: no
 * returning atomic on peer memory.
 * Neighbours that live in THIS process (an in-process world: several ranks of one partition on one stream) are named by
 * pointer -- a HIP IPC handle of one's own process cannot be opened: mpm_chain_direct_base hands a rank's region out,
 * mpm_chain_direct_connect_local takes the neighbours' (NULL where there is none). */
MPM_API int mpm_chain_direct_base(mpm_handle_t h, void **base_out);
MPM_API int mpm_chain_direct_connect_local(mpm_handle_t h, void *left_base, void *right_base);

/* TEAM transport of the distributed contact solve (round 6; the reference has one device, settings.h:40, and reads its
 * global scalars back per Newton iteration, cuda_mpm_solver.cu:318-319, 359-363, 515-517, 567-570): on a partitioned
 * domain the per-node Hessian / gradient sums of the zone blocks go to the two neighbours and the line-search sums to
 * every rank as stores into each other's memory + sequence flags ON THE ENGINE'S STREAM; every rank adds all ranks' sums
 * in rank order (identical bits, identical `E1 <= E0` decisions, no collective library), whether any rank has a pair at
 * all and whether any rank must refuse its solve (buffers overflowed, a wrong guess of its host) is agreed the same way,
 * and the host only polls the mailbox, as on one GPU.  Needs mpm_dist_init; at most 8 ranks (one node).
 *   mpm_team_prepare(h, zone_capacity_blocks, handle_out, base_out)   allocates this rank's region (fine-grained, as
 *        above), returns its IPC handle (64 bytes, may be NULL) and its address (for ranks of the same process, may be NULL)
 *   mpm_team_connect(h, handles, local_bases)   handles: world x 64 bytes in rank order (own entry ignored) or NULL;
 *        local_bases: world pointers or NULL -- a rank of this process is named by its region's address, any other by
 *        its handle.
 * mpm_chain_destroy -- and mpm_chain_init, which starts from a clean chain -- release the team's region too: set the chain up
 * first (mpm_chain_init, mpm_chain_direct_*), then the team.
 * With the team connected, mpm_update_contact on a partitioned engine runs the device-resident solve (EVERY rank must
 * call it in every coupled substep, with or without pairs of its own), and mpm_run_coupled_substeps accepts a partitioned
 * engine whose halo runs over the direct transport: n coupled substeps per call, no migration inside (the caller runs the
 * substeps between two migrations in one call), no contact-free speculation.  mpm_world_coupled_substeps does the same for
 * the n_local ranks of an in-process world (all on one stream), enqueued phase by phase across the ranks; results: n_local
 * arrays of n entries, or NULL.  Validated between processes sharing one GPU and in in-process worlds: the protocol, the
 * indexing, the rank-order sums -- NOT the ordering of peer stores across two devices. */
MPM_API int mpm_team_prepare(mpm_handle_t h, size_t zone_capacity_blocks, char handle_out[64], void **base_out);
MPM_API int mpm_team_connect(mpm_handle_t h, const char *handles, void *const *local_bases);

/* ---- multi-GPU, ONE domain cut into x slabs (strong scaling) ------------------------------
 * Every rank is created and finalised with the WHOLE scene (same mpm_add_qr_cloth calls: replicated
 * topology, full-capacity arrays) and then keeps only its share: rank r owns the particles whose
 * base cell lies in x blocks [own_lo_block, own_hi_block) (the outermost ranks extend to the walls),
 * plus ghost copies of the neighbours' particles within ghost_cells of a cut.  Ghosts take part in
 * CalcFemStateAndForce and GridToParticle on both ranks (same inputs, same arithmetic: the copies
 * stay bit-identical without communication) and scatter nothing in ParticleToGrid.  Per substep the
 * ranks exchange the node sums of the blocks within zone_blocks of a cut: mpm_substep_begin_halo with
 * zones [cut - zone_blocks, cut + zone_blocks - 1] and shift 0, then mpm_substep_end_halo (or
 * mpm_chain_substeps with pitch 0).  Every few substeps particles change hands:
 *   mpm_dist_migrate_pack -> exchange the two record buffers with the neighbours ->
 *   mpm_dist_migrate_apply -> (the next RebuildMapping merges / drops them).
 * Requirements, checked: 4 * zone_blocks >= ghost_cells + ghost_margin_cells + 2; a slab with two
 * neighbours is at least 2 * zone_blocks wide; a particle whose stencil leaves the shared zone, or a
 * face that misses a corner vertex (mesh edge longer than ghost_margin_cells), raises MPM_ERR_HALO.
 * Arrays downloaded from a rank hold NaN / -1 for particles it does not have; mpm_dist_roles tells
 * which are owned (1), ghosts (2) or absent (0), per slot.  The reference has no multi-GPU path.
 * Meshes: any valence.  The per-slot topology that migrates with a vertex holds eight (face, corner) ids (cloth meshes
 * have six faces around a vertex); a mesh with a vertex of more keeps the scene's adjacency (4 bytes per vertex + 12 per
 * face) on every rank, and such a vertex sums its force over it.  After the call a rank's particle arrays are sized for
 * slot_headroom x what it holds (default 1.5; MPM_DIST_HEADROOM, 0 = keep the whole scene's size); a rank whose share
 * outgrows that is re-allocated at the migration that would overflow it (the stream is idle there), up to
 * the whole scene's size. */
typedef struct {
    int32_t rank, world;
    int32_t own_lo_block, own_hi_block;     /* this rank's x blocks */
    int32_t left_lo_block, right_hi_block;  /* outer ends of the neighbours' ranges (ignored without neighbour) */
    int32_t zone_blocks;                    /* depth of the exchanged zone either side of a cut */
    int32_t ghost_cells;                    /* width of the ghost band for face particles (>= longest mesh edge) */
    int32_t ghost_margin_cells;             /* the band for vertex particles is wider by this much (>= longest
                                               mesh edge), so that a ghost face always has its corners */
} mpm_dist_config_t;
MPM_API int mpm_dist_init(mpm_handle_t h, const mpm_dist_config_t *config);
/* ghost_cells = ghost_margin_cells = 0 selects BANDS FROM THE MESH: fractional widths (in cells, measured on x / dx - 0.5)
 * chosen so that the drift every particle may accumulate along x between two migrations is as large as the zone allows:
 *   reach = 0.75 x longest mesh edge (cells);   drift = (4 zone_blocks - 2 - 2 reach) / 3;
 *   face band = reach + 2 drift;   vertex band = 2 reach + 2 drift.
 * (zone_blocks = 2 and 0.62-cell edges: drift 1.7 cells against 0.8 for the integer bands 2 + 2; zone_blocks = 1, the
 * only depth a slab two blocks wide allows: 0.36 cells, where integer bands 1 + 1 leave none.)  Given integer bands
 * allow drift = min((ghost_cells - reach) / 2, 4 zone_blocks - 2 - ghost_cells - ghost_margin_cells). */
typedef struct {
    float face_band_cells, vertex_band_cells;   /* as in use */
    float drift_budget_cells;                   /* what a particle may drift along x between two migrations */
    float longest_edge_cells;
    uint32_t slot_resizes;                      /* re-allocations of the rank's slot space (1 = mpm_dist_init's own) */
    uint32_t migrations;                        /* mpm_dist_migrate_pack calls so far */
    uint32_t retunes;                           /* times mpm_dist_retune changed the band widths */
} mpm_dist_geometry_t;
MPM_API int mpm_dist_get_geometry(mpm_handle_t h, mpm_dist_geometry_t *out);
/* Slot space of a partitioned rank = factor x what it holds after the partition (default 1.5, or MPM_DIST_HEADROOM;
 * 0 = keep the whole scene's size).  Before mpm_dist_init.  Whatever the factor, a migration that would overflow
 * the slot space re-allocates it first (mpm_dist_migrate_apply), up to the whole scene's size. */
MPM_API int mpm_dist_set_headroom(mpm_handle_t h, float factor);
/* Adaptive migration cadence.  mpm_dist_migrate_pack also estimates how long no particle this rank holds can drift
 * further along x than drift_budget_cells if all keep moving ballistically (a particle far from both cuts has to get
 * near one first); this call waits for the stream and returns that time (seconds, may be infinity).  The ranks take
 * the minimum over all of them and migrate again when a share of it has passed (mpm_chain_enable_migration with
 * every = 0 does exactly that: ncclAllReduce(min), half of the common estimate). */
MPM_API int mpm_dist_migration_quiet_time(mpm_handle_t h, float *seconds_out);
/* Bands from the mesh follow the motion: called by every rank with the ranks' COMMON estimate right after a migration
 * (mpm_chain_substeps does it itself), this re-sizes the bands so that at the speed that estimate implies a migration is
 * due every ~16 substeps (MPM_DIST_INTERVAL): wide bands for a cloth that moves along x, the narrowest (0.125 cells of
 * drift: fewest ghost particles) for one that does not; within what the zone allows, in steps of an eighth of a cell.
 * All ranks compute the same widths from the same numbers; they take effect at the next migration.  No-op for given
 * integer bands or with MPM_DIST_RETUNE=0. */
MPM_API int mpm_dist_retune(mpm_handle_t h, float quiet_time_all, float dt, int *changed_out);
MPM_API size_t mpm_dist_migration_buffer_bytes(size_t capacity_particles);
/* send_left / send_right: device buffers of mpm_dist_migration_buffer_bytes(capacity) each (both
 * required; a rank without that neighbour gets an empty one).  recv_*: what the neighbours packed, or NULL. */
MPM_API int mpm_dist_migrate_pack(mpm_handle_t h, void *send_left, void *send_right, size_t capacity_particles);
MPM_API int mpm_dist_migrate_apply(mpm_handle_t h, const void *recv_left, const void *recv_right,
                                   size_t capacity_particles);
MPM_API int mpm_dist_roles(mpm_handle_t h, uint8_t *roles_out /* n_particles */);
/* What mpm_dist_migrate_apply decides from the two 16-byte headers of the received buffers ([0] records, [1] how many of
 * them are faces, [2..3] zero; NULL = no such neighbour) before it sizes anything: the headers are CHECKED against the
 * buffers' capacity and the scene (more records than the buffers hold: MPM_ERR_CAPACITY, the sender overflowed; more
 * faces than records or non-zero padding: MPM_ERR_INVALID, a corrupt header; inconsistent own counts:
 * MPM_ERR_INTERNAL), then out6 = {arriving faces, arriving vertices, face slots needed, vertex slots needed, face
 * slots to re-allocate to, vertex slots to re-allocate to} (the last two equal the current slot space when it
 * suffices; never more than the scene has).  Host arithmetic only: works without a GPU (tests/test_error_paths.py). */
MPM_API int mpm_dist_plan_migration(const uint32_t *hdr_left, const uint32_t *hdr_right, size_t capacity_particles,
                                    size_t scene_faces, size_t scene_vertices, size_t held_faces, size_t held_vertices,
                                    size_t face_slots, size_t vertex_slots, float headroom, size_t out6[6]);
/* Re-allocation of a partitioned rank's slot space is TWO-PHASE: every new array is allocated before anything of the
 * engine is touched, so a failed allocation (MPM_ERR_NOMEM) leaves the handle exactly as it was -- usable, at its old
 * size, with the arriving records not applied (the caller may free memory and call mpm_dist_migrate_apply again with
 * the same buffers). */

/* Tests of the error contract.  mpm_debug_throw raises a C++ exception inside an entry point (kind 0: std::bad_alloc,
 * 1: std::length_error from a container asked for an absurd size, 2: a non-std exception) and returns what the
 * boundary's catch-all made of it: MPM_ERR_NOMEM / MPM_ERR_INTERNAL, message in mpm_last_error(); host code only.
 * mpm_debug_fail_alloc: the engine's nth device allocation from now fails as if the device were out of memory
 * (0 = off). */
MPM_API int mpm_debug_throw(int kind);
MPM_API int mpm_debug_fail_alloc(mpm_handle_t h, int nth);

/* UpdateContact on a partitioned domain.  Every rank solves for the grid nodes it holds with the
 * contacts of the particles it OWNS (pass only those to mpm_copy_contact_pairs;
 * mpm_generate_contact_pairs does so by itself).  Per Newton iteration the ranks (1) exchange the
 * contact Hessian / gradient sums of the nodes in the zones next to the cuts (a node there can be
 * reached by contacts of both ranks), after which both compute the same direction for it, and (2)
 * all-reduce the line-search energies, sum |Dir|^2 and the DoF count -- the scalars the reference
 * reads back per iteration (cuda_mpm_solver.cu:318-319, 359-363, 515-517, 567-570); shared nodes are
 * counted on their owner.  The step and the stopping decision then agree on all ranks.
 * Transport: the native chain when mpm_chain_init was called (RCCL on the engine's stream), else the
 * two callbacks below.  exchange: send_* / recv_* are device buffers of `bytes` bytes each, the
 * engine's stream has been synchronised before the call and the received bytes must be in place on
 * return (a missing neighbour's buffers are to be ignored).  allreduce: sum `n` doubles in place over
 * all ranks (host memory).  Per-body impulses (mpm_external_body_force_to_host) are per-rank partial
 * sums: add them over the ranks. */
typedef int (*mpm_exchange_fn)(void *user, void *send_left, void *send_right, void *recv_left, void *recv_right,
                               size_t bytes);
typedef int (*mpm_allreduce_fn)(void *user, double *values, size_t n);
MPM_API int mpm_dist_set_transport(mpm_handle_t h, mpm_exchange_fn exchange, mpm_allreduce_fn allreduce, void *user,
                                   size_t zone_capacity_blocks);

/* Optional, between the two: the part of UpdateGrid and GridToParticle that does not depend on the
 * neighbours' sums (blocks outside the zones given to begin, work items whose tiles do not touch a
 * zone), to be enqueued while the exchange is in flight; mpm_substep_end_halo then only does the rest. */
MPM_API int mpm_substep_mid_halo(mpm_handle_t h, float dt, int mpm_bc);
MPM_API int mpm_substep_end_halo(mpm_handle_t h, float dt, int mpm_bc, int n_bufs, const void *const *recv_bufs,
                                 size_t capacity_blocks);

/* Use a caller-provided hipStream_t (e.g. torch's current stream); NULL
 * restores the engine's own stream. */
MPM_API int mpm_set_stream(mpm_handle_t h, void *hip_stream);

MPM_API int mpm_get_stats(mpm_handle_t h, mpm_stats_t *out);

/* Diagnostic build support: 16 device counters that kernels fill only when the
 * MPM_DBG environment variable has bit 2 set (see DESIGN.md "Diagnostics"). */
MPM_API int mpm_debug_counters(mpm_handle_t h, uint64_t *out16, int reset);

/* Tests: one table of the last conditional re-sort (drake_amd/csrc/mpm_rebuild.h), copied to the host as it stands.
 * Launches what phase calls have held back, waits for the engine's stream, then copies.  Every table is an array of
 * 4-byte words (int4 / int2 records flattened); *count_out gets the number of words (also when `out` is too small,
 * which fails with MPM_ERR_INVALID).
 *   MPM_RT_CTL     14 words: cur, need_rebuild, rebuilds, nfa, nva, add_f, add_v, n_home, n_active, n_items,
 *                  n_items_wanted, error, quiet_time (float bits), ticket
 *   MPM_RT_PARAMS  16 words: Nf, Np, bits, nb, nblocks, capH, capA, capI, capS, item_groups, item_groups_small,
 *                  item_small_below, anticip (float bits: cells binned ahead per unit of velocity, as the next re-sort
 *                  would use it), fem_fast, dist.on, NpG
 *   per slot (Np words): PKEY, PRANK, SRC_OF, DST_OF, PID (of the current particle set); IMAP: NpG words
 *   per home block (n_home records): HOME_BLOCK, HOME_RANGE (4), HOME_ITEMS (2), HOME_NGROUPS, HOME_NBR_ACT (27);
 *                  HOME_GROUPS: the whole pool, (Np / 64 + capH + 2) records of 4
 *   per active block (n_active records): ACT_BLOCK, ACT_NBR_HOME (27), ACT_NBR_ITEMS (27)
 *   per item (n_items records): ITEM_DESC (4), ITEM_ORDER, ITEM_POS, ITEM_FLAT (8), ITEM_RNG (4)
 *   whole arrays: LUT_HOME, LUT_ACT, BLKSTART0/1, BLKCNT0/1 (nblocks), CELLCNT0/1 (cells), HOME_BITS (nblocks / 32 + 1),
 *                  TICKETS (1024)
 *   FACE_REFS      per face slot (Nf records of 4): the face's record of corner references in the current set, bit
 *                  for bit: (corner ranks, slot of corner 0, of corner 1, of corner 2) */
enum mpm_resort_table {
    MPM_RT_CTL = 0, MPM_RT_PARAMS, MPM_RT_PKEY, MPM_RT_PRANK, MPM_RT_SRC_OF, MPM_RT_DST_OF, MPM_RT_IMAP, MPM_RT_PID,
    MPM_RT_HOME_BLOCK, MPM_RT_HOME_RANGE, MPM_RT_HOME_ITEMS, MPM_RT_HOME_NGROUPS, MPM_RT_HOME_GROUPS, MPM_RT_HOME_NBR_ACT,
    MPM_RT_ACT_BLOCK, MPM_RT_ACT_NBR_HOME, MPM_RT_ACT_NBR_ITEMS, MPM_RT_LUT_HOME, MPM_RT_LUT_ACT,
    MPM_RT_ITEM_DESC, MPM_RT_ITEM_ORDER, MPM_RT_ITEM_POS, MPM_RT_ITEM_FLAT, MPM_RT_ITEM_RNG,
    MPM_RT_BLKSTART0, MPM_RT_BLKSTART1, MPM_RT_BLKCNT0, MPM_RT_BLKCNT1, MPM_RT_CELLCNT0, MPM_RT_CELLCNT1,
    MPM_RT_HOME_BITS, MPM_RT_TICKETS, MPM_RT_FACE_REFS
};
MPM_API int mpm_debug_resort_tables(mpm_handle_t h, int which, void *out, size_t capacity_bytes, size_t *count_out);

/* Tests: the device radix sort (drake_amd/csrc/mpm_sort.h) on caller-made pairs.  Two buffer pairs a and b of n pairs
 * each are filled with byte patterns (keys a 0xA5, values a 0x5A, keys b 0xB6, values b 0x6B); the first n pairs --
 * with device_count >= 0 only the first device_count -- are uploaded into a; the n pairs are sorted by the key bits
 * [0, bits), stable.  device_count >= 0: the count is handed over in device memory and n is only the launch bound.
 * want_in_place != 0: the result is asked for in a; 0: wherever the last pass left it, info_out[3] says where.
 * keys_out / vals_out: uint32[2 n], pair a then pair b, both downloaded in full.
 * info_out: {digit bits, passes, tiles, result in b}. */
MPM_API int mpm_debug_sort_pairs(mpm_handle_t h, const uint32_t *keys, const uint32_t *vals, size_t n, int bits,
                                 int device_count, int want_in_place, uint32_t *keys_out, uint32_t *vals_out,
                                 int info_out[4]);

/* Copies one engine array to the host (see mpm_array_id).  `bytes` is the
 * size of `out`; the call fails if it is too small. *written gets the number
 * of bytes produced (may be NULL). */
MPM_API int mpm_download_array(mpm_handle_t h, int which, void *out, size_t bytes, size_t *written);

/* Overwrites particle state -- checkpoint restore and test injection.  pos,
 * vel (float[3*np]), affine (float[9*np]), volumes (float[np]) are in slot
 * order; deformation_gradients (float[9*nf]) in original face order, like
 * mpm_download_array returns them.  Any pointer may be NULL (left unchanged). */
MPM_API int mpm_upload_particle_state(mpm_handle_t h, const float *pos, const float *vel, const float *affine,
                                      const float *volumes, const float *deformation_gradients);

/* The root finder inside UpdateContact's exact line search (cuda_mpm_solver.cu:383-471), a float
 * clone of Drake's DoNewtonWithBisectionFallback (multibody/contact_solvers/
 * newton_with_bisection.cc:14-119), exposed so that the reference's own root-finding cases
 * (multibody/contact_solvers/test/newton_with_bisection_test.cc:55-225) can be run through the
 * product's code.  fn(user, x, &f, &df) evaluates the function and its derivative.  flags = 0 gives
 * Drake's semantics; the solver uses MPM_RF_SIGN3 | MPM_RF_NO_ENDS | MPM_RF_STEP_LAST (the clone's
 * deviations, see drake_amd/csrc/mpm_rootfind.h).  Returns 0 on convergence, 1 when max_evals ran
 * out (Drake throws), negative on bad arguments.  Host code only: works without a GPU. */
enum { MPM_RF_SIGN3 = 1, MPM_RF_NO_ENDS = 2, MPM_RF_STEP_LAST = 4 };
typedef void (*mpm_rootfind_fn)(void *user, double x, double *f, double *df);
MPM_API int mpm_newton_bisect_f64(mpm_rootfind_fn fn, void *user, double x_lo, double x_hi, double guess,
                                  double x_tol, double f_tol, int max_evals, int flags, double *root_out,
                                  int *evals_out);
MPM_API int mpm_newton_bisect_f32(mpm_rootfind_fn fn, void *user, float x_lo, float x_hi, float guess, float x_tol,
                                  float f_tol, int max_evals, int flags, float *root_out, int *evals_out);

#ifdef __cplusplus
}
#endif
#endif /* MPM_HIP_H_ */
