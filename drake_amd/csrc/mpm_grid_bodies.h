// Rigid bodies in the grid update (mpm_set_grid_bodies, mpm_bc = MPM_BC_BODIES; include/mpm_hip.h).
// The boundary condition of update_grid_kernel (cuda_mpm_kernels.cuh:660-789) for posed, moving bodies of every kind the
// contact path knows -- the six analytic kinds of mpm_collider_t and the mesh lattices of mpm_sdf_shape_from_mesh --, with
// the impulse each body receives added to the accumulators of the contact impulses.  Membership and normal come from the
// pair generator's own functions (collider_inside, collider_sdf, mesh_sdf): both coupling paths agree about where a
// body's surface is.
#pragma once
#include "mpm_contact_dev.h"
#include "mpm_device.h"
#include "mpm_step.h"

namespace mpm {

struct GridBody {
    Collider c;        // pose, dimensions, spatial velocity and accumulator index (a mesh body: kind and dims unused)
    int mode;          // 0 fixed, 1 slip while approaching, 2 slip whenever inside (GridCollider::mode)
    float friction;
    int mesh;          // index into GridBodyTable::mesh, or -1: an analytic body
    float bound;       // no point of the body is farther from c.p (infinite for a half-space)
};
// The table lives in device memory (2 KB of bodies, 2.5 KB of lattices: too much to ride next to DP in the kernel
// arguments); mpm_set_grid_bodies refreshes it.  Every lane reads the same entry: the loads are scalar.
struct GridBodyTable {
    int n;
    int pad[3];
    GridBody b[MAX_GRID_COLLIDERS];
    MeshCollider mesh[MAX_GRID_COLLIDERS];
};

// Instances by what the table needs (KINDS bit 0: an ellipsoid, whose FP64 nearest-point solve costs registers; bit 1: a
// mesh body, which reads lattices), as the pair kernels have their <ELL> and <MESH> instances.  k_grid<1>'s launch
// geometry; `body_acc` / `n_bodies`: the accumulators of k_ct_impulse and k_pin.
template <int KINDS>
__global__ __launch_bounds__(256) void k_grid_bodies(DP p, const GridBodyTable* __restrict__ gb, long long* body_acc, int n_bodies) {
    constexpr int MODE = 1;
    constexpr bool ELL = (KINDS & 1) != 0, MESH = (KINDS & 2) != 0;
#define MPM_GRID_BODIES 1
#include "mpm_grid_update.inc"
#undef MPM_GRID_BODIES
}

}  // namespace mpm
