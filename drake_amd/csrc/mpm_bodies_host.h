// Host side of what acts on the cloth from outside: fixed constraints (pins on moving bodies), the analytic colliders of
// the grid update and its rigid bodies -- what the entry points in mpm_engine.hip call once their arguments are checked.
// Included by mpm_engine.hip after mpm_host.h, mpm_io.h and mpm_contact.h.
#pragma once
#include <memory>
#include <unordered_map>
#include <unordered_set>

#include "mpm_contact.h"
#include "mpm_host.h"
#include "mpm_io.h"

// ---- anchors: springs and cords from cloth vertices to rigid bodies (mpm_set_anchors, mpm_get_anchors, mpm_anchor_forces,
// mpm_anchor_state, mpm_anchors_max_stable_dt, mpm_anchor_point; mpm_anchors.h) ----
// The table `t` with its limit and the caller's anchors put in force: new device arrays, upload, swap.  The caller has
// settled the owed substeps.  A failure changes nothing: the new buffers go, the table in force stays.
static int anchors_swap(mpm_engine* e, AnchorTable& t, float max_dt, size_t n, const mpm_anchor_t* anchors) {
    static_assert(sizeof(AnchorRecord) == sizeof(AnchorRec) && sizeof(AnchorOne) == sizeof(AnchorRec) && sizeof(AnchorRec) == 32,
                  "anchor record layouts differ");
    mpm_engine::Anchors next;
    FreshArrays fresh(e);
    if (int rc = rows_upload(e, fresh, t, &next.args)) return rc;
    if (n) {   // (k_anchor_energy's records, behind the table's)
        AnchorRec* d_one = nullptr;
        if (int rc = fresh.alloc(&d_one, n, false)) return rc;
        H2D(e, d_one, t.one.data(), n * sizeof(AnchorRec));
        next.d_one = d_one;
    }
    rows_free(e, e->anchors.args);
    AnchorRec* o_one = const_cast<AnchorRec*>(e->anchors.d_one);
    e->dfree(o_one);
    next.set.assign(anchors, anchors + n);
    next.max_dt = max_dt;
    next.unresolved = t.unresolved;
    next.d_pose = e->anchors.d_pose;   // (the pose table outlives the anchor tables: anchors_ready sizes it)
    next.cap_pose = e->anchors.cap_pose;
    e->anchors = next;
    fresh.commit();
    return 0;
}
// mpm_set_anchors in three steps: the table on the host, its limit from the vertices' masses, the swap.  A body without
// a motion yet leaves its records unresolved: anchors_ready lays the table out again once every body has its slot.
static int set_anchors(mpm_engine* e, size_t n, const mpm_anchor_t* anchors) {
    static_assert(sizeof(Anchor) == sizeof(mpm_anchor_t) && sizeof(Anchor) == 36, "anchor layouts differ");
    const Anchor* A = reinterpret_cast<const Anchor*>(anchors);
    const std::string refusal = anchor_table_refusal(A, n, e->nv);
    if (!refusal.empty()) return fail(MPM_ERR_INVALID, refusal);
    REQUIRE(e->np < (size_t)1 << 31, "anchors: too many particles");
    const std::vector<uint32_t>& mb = e->pin.motion_body;
    auto slot_of = [&](uint32_t body) {
        const auto it = std::find(mb.begin(), mb.end(), body);
        return it != mb.end() ? (uint32_t)(it - mb.begin()) : ANCHOR_NO_SLOT;
    };
    AnchorTable t;
    std::string why;
    if (!anchor_table(A, n, e->nf, e->nv, ANCHOR_SLICE, slot_of, t, why)) return fail(MPM_ERR_INVALID, why);
    // substeps that mpm_run_substeps deferred are owed with the table they were enqueued with
    if (int rc = settle(e)) return rc;
    float max_dt = INFINITY;
    if (n) {
        std::vector<float> mass;
        if (int rc = vertex_masses(e, mass)) return rc;
        double W, G;
        anchor_rates(t, mass.data(), e->nf, &W, &G);
        max_dt = link_limit(W, G);
    }
    return anchors_swap(e, t, max_dt, n, anchors);
}
// What a launch of the anchor kernels needs: every anchor's body has a motion (MPM_ERR_INVALID otherwise, before
// anything is enqueued), the table carries the motion slots, the pose table holds every slot and k_pin's ticket exists.
static int anchors_ready(mpm_engine* e) {
    mpm_engine::Anchors& an = e->anchors;
    if (!an.on()) return 0;
    mpm_engine::PinState& ps = e->pin;
    if (an.unresolved) {
        std::unordered_set<uint32_t> have(ps.motion_body.begin(), ps.motion_body.end());
        for (const mpm_anchor_t& q : an.set)
            if (!have.count(q.body))
                return fail(MPM_ERR_INVALID, "anchor on body " + std::to_string(q.body) + ", which has no motion: call mpm_set_body_motions first");
        const std::vector<mpm_anchor_t> again = an.set;   // (no substep has been enqueued with the unresolved table)
        if (int rc = set_anchors(e, again.size(), again.data())) return rc;
    }
    if (an.cap_pose < ps.cap_mot) {
        HIP_TRY(hipStreamSynchronize(e->stream));   // (earlier substeps may still read the old table)
        e->dfree(an.d_pose);
        an.cap_pose = 0;
        if (int rc = e->dalloc(&an.d_pose, ps.cap_mot, true)) return rc;
        an.cap_pose = ps.cap_mot;
    }
    if (!ps.d_ticket)
        if (int rc = e->dalloc(&ps.d_ticket, 1, true)) return rc;
    return 0;
}
// the table as a launch reads it, behind k_anchor_pose on the stream
static AnchorArgs anchors_posed(mpm_engine* e) {
    const mpm_engine::PinState& ps = e->pin;
    AnchorArgs a = e->anchors.args;
    a.pose = e->anchors.d_pose;
    a.n_mot = (int)ps.motion_body.size();
    hipLaunchKernelGGL(k_anchor_pose, dim3(((unsigned)a.n_mot + 63u) / 64u), dim3(64), 0, e->stream, (const BodyMotionDev*)ps.d_mot, a.n_mot,
                       e->anchors.d_pose);
    return a;
}

static int anchor_forces(mpm_engine* e, float* f_out) {
    if (!e->anchors.on()) {
        std::memset(f_out, 0, e->nv * 12);
        return 0;
    }
    if (int rc = anchors_ready(e)) return rc;
    return rows_eval(e, k_anchor_eval, anchors_posed(e), f_out);
}

// One double term, one float length and one float point per anchor from the device, the terms added here in anchor order:
// a fixed order, no atomics (as link_energy)
static int anchor_state(mpm_engine* e, double* energy_out, float* length_out, float* point_out, double* impulse_quantum_out) {
    const size_t n = e->anchors.set.size();
    double sum = 0.0;
    if (n) {
        if (int rc = anchors_ready(e)) return rc;
        if (int rc = e->stage(n * 24)) return rc;
        double* d_term = (double*)e->d_stage;
        float* d_len = (float*)(d_term + n);
        float* d_point = d_len + n;
        const AnchorArgs a = anchors_posed(e);
        hipLaunchKernelGGL(k_anchor_energy, dim3(((unsigned)n + 255u) / 256u), dim3(256), 0, e->stream, e->dp, e->anchors.d_one, (int)n,
                           a.pose, a.n_mot, d_term, d_len, d_point);
        std::vector<double> term(n);
        D2H(e, term.data(), d_term, n * 8);
        if (length_out) D2H(e, length_out, d_len, n * 4);
        if (point_out) D2H(e, point_out, d_point, n * 12);
        for (size_t i = 0; i < n; ++i) sum += term[i];
    }
    if (energy_out) *energy_out = sum;
    // (what mpm_external_body_force_to_host multiplies the integer sums by)
    if (impulse_quantum_out) *impulse_quantum_out = e->cb.imp_unfix > 0.0 ? e->cb.imp_unfix : e->dp.unfix_p;
    return 0;
}

// host code only: pin_pose and anchor_point, compiled for the host
static void anchor_point_host(const mpm_body_motion_t* m, double t, const float p_BQ[3], float y[3], float v_Q[3]) {
    BodyMotionDev r{};
    for (int i = 0; i < 3; ++i) {
        r.p[i] = m->p_WB[i];
        r.v[i] = m->v[i];
        r.w[i] = m->w[i];
    }
    for (int i = 0; i < 9; ++i) r.R[i] = m->R_WB[i];
    double pt[3], Rt[9];
    pin_pose(r, t, pt, Rt);
    float yy[3], vq[3];
    anchor_point(pt, Rt, r.v, r.w, p_BQ, yy, vq);
    for (int i = 0; i < 3; ++i) {
        if (y) y[i] = yy[i];
        if (v_Q) v_Q[i] = vq[i];
    }
}

// ---- fixed constraints: checks of the substep entry points ------------------------------------------------------------
// Every pin's body has a motion (MPM_ERR_INVALID otherwise, before anything is enqueued), and the device table is the
// current pin set with each pin's motion slot resolved.  The same for the anchors (anchors_ready).
static int pins_ready(mpm_engine* e) {
    mpm_engine::PinState& ps = e->pin;
    if (int rc = anchors_ready(e)) return rc;
    if (ps.set.empty()) return 0;
    std::unordered_map<uint32_t, uint32_t> slot_of;
    for (size_t k = 0; k < ps.motion_body.size(); ++k) slot_of[ps.motion_body[k]] = (uint32_t)k;
    for (const mpm_pin_t& q : ps.set)
        if (!slot_of.count(q.body))
            return fail(MPM_ERR_INVALID, "pin on body " + std::to_string(q.body) + ", which has no motion: call mpm_set_body_motions first");
    if (!ps.table_dirty) return 0;
    std::vector<PinDev> t(ps.set.size());
    for (size_t k = 0; k < t.size(); ++k) {
        const mpm_pin_t& q = ps.set[k];
        t[k] = PinDev{(uint32_t)e->dp.NfG + q.vertex, slot_of[q.body], q.body, {q.p_BQ[0], q.p_BQ[1], q.p_BQ[2]}};
    }
    if (t.size() > ps.cap_pins) {
        HIP_TRY(hipStreamSynchronize(e->stream));   // (earlier substeps may still read the old table)
        e->dfree(ps.d_pins);
        ps.cap_pins = 0;
        if (int rc = e->dalloc(&ps.d_pins, t.size(), false)) return rc;
        ps.cap_pins = t.size();
    }
    if (!ps.d_ticket)
        if (int rc = e->dalloc(&ps.d_ticket, 1, true)) return rc;
    H2D(e, ps.d_pins, t.data(), t.size() * sizeof(PinDev));
    ps.table_dirty = false;
    return 0;
}

// ---- fixed constraints (mpm_set_pins, mpm_set_body_motions, mpm_pins_inside_collider) --------------------------------
static int set_pins(mpm_engine* e, size_t n, const mpm_pin_t* pins) {
    std::vector<uint8_t> seen(e->nv, 0);
    for (size_t k = 0; k < n; ++k) {
        REQUIRE(pins[k].vertex < e->nv, "pin vertex out of range");
        REQUIRE(!seen[pins[k].vertex], "a vertex is pinned twice");
        seen[pins[k].vertex] = 1;
        REQUIRE(finite_n(pins[k].p_BQ, 3), "pin p_BQ not finite");
    }
    e->pin.set.assign(pins, pins + n);
    e->pin.table_dirty = true;
    return 0;
}

static int set_body_motions(mpm_engine* e, size_t n, const mpm_body_motion_t* m) {
    std::unordered_set<uint32_t> bodies;
    for (size_t k = 0; k < n; ++k) {
        REQUIRE(bodies.insert(m[k].body).second, "a body appears twice in one mpm_set_body_motions");
        REQUIRE(finite_n(m[k].p_WB, 3) && finite_n(m[k].v, 3) && finite_n(m[k].w, 3), "body motion not finite");
        REQUIRE(is_rotation(m[k].R_WB), "body motion: R_WB is not a rotation");
    }
    mpm_engine::PinState& ps = e->pin;
    std::vector<uint32_t> slot(n);
    size_t n_slots = ps.motion_body.size();
    for (size_t k = 0; k < n; ++k) {
        const auto it = std::find(ps.motion_body.begin(), ps.motion_body.end(), m[k].body);
        slot[k] = it != ps.motion_body.end() ? (uint32_t)(it - ps.motion_body.begin()) : (uint32_t)n_slots++;
    }
    if (n_slots > ps.cap_mot) {   // grow, keeping the clocks of the motions already set
        const size_t cap = std::max<size_t>(n_slots, std::max<size_t>(16, ps.cap_mot * 2));
        BodyMotionDev* bigger = nullptr;
        if (int rc = e->dalloc(&bigger, cap, true)) return rc;
        if (ps.d_mot)
            HIP_TRY(hipMemcpyAsync(bigger, ps.d_mot, ps.motion_body.size() * sizeof(BodyMotionDev), hipMemcpyDeviceToDevice, e->stream));
        HIP_TRY(hipStreamSynchronize(e->stream));
        e->dfree(ps.d_mot);
        ps.d_mot = bigger;
        ps.cap_mot = cap;
    }
    for (size_t k = 0; k < n; ++k)
        if (slot[k] >= ps.motion_body.size()) ps.motion_body.push_back(m[k].body);
    std::vector<BodyMotionDev> rec(n);
    for (size_t k = 0; k < n; ++k) {
        BodyMotionDev& r = rec[k];
        r = BodyMotionDev{};
        for (int i = 0; i < 3; ++i) {
            r.p[i] = m[k].p_WB[i];
            r.v[i] = m[k].v[i];
            r.w[i] = m[k].w[i];
        }
        for (int i = 0; i < 9; ++i) r.R[i] = m[k].R_WB[i];
        r.t = 0.0;
        HIP_TRY(hipMemcpyAsync(ps.d_mot + slot[k], &rec[k], sizeof(BodyMotionDev), hipMemcpyHostToDevice, e->stream));
    }
    HIP_TRY(hipStreamSynchronize(e->stream));
    ps.table_dirty = true;   // (a pin whose body has just got its first motion is resolved at the next substep)
    return 0;
}

static int pins_inside_collider(mpm_engine* e, const mpm_collider_t* shape, uint32_t body, const float p_WB[3],
                                const float R_WB[9], size_t* n_added) {
    REQUIRE(finite_n(p_WB, 3), "body pose not finite");
    REQUIRE(is_rotation(R_WB), "R_WB is not a rotation");
    if (int rc = validate_colliders(1, shape)) return rc;
    const size_t nv = e->nv;
    std::vector<float> x(nv * 3), phi(nv), grad(nv * 3);
    if (nv) {
        if (int rc = download_original_vertices(e, x.data())) return rc;
        if (int rc = collider_signed_distance(e, shape, nv, x.data(), phi.data(), grad.data())) return rc;
    }
    mpm_engine::PinState& ps = e->pin;
    std::vector<uint8_t> pinned(nv, 0);
    for (const mpm_pin_t& q : ps.set) pinned[q.vertex] = 1;
    std::vector<mpm_pin_t> add;
    for (size_t v = 0; v < nv; ++v) {
        if (!(phi[v] <= 0.f) || pinned[v]) continue;
        mpm_pin_t q{(uint32_t)v, body, {0.f, 0.f, 0.f}};
        const double d[3] = {(double)x[v * 3] - p_WB[0], (double)x[v * 3 + 1] - p_WB[1], (double)x[v * 3 + 2] - p_WB[2]};
        for (int i = 0; i < 3; ++i)
            q.p_BQ[i] = (float)((double)R_WB[i] * d[0] + (double)R_WB[3 + i] * d[1] + (double)R_WB[6 + i] * d[2]);
        add.push_back(q);
    }
    if (n_added) *n_added = 0;
    REQUIRE(!add.empty(), "no vertex that is not pinned already lies inside the shape");
    ps.set.insert(ps.set.end(), add.begin(), add.end());
    ps.table_dirty = true;
    if (n_added) *n_added = add.size();
    return 0;
}

// ---- analytic colliders of the grid update ---------------------------------------------------
// The reference's compile-time scenes (cuda_mpm_kernels.cuh:673-774) as tables; MPM_BC_TABLE selects
// the table set with mpm_set_grid_colliders.
static GridCollider gc_sphere(float x, float y, float z, float r, int mode, float friction) {
    GridCollider c{};
    c.shape = 0; c.mode = mode;
    c.p[0] = x; c.p[1] = y; c.p[2] = z;
    c.radius = r; c.friction = friction;
    return c;
}
static int grid_collider_preset(int bc, float sdf_friction, GridColliders* out) {
    out->n = 0;
    switch (bc) {
        case -1: return 0;
        case 0:   // one sphere, slip, active while approaching (:673-692)
            out->c[out->n++] = gc_sphere(.5f, .5f, .5f, .08f, 1, sdf_friction);
            return 0;
        case 1:   // two fixed spheres (:694-734)
            out->c[out->n++] = gc_sphere(.38f, .38f, .75f, .04f, 0, sdf_friction);
            out->c[out->n++] = gc_sphere(.38f, .62f, .75f, .04f, 0, sdf_friction);
            return 0;
        case 2: { // plane z < 0.11, slip, active whenever inside (:737-749)
            GridCollider c{};
            c.shape = 1; c.mode = 2;
            c.p[2] = .11f; c.n[2] = 1.f; c.friction = sdf_friction;
            out->c[out->n++] = c;
            return 0;
        }
        case 3: { // four pin spheres (:752-774)
            const float span[2] = {.3f, .7f};
            for (int k = 0; k < 4; ++k) out->c[out->n++] = gc_sphere(span[k % 2], span[k / 2], .5f, .02f, 0, sdf_friction);
            return 0;
        }
        default: return -1;
    }
}
// MPM_BC_BODIES: n = -1 stands for "the engine's body table" (launch_grid picks k_grid_bodies); an empty table is mpm_bc = -1
static int grid_colliders_for(mpm_engine* e, int bc, GridColliders* out) {
    if (bc == MPM_BC_BODIES) {
        *out = GridColliders{};
        out->n = e->grid_bodies.empty() ? 0 : -1;
        return 0;
    }
    if (bc == MPM_BC_TABLE) {
        *out = e->grid_colliders;
        return 0;
    }
    if (grid_collider_preset(bc, e->mat.sdf_friction, out))
        return fail(MPM_ERR_INVALID, "mpm_bc must be -1, 0, 1, 2, 3, MPM_BC_TABLE or MPM_BC_BODIES");
    return 0;
}

static int set_grid_colliders(mpm_engine* e, size_t n, const mpm_grid_collider_t* colliders) {
    if (e->finalized) {
        // substeps that mpm_run_substeps deferred are owed with the table they were enqueued with
        if (int rc = use(e)) return rc;
        if (int rc = settle(e)) return rc;
    }
    GridColliders gc{};
    for (size_t k = 0; k < n; ++k) {
        const mpm_grid_collider_t& c = colliders[k];
        REQUIRE(c.shape == MPM_GC_SPHERE || c.shape == MPM_GC_HALF_SPACE, "unknown grid collider shape");
        REQUIRE(c.mode >= MPM_GC_FIXED && c.mode <= MPM_GC_SLIP, "unknown grid collider mode");
        if (c.shape == MPM_GC_SPHERE) REQUIRE(c.radius > 0.f, "sphere radius must be positive");
        if (c.shape == MPM_GC_HALF_SPACE) {
            const float l = c.n[0] * c.n[0] + c.n[1] * c.n[1] + c.n[2] * c.n[2];
            REQUIRE(std::fabs(l - 1.f) < 1e-4f, "half-space normal must be a unit vector");
        }
        std::memcpy(&gc.c[k], &c, sizeof(GridCollider));
        if (c.friction < 0.f) gc.c[k].friction = e->mat.sdf_friction;
    }
    gc.n = (int)n;
    e->grid_colliders = gc;
    e->grid_colliders_version += 1;
    return 0;
}

static int grid_collider_preset_out(int mpm_bc, float sdf_friction, mpm_grid_collider_t* out, size_t capacity, size_t* n_out) {
    GridColliders gc{};
    if (grid_collider_preset(mpm_bc, sdf_friction, &gc)) return fail(MPM_ERR_INVALID, "mpm_bc must be -1, 0, 1, 2 or 3");
    *n_out = (size_t)gc.n;
    REQUIRE((size_t)gc.n <= capacity && (gc.n == 0 || out), "output array too small");
    for (int k = 0; k < gc.n; ++k) std::memcpy(&out[k], &gc.c[k], sizeof(GridCollider));
    return 0;
}

// ---- rigid bodies of the grid update (mpm_set_grid_bodies, mpm_get_grid_bodies; k_grid_bodies in mpm_grid_bodies.h) ----
// no point of the body is farther from its origin than this (k_grid_bodies' test per wave); a little slack for the float
// evaluation, infinite when the dimensions say nothing (a half-space; NaN or infinite dimensions of kinds 1-3)
static float grid_body_bound(const mpm_grid_body_t& b, const SdfShape* sh) {
    double r;
    if (sh) {
        r = 0.0;
        for (int a = 0; a < 3; ++a) {
            const double m = std::max(std::fabs((double)sh->lo[a]), std::fabs((double)sh->hi[a]));
            r += m * m;
        }
        r = std::sqrt(r);
    } else {
        const double d0 = std::fabs((double)b.shape.dims[0]), d1 = std::fabs((double)b.shape.dims[1]),
                     d2 = std::fabs((double)b.shape.dims[2]);
        switch (b.shape.kind) {
            case MPM_COLLIDER_SPHERE: r = d0; break;
            case MPM_COLLIDER_BOX: r = std::sqrt(d0 * d0 + d1 * d1 + d2 * d2); break;
            case MPM_COLLIDER_CAPSULE: r = d0 + d1; break;
            case MPM_COLLIDER_CYLINDER: r = std::sqrt(d0 * d0 + d1 * d1); break;
            case MPM_COLLIDER_ELLIPSOID: r = std::max(d0, std::max(d1, d2)); break;
            default: return INFINITY;
        }
    }
    r = r * (1.0 + 1e-4) + 1e-6;
    return std::isfinite(r) && r < 1e30 ? (float)r : INFINITY;
}

static int set_grid_bodies(mpm_engine* e, size_t n, const mpm_grid_body_t* bodies) {
    for (size_t k = 0; k < n; ++k) {
        const mpm_grid_body_t& b = bodies[k];
        if (b.sdf_shape == MPM_GB_NO_MESH) {
            if (int rc = validate_colliders(1, &b.shape)) return rc;
        } else {
            REQUIRE(b.sdf_shape < e->cb.shapes.size(), "grid body: unknown shape id");
        }
        REQUIRE(b.mode >= MPM_GC_FIXED && b.mode <= MPM_GC_SLIP, "unknown grid body mode");
        REQUIRE(std::isfinite(b.friction), "grid body: friction not finite");
        REQUIRE(finite_n(b.shape.p_WB, 3) && finite_n(b.shape.v, 3) && finite_n(b.shape.w, 3), "grid body: pose or velocity not finite");
        REQUIRE(is_rotation(b.shape.R_WB), "grid body: R_WB is not a rotation");
    }
    // substeps that mpm_run_substeps deferred are owed with the table they were enqueued with
    if (int rc = settle(e)) return rc;
    auto table = std::make_unique<GridBodyTable>();
    std::memset(table.get(), 0, sizeof(GridBodyTable));
    int kinds = 0, n_mesh = 0;
    for (size_t k = 0; k < n; ++k) {
        const mpm_grid_body_t& b = bodies[k];
        GridBody& d = table->b[k];
        std::memcpy(&d.c, &b.shape, sizeof(Collider));
        d.mode = b.mode;
        d.friction = b.friction < 0.f ? e->mat.sdf_friction : b.friction;
        d.mesh = -1;
        const SdfShape* sh = nullptr;
        if (b.sdf_shape != MPM_GB_NO_MESH) {
            sh = &e->cb.shapes[b.sdf_shape];
            mpm_sdf_collider_t sc{};
            sc.shape = b.sdf_shape;
            sc.body = b.shape.body;
            std::memcpy(sc.p_WB, b.shape.p_WB, sizeof(sc.p_WB));
            std::memcpy(sc.R_WB, b.shape.R_WB, sizeof(sc.R_WB));
            std::memcpy(sc.v, b.shape.v, sizeof(sc.v));
            std::memcpy(sc.w, b.shape.w, sizeof(sc.w));
            table->mesh[n_mesh] = mesh_collider(*sh, sc);
            d.mesh = n_mesh++;
            d.c.kind = 0;   // (kind and dims of a mesh body are not read)
            kinds |= 2;
        } else if (b.shape.kind == MPM_COLLIDER_ELLIPSOID) {
            kinds |= 1;
        }
        d.bound = grid_body_bound(b, sh);
    }
    table->n = (int)n;
    if (n) {
        if (!e->d_grid_bodies)
            if (int rc = e->dalloc(&e->d_grid_bodies, 1, true)) return rc;
        // (stream-ordered, and a synchronisation point: the kernels enqueued so far have read the old table)
        H2D(e, e->d_grid_bodies, table.get(), sizeof(GridBodyTable));
    }
    e->grid_bodies.assign(bodies, bodies + n);
    e->grid_bodies_kinds = kinds;
    e->grid_colliders_version += 1;
    return 0;
}
