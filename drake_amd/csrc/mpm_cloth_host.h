// Host side of the per-cloth features: cloth materials, external force fields, row tables, bending stiffness, links,
// pressure, shell bending and its creases, damping, the weave, tearing, breakable links, the rest shape and the per-cloth report -- what the entry points in mpm_engine.hip call once their
// arguments are checked.
// Included by mpm_engine.hip after mpm_host.h and mpm_io.h.
#pragma once
#include "mpm_host.h"
#include "mpm_io.h"

// ---- cloth materials ------------------------------------------------------------------------------------------------------
static mpm_cloth_material_t engine_cloth_material(const mpm_engine* e) {
    const mpm_material_t& em = e->mat;
    return mpm_cloth_material_t{em.youngs_modulus, em.poisson_ratio, em.density, em.gamma, em.K, em.c_F};
}
// The Lame parameters from Young's modulus and Poisson's ratio, in float: the one place that forms them (DP::M at Finalize,
// k_fem_mat's table, the damping coefficients, mpm_cloth_energy_density), so that all of them hold the same bits.
static void lame(float youngs_modulus, float poisson_ratio, float* mu, float* lambda) {
    *mu = youngs_modulus / (2.f * (1.f + poisson_ratio));
    *lambda = youngs_modulus * poisson_ratio / ((1.f + poisson_ratio) * (1.f - 2.f * poisson_ratio));
}
// A multi-material engine at Finalize, after the volumes are in place: k_fem_mat's table (the Lame parameters formed as
// for the engine's material) and every particle's q[0].w scaled to its mass.  cloth_of_pid: [original id] cloth.
static int init_cloth_materials(mpm_engine* e, const std::vector<uint8_t>& cloth_of_pid) {
    std::vector<ClothMat> t(e->cloths.size());
    for (size_t c = 0; c < t.size(); ++c) {
        const mpm_cloth_material_t& m = e->cloths[c].m;
        float mu, lambda;
        lame(m.youngs_modulus, m.poisson_ratio, &mu, &lambda);
        t[c] = ClothMat{mu, lambda, m.gamma, m.K, m.c_F, m.density, 0.f, 0.f};
    }
    if (int rc = e->dalloc(&e->d_cloth_mat, t.size(), false)) return rc;
    H2D(e, e->d_cloth_mat, t.data(), t.size() * sizeof(ClothMat));
    uint8_t* d_cloth = nullptr;
    if (int rc = e->dalloc(&d_cloth, e->np, false)) return rc;
    H2D(e, d_cloth, cloth_of_pid.data(), e->np);
    hipLaunchKernelGGL(k_init_masses, dim3(e->g_np), dim3(256), 0, e->stream, e->dp, (const ClothMat*)e->d_cloth_mat,
                       (const uint8_t*)d_cloth);
    HIP_TRY(hipStreamSynchronize(e->stream));
    e->dfree(d_cloth);
    return 0;
}

// the Lame parameters of cloth c as the elastic kernels use them (init_cloth_materials; DP::M of a single-material engine)
static void cloth_lame(const mpm_engine* e, size_t c, float* mu, float* lambda) {
    if (!e->multi_mat) {
        *mu = e->dp.M.mu;
        *lambda = e->dp.M.lambda;
        return;
    }
    lame(e->cloths[c].m.youngs_modulus, e->cloths[c].m.poisson_ratio, mu, lambda);
}

// ---- external force fields (mpm_set_force_fields, mpm_get_force_fields, mpm_force_field_acceleration; mpm_fields.h) ----
static int validate_force_fields(size_t n, const mpm_force_field_t* f) {
    static_assert(sizeof(ForceField) == sizeof(mpm_force_field_t), "force field layouts differ");
    REQUIRE(n <= (size_t)MAX_FORCE_FIELDS, "too many force fields (at most 8)");
    REQUIRE(n == 0 || f, "null force field array");
    for (size_t k = 0; k < n; ++k) {
        const mpm_force_field_t& q = f[k];
        REQUIRE(q.kind >= MPM_FF_ACCEL && q.kind <= MPM_FF_NORMAL_DRAG, "force field: unknown kind");
        REQUIRE((q.flags & ~(uint32_t)(MPM_FF_QUADRATIC | MPM_FF_REGION)) == 0, "force field: unknown flags");
        REQUIRE(std::isfinite(q.gamma) && finite_n(q.u0, 3) && finite_n(q.G, 9) && finite_n(q.x0, 3) && finite_n(q.lo, 3) &&
                    finite_n(q.hi, 3),
                "force field: a number is not finite");
        REQUIRE(q.gamma >= 0.f, "force field: gamma < 0");
        REQUIRE(q.lo[0] <= q.hi[0] && q.lo[1] <= q.hi[1] && q.lo[2] <= q.hi[2], "force field: lo > hi");
    }
    return 0;
}

static int set_force_fields(mpm_engine* e, size_t n, const mpm_force_field_t* fields) {
    // substeps that mpm_run_substeps deferred are owed with the table they were enqueued with
    if (int rc = settle(e)) return rc;
    double gamma = 0.0;
    if (n) {
        ForceFieldTable table;
        std::memset(&table, 0, sizeof(table));
        table.n = (int)n;
        std::memcpy(table.f, fields, n * sizeof(ForceField));
        for (size_t k = 0; k < n; ++k)
            if (fields[k].kind != MPM_FF_ACCEL && !(fields[k].flags & MPM_FF_QUADRATIC)) gamma += (double)fields[k].gamma;
        if (!e->d_force_fields)
            if (int rc = e->dalloc(&e->d_force_fields, 1, true)) return rc;
        // (stream-ordered, and a synchronisation point: the kernels enqueued so far have read the old table)
        H2D(e, e->d_force_fields, &table, sizeof(table));
    }
    e->force_fields.assign(fields, fields + n);
    e->force_fields_gamma = gamma;
    return 0;
}

// host code only: no device is touched
static int force_field_accelerations(const mpm_force_field_t* fields, size_t n_fields, size_t n, const float* x, const float* v,
                                     const float* director, float* acc_out) {
    const ForceField* f = reinterpret_cast<const ForceField*>(fields);
    const float zero[3] = {0.f, 0.f, 0.f};
    for (size_t k = 0; k < n; ++k)
        force_field_acceleration(f, (int)n_fields, x + 3 * k, v + 3 * k, director ? director + 3 * k : zero, director != nullptr,
                                 acc_out + 3 * k);
    return 0;
}

// ---- vertex row tables on the device (mpm_row_table.h): what bending, hinge damping and links share ----
// one lane per row, 256 to a block
static dim3 rows_grid(int n_rows) { return dim3(((unsigned)n_rows + 255u) / 256u); }
// A table's three arrays as new device arrays in `fresh`, and `out` (BendArgs, LinkArgs) filled; a table without rows
// leaves `out` empty.  Stream-ordered, and a synchronisation point either way: the kernels enqueued so far have read the
// old table.  (A table whose rows all have width 0 has no record to copy: a cloth with k > 0 and no hinge.)
template <class Args, class Record>
static int rows_upload(mpm_engine* e, FreshArrays& fresh, const RowTable<Record>& t, Args* out) {
    static_assert(sizeof(Record) == sizeof(*out->ent), "record layouts differ");
    *out = Args{};
    if (t.row_pid.empty()) {
        HIP_TRY(hipStreamSynchronize(e->stream));
        return 0;
    }
    int* d_row = nullptr;
    unsigned* d_off = nullptr;
    Record* d_ent = nullptr;
    if (int rc = fresh.alloc(&d_row, t.row_pid.size(), false)) return rc;
    if (int rc = fresh.alloc(&d_off, t.slice_off.size(), false)) return rc;
    if (int rc = fresh.alloc(&d_ent, t.ent.size(), false)) return rc;
    H2D(e, d_row, t.row_pid.data(), t.row_pid.size() * sizeof(int));
    H2D(e, d_off, t.slice_off.data(), t.slice_off.size() * sizeof(unsigned));
    if (!t.ent.empty()) H2D(e, d_ent, t.ent.data(), t.ent.size() * sizeof(Record));
    *out = Args{d_row, d_off, reinterpret_cast<decltype(out->ent)>(d_ent), (int)t.row_pid.size()};
    return 0;
}
// ... and the arrays of the table that was in force released (the caller assigns the new one)
template <class Args>
static void rows_free(mpm_engine* e, const Args& a) {
    void *row = (void*)a.row_pid, *off = (void*)a.slice_off, *ent = (void*)a.ent;   // (dfree looks the address up)
    e->dfree(row);
    e->dfree(off);
    e->dfree(ent);
}
// mpm_bending_forces, mpm_link_forces: a table's rows on the current state through its *_eval kernel, in original vertex
// order; zero for the vertices without a row, and for all of them where the table is empty
template <class Args>
static int rows_eval(mpm_engine* e, void (*kernel)(DP, Args, float*), const Args& a, float* f_out) {
    const size_t bytes = e->nv * 12;
    if (a.n_rows <= 0) {
        std::memset(f_out, 0, bytes);
        return 0;
    }
    if (int rc = e->stage(bytes)) return rc;
    HIP_TRY(hipMemsetAsync(e->d_stage, 0, bytes, e->stream));
    hipLaunchKernelGGL(kernel, rows_grid(a.n_rows), dim3(256), 0, e->stream, e->dp, a, (float*)e->d_stage);
    D2H(e, f_out, e->d_stage, bytes);
    return 0;
}

// ---- bending stiffness (mpm_set_bending, mpm_get_bending, mpm_bending_forces, mpm_bending_max_stable_dt,
// mpm_bending_matrix; mpm_bending.h) ----
static void damping_limit(mpm_engine* e);
// host code only: no device is touched
static int bending_matrix_out(const float* pos, size_t n_verts, const int32_t* indices, size_t n_faces, size_t* row_offsets,
                              int32_t* cols, double* vals, size_t capacity, size_t* nnz_out) {
    BendCsr Q;
    std::string why;
    if (!bending_matrix(pos, n_verts, indices, n_faces, 0, Q, why)) return fail(MPM_ERR_INVALID, why);
    if (row_offsets) std::copy(Q.off.begin(), Q.off.end(), row_offsets);
    const size_t n = std::min(capacity, Q.col.size());
    std::copy(Q.col.begin(), Q.col.begin() + (long)n, cols);
    std::copy(Q.val.begin(), Q.val.begin() + (long)n, vals);
    if (nnz_out) *nnz_out = Q.col.size();
    return 0;
}

// The stability limit of an explicit step against a rate omega (dt * omega <= 2): the float not above 2 / omega, rounded
// towards zero so that it is never above the bound; INFINITY when nothing limits the step (omega not positive).
static float stable_dt_limit(double omega) {
    if (!(omega > 0.0)) return INFINITY;
    const double lim = 2.0 / omega;
    float dt = (float)lim;
    if ((double)dt > lim) dt = std::nextafterf(dt, 0.f);
    return dt;
}
// Every vertex's mass as ParticleToGrid forms it: q[0].w x DP::M.density, both floats, by original vertex id.  One gather:
// with `w_all` every particle's q[0].w in original order (faces, then vertices) is handed out too.
static int vertex_masses(mpm_engine* e, std::vector<float>& mass, std::vector<float>* w_all = nullptr) {
    int* iota = nullptr;
    if (int rc = device_iota(e, &iota)) return rc;
    mass.resize(e->nv);
    const float* w = mass.data();
    if (w_all) {
        w_all->resize(e->np);
        if (int rc = gather_to_host<F_VOL>(e, w_all->data(), e->np, iota)) return rc;
        w = w_all->data() + e->nf;
    } else if (int rc = gather_to_host<F_VOL>(e, mass.data(), e->nv, iota + e->nf)) {
        return rc;
    }
    for (size_t i = 0; i < e->nv; ++i) mass[i] = std::fabs(w[i]) * e->dp.M.density;
    return 0;
}

// mpm_bending_max_stable_dt of a table (bending_table's rows) on the vertices' masses: symplectic Euler on the lumped
// system needs dt * omega <= 2, with Gershgorin's bound omega^2 <= max_i (1 / m_i) sum_j |k Q_ij|
static float bending_limit(const BendTable& t, const std::vector<float>& mass, size_t nf) {
    return stable_dt_limit(std::sqrt(max_row_rate(t.abs_sum.data(), t.row_pid.size(), 1.0,
                                                  [&](size_t r) { return mass[(size_t)t.row_pid[r] - nf]; })));
}
// The table `t` with its limit and the caller's stiffnesses put in force: new device arrays, upload, swap.  The caller has
// settled the owed substeps.  A failure changes nothing: the new buffers go, the table in force stays.
static int bending_swap(mpm_engine* e, BendTable& t, float max_dt, size_t n_cloths, const float* stiffness) {
    const size_t n_rows = t.row_pid.size();
    mpm_engine::Bending next;
    FreshArrays fresh(e);
    if (int rc = rows_upload(e, fresh, t, &next.args)) return rc;
    rows_free(e, e->bend.args);
    next.k.assign(stiffness, stiffness + n_cloths);
    next.max_dt = max_dt;
    next.row_vertex.resize(n_rows);
    for (size_t r = 0; r < n_rows; ++r) next.row_vertex[r] = t.row_pid[r] - (int)e->nf;
    next.abs_sum.swap(t.abs_sum);
    e->bend = next;
    fresh.commit();
    return 0;
}
// mpm_set_bending in three steps: the table on the host, its limit from the vertices' masses, the swap
static int set_bending(mpm_engine* e, size_t n_cloths, const float* stiffness) {
    for (size_t c = 0; c < n_cloths; ++c)
        REQUIRE(std::isfinite(stiffness[c]) && stiffness[c] >= 0.f, "bending: a stiffness is negative or not finite");
    BendTable t;
    std::string why;
    if (!bending_table(e->cloths, e->h_rest.data(), e->h_idx.data(), e->nf, n_cloths, stiffness, BEND_SLICE, t, why))
        return fail(MPM_ERR_INVALID, why);
    // substeps that mpm_run_substeps deferred are owed with the stiffness they were enqueued with
    if (int rc = settle(e)) return rc;
    float max_dt = INFINITY;
    if (!t.row_pid.empty()) {
        std::vector<float> mass;
        if (int rc = vertex_masses(e, mass)) return rc;
        max_dt = bending_limit(t, mass, e->nf);
    }
    if (int rc = bending_swap(e, t, max_dt, n_cloths, stiffness)) return rc;
    damping_limit(e);   // (the hinge damping is beta k Q: its share of mpm_damping_max_stable_dt follows the new k)
    return 0;
}

static int bending_forces(mpm_engine* e, float* f_out) { return rows_eval(e, k_bend_eval, e->bend.args, f_out); }

// ---- links between cloth vertices (mpm_set_links, mpm_get_links, mpm_link_forces, mpm_link_energy,
// mpm_links_max_stable_dt; mpm_links.h) ----
// The table `t` with its limit and the caller's links put in force: new device arrays, upload, swap.  The caller has
// settled the owed substeps.  A failure changes nothing: the new buffers go, the table in force stays.
static void link_break_free(mpm_engine* e);
static int links_swap(mpm_engine* e, LinkTable& t, float max_dt, size_t n, const mpm_link_t* links) {
    static_assert(sizeof(LinkPair) == sizeof(float4), "link record layouts differ");
    mpm_engine::Links next;
    FreshArrays fresh(e);
    if (int rc = rows_upload(e, fresh, t, &next.args)) return rc;
    if (n) {   // (k_link_energy's records, behind the table's)
        float4* d_pair = nullptr;
        if (int rc = fresh.alloc(&d_pair, n, false)) return rc;
        H2D(e, d_pair, t.pair.data(), n * sizeof(float4));
        next.d_pair = d_pair;
    }
    rows_free(e, e->links.args);
    float4* o_pair = const_cast<float4*>(e->links.d_pair);
    e->dfree(o_pair);
    link_break_free(e);   // (the limits and flags go with the table they belonged to: `next` has none)
    next.set.assign(links, links + n);
    next.max_dt = max_dt;
    e->links = next;
    fresh.commit();
    return 0;
}
// mpm_set_links in three steps: the table on the host, its limit from the vertices' masses, the swap
static int set_links(mpm_engine* e, size_t n, const mpm_link_t* links) {
    static_assert(sizeof(Link) == sizeof(mpm_link_t), "link layouts differ");
    const Link* L = reinterpret_cast<const Link*>(links);
    const std::string refusal = link_table_refusal(L, n, e->nv);
    if (!refusal.empty()) return fail(MPM_ERR_INVALID, refusal);
    REQUIRE(e->np < (size_t)1 << 31, "links: too many particles");
    LinkTable t;
    std::string why;
    if (!link_table(L, n, e->nf, e->nv, LINK_SLICE, t, why)) return fail(MPM_ERR_INVALID, why);
    // substeps that mpm_run_substeps deferred are owed with the table they were enqueued with
    if (int rc = settle(e)) return rc;
    float max_dt = INFINITY;
    if (n) {
        std::vector<float> mass;
        if (int rc = vertex_masses(e, mass)) return rc;
        double W, G;
        link_rates(t, mass.data(), e->nf, &W, &G);
        max_dt = link_limit(W, G);
    }
    return links_swap(e, t, max_dt, n, links);
}

static int link_forces(mpm_engine* e, float* f_out) { return rows_eval(e, k_link_eval, e->links.args, f_out); }

// One double term and one float length per link from the device, the terms added here in link order: a fixed order,
// no atomics (the sums of mpm_measure.h follow the same rule)
static int link_energy(mpm_engine* e, double* energy_out, float* length_out) {
    const size_t n = e->links.set.size();
    double sum = 0.0;
    if (n) {
        if (int rc = e->stage(n * 12)) return rc;
        double* d_term = (double*)e->d_stage;
        float* d_len = (float*)(d_term + n);
        hipLaunchKernelGGL(k_link_energy, dim3(((unsigned)n + 255u) / 256u), dim3(256), 0, e->stream, e->dp, e->links.d_pair, (int)n,
                           (const uint8_t*)e->links.brk.broken, d_term, d_len);
        std::vector<double> term(n);
        D2H(e, term.data(), d_term, n * 8);
        if (length_out) D2H(e, length_out, d_len, n * 4);
        for (size_t i = 0; i < n; ++i) sum += term[i];
    }
    *energy_out = sum;
    return 0;
}

// ---- breakable links (mpm_set_link_limits, mpm_get_link_limits, mpm_set_broken_links, mpm_link_break_state,
// mpm_link_break_measure, mpm_link_breaks; mpm_links.h) ----
// the breaking tables released (the limits as given stay with the caller)
static void link_break_free(mpm_engine* e) {
    mpm_engine::Links& o = e->links;
    float* o_B2 = const_cast<float*>(o.brk.B2);
    unsigned* o_entry = const_cast<unsigned*>(o.brk.entry);
    int2* o_range = const_cast<int2*>(o.d_range);
    e->dfree(o_B2);
    e->dfree(o_entry);
    e->dfree(o.brk.broken);
    e->dfree(o_range);
    e->dfree(o.d_count);
    o.brk = LinkBreakArgs{};
    o.d_range = nullptr;
    o.d_count = nullptr;
}
// the broken links, counted on the device in link order (k_tear_count on the single range (0, n)); 0 while the tables
// do not exist
static int link_break_count(mpm_engine* e, uint32_t* n_out) {
    *n_out = 0u;
    if (!e->links.breaking()) return 0;
    hipLaunchKernelGGL(k_tear_count, dim3(1), dim3(256), 0, e->stream, (const uint8_t*)e->links.brk.broken, e->links.d_range,
                       e->links.d_count);
    HIP_TRY(hipGetLastError());
    D2H(e, n_out, e->links.d_count, sizeof(uint32_t));
    return 0;
}
// Puts the limits `limits` (checked; one per link, or none: all off) in force, and the flags `broken` if given (one byte
// per link; null: the flags stay as they are).  The tables exist while some limit is > 0 or some flag is set; otherwise
// they are freed and the engine launches what it launched before.  With flags given, LinkArgs::ent of the table in force
// is rebuilt from the caller's links with the flagged links' entries replaced by their rows' padding, and uploaded: that
// is scissors and restore alike.  The caller has settled the owed substeps.  A failure changes nothing.
static int link_break_apply(mpm_engine* e, std::vector<float> limits, const uint8_t* broken) {
    mpm_engine::Links& o = e->links;
    const size_t n = o.set.size();
    const Link* L = reinterpret_cast<const Link*>(o.set.data());
    std::vector<float> B2(std::max<size_t>(n, 1), 0.f);
    if (!limits.empty()) {
        const std::string refusal = link_limits(limits.data(), L, n, B2.data());
        if (!refusal.empty()) return fail(MPM_ERR_INVALID, refusal);
    }
    bool any = false;
    for (size_t i = 0; i < n; ++i) any = any || B2[i] > 0.f;
    std::vector<uint8_t> flags;
    if (broken) {
        flags.resize(n);
        for (size_t i = 0; i < n; ++i) {
            flags[i] = broken[i] != 0 ? 1 : 0;
            any = any || flags[i] != 0;
        }
    } else if (!any) {
        uint32_t k;
        if (int rc = link_break_count(e, &k)) return rc;
        any = k != 0u;
    }
    // the table on the host again, where its entries' places or its records are needed
    LinkTable t;
    const bool create = any && n != 0 && !o.breaking();
    if (n != 0 && (create || (broken && o.breaking()))) {
        std::string why;
        if (!link_table(L, n, e->nf, e->nv, LINK_SLICE, t, why)) return fail(MPM_ERR_INVALID, why);
        for (size_t i = 0; broken && i < n; ++i)
            if (flags[i]) {
                t.ent[t.entry_of_link[2 * i]] = LinkRecord{t.pair[i].a, 0.f, 0.f, 0.f};
                t.ent[t.entry_of_link[2 * i + 1]] = LinkRecord{t.pair[i].b & ~LINK_FLAG_BIT, 0.f, 0.f, 0.f};
            }
    }
    // (a synchronisation point: the kernels enqueued so far have read the old tables)
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (create) {
        FreshArrays fresh(e);
        float* d_B2 = nullptr;
        unsigned* d_entry = nullptr;
        uint8_t* d_broken = nullptr;
        int2* d_range = nullptr;
        uint32_t* d_count = nullptr;
        if (int rc = fresh.alloc(&d_B2, n, false)) return rc;
        if (int rc = fresh.alloc(&d_entry, 2 * n, false)) return rc;
        if (int rc = fresh.alloc(&d_broken, n, true)) return rc;
        if (int rc = fresh.alloc(&d_range, 1, false)) return rc;
        if (int rc = fresh.alloc(&d_count, 1, true)) return rc;
        const int2 range = make_int2(0, (int)n);
        H2D(e, d_entry, t.entry_of_link.data(), 2 * n * sizeof(unsigned));
        H2D(e, d_range, &range, sizeof(range));
        o.brk = LinkBreakArgs{o.d_pair, d_B2, d_entry, d_broken, const_cast<float4*>(o.args.ent), (int)n};
        o.d_range = d_range;
        o.d_count = d_count;
        fresh.commit();
    }
    if (o.breaking()) {
        if (broken) {
            H2D(e, o.brk.ent, t.ent.data(), t.ent.size() * sizeof(LinkRecord));
            H2D(e, o.brk.broken, flags.data(), n);
        }
        if (any) H2D(e, const_cast<float*>(o.brk.B2), B2.data(), n * sizeof(float));
        else link_break_free(e);
    }
    o.limits.swap(limits);
    return 0;
}
// mpm_link_break_state: the flags and their count
static int link_break_state(mpm_engine* e, uint8_t* broken_out, uint32_t* count_out) {
    uint32_t k;
    if (int rc = link_break_count(e, &k)) return rc;
    if (count_out) *count_out = k;
    const size_t n = e->links.set.size();
    if (broken_out && n) {
        if (e->links.breaking()) D2H(e, broken_out, e->links.brk.broken, n);
        else std::memset(broken_out, 0, n);
    }
    return 0;
}
// mpm_link_break_measure: one launch of k_link_break_eval on the current state, in link order
static int link_break_measure(mpm_engine* e, float* l2_out, uint8_t* would_break_out) {
    const size_t n = e->links.set.size();
    if (n == 0) return 0;
    if (int rc = e->stage(5 * n)) return rc;
    float* d_l2 = (float*)e->d_stage;
    uint8_t* d_br = (uint8_t*)e->d_stage + 4 * n;
    hipLaunchKernelGGL(k_link_break_eval, dim3(((unsigned)n + 255u) / 256u), dim3(256), 0, e->stream, e->dp, e->links.d_pair,
                       e->links.brk.B2, (int)n, d_l2, d_br);
    HIP_TRY(hipGetLastError());
    if (l2_out) D2H(e, l2_out, d_l2, 4 * n);
    if (would_break_out) D2H(e, would_break_out, d_br, n);
    return 0;
}
// host code only: the device function of the kernels, compiled for the host
static int link_breaks_host(size_t n, const float* xa3, const float* xb3, const float* B2, float* l2_out, uint8_t* breaks_out) {
    for (size_t i = 0; i < n; ++i) {
        const float *xa = xa3 + 3 * i, *xb = xb3 + 3 * i;
        const float d[3] = {xb[0] - xa[0], xb[1] - xa[1], xb[2] - xa[2]};
        float l2;
        const bool breaks = link_breaks(d, B2[i], &l2);
        if (l2_out) l2_out[i] = l2;
        if (breaks_out) breaks_out[i] = breaks ? 1 : 0;
    }
    return 0;
}

// ---- enclosed-volume pressure per cloth (mpm_set_pressure, mpm_get_pressure, mpm_pressure_forces, mpm_pressure_state,
// mpm_mesh_is_closed, mpm_pressure_vertex_force; mpm_pressure.h) ----
// The table `t` for the caller's per-cloth parameters (checked; none: off) put in force: new device arrays, upload, swap.
// Beside the row table go the rows' cloths, the parameters, the chunk list of k_pressure_volume (the gas cloths' chunks,
// then all cloths'), its partial sums, both range tables and the per-cloth state.  The caller has settled the owed
// substeps.  A failure changes nothing: the new buffers go, the table in force stays.
static int pressure_swap(mpm_engine* e, const PressureTable& t, size_t n_cloths, const mpm_cloth_pressure_t* per_cloth) {
    static_assert(sizeof(ClothPressure) == sizeof(mpm_cloth_pressure_t) && sizeof(ClothPressureState) == sizeof(mpm_cloth_pressure_state_t) &&
                      sizeof(ClothPressureState) == 24,
                  "pressure layouts differ");
    const size_t nc = e->cloths.size();
    std::vector<ClothPressure> par(nc, ClothPressure{PRESSURE_OFF, 0.f, 0.f, 0.f, 0.f});
    if (n_cloths) std::memcpy(par.data(), per_cloth, nc * sizeof(ClothPressure));
    std::vector<int4> chunks, ranges_gas, ranges_all;
    pressure_chunks(e->cloths, [&](size_t c) { return par[c].mode == PRESSURE_GAS; }, chunks, ranges_gas);
    const int n_gas = (int)chunks.size();
    pressure_chunks(e->cloths, [](size_t) { return true; }, chunks, ranges_all);
    mpm_engine::Pressure next;
    FreshArrays fresh(e);
    if (int rc = rows_upload(e, fresh, t, &next.args)) return rc;
    int4 *d_chunks = nullptr, *d_rg = nullptr, *d_ra = nullptr;
    double* d_partial = nullptr;
    uint32_t* d_vent = nullptr;
    ClothPressure* d_par = nullptr;
    ClothPressureState* d_state = nullptr;
    int* d_row_cloth = nullptr;
    if (int rc = fresh.alloc(&d_chunks, std::max<size_t>(chunks.size(), 1), false)) return rc;
    if (int rc = fresh.alloc(&d_partial, std::max<size_t>(chunks.size(), 1), true)) return rc;
    if (int rc = fresh.alloc(&d_vent, std::max<size_t>(chunks.size(), 1), true)) return rc;
    if (int rc = fresh.alloc(&d_rg, std::max<size_t>(nc, 1), false)) return rc;
    if (int rc = fresh.alloc(&d_ra, std::max<size_t>(nc, 1), false)) return rc;
    if (int rc = fresh.alloc(&d_par, std::max<size_t>(nc, 1), true)) return rc;
    if (int rc = fresh.alloc(&d_state, std::max<size_t>(nc, 1), true)) return rc;
    if (!chunks.empty()) H2D(e, d_chunks, chunks.data(), chunks.size() * sizeof(int4));
    if (nc) {
        H2D(e, d_rg, ranges_gas.data(), nc * sizeof(int4));
        H2D(e, d_ra, ranges_all.data(), nc * sizeof(int4));
        H2D(e, d_par, par.data(), nc * sizeof(ClothPressure));
    }
    if (next.args.n_rows) {
        if (int rc = fresh.alloc(&d_row_cloth, t.row_cloth.size(), false)) return rc;
        H2D(e, d_row_cloth, t.row_cloth.data(), t.row_cloth.size() * sizeof(int));
    }
    next.args.row_cloth = d_row_cloth;
    next.args.par = d_par;
    next.args.state = d_state;
    next.vol = PressureVolumeArgs{d_chunks, d_partial, d_ra, d_par, d_state, 0, d_vent, nullptr};
    next.d_ranges_gas = d_rg;
    next.n_gas_chunks = n_gas;
    next.n_all_chunks = (int)chunks.size() - n_gas;
    next.built = true;
    if (n_cloths) next.set.assign(per_cloth, per_cloth + n_cloths);
    {   // the arrays of the table that was in force
        const mpm_engine::Pressure& o = e->pressure;
        rows_free(e, o.args);
        void* old[] = {(void*)o.args.row_cloth, (void*)o.vol.chunks, (void*)o.vol.partial, (void*)o.vol.ranges, (void*)o.vol.par,
                       (void*)o.vol.state, (void*)o.d_ranges_gas, (void*)o.vol.vent};
        for (void* q : old) e->dfree(q);
    }
    e->pressure = next;
    fresh.commit();
    return 0;
}
// mpm_set_pressure: the numbers, the gas cloths' meshes and rest volumes, the table on the host, the swap
static int set_pressure(mpm_engine* e, size_t n_cloths, const mpm_cloth_pressure_t* per_cloth) {
    const ClothPressure* P = reinterpret_cast<const ClothPressure*>(per_cloth);
    const std::string refusal = pressure_refusal(P, n_cloths);
    if (!refusal.empty()) return fail(MPM_ERR_INVALID, refusal);
    REQUIRE(e->np < (size_t)1 << 31, "pressure: too many particles");
    for (size_t c = 0; c < n_cloths; ++c) {
        if (P[c].mode != PRESSURE_GAS) continue;
        const mpm_engine::Cloth& cl = e->cloths[c];
        int32_t edge[2] = {0, 0};
        if (!mesh_is_closed(e->h_idx.data() + 3 * cl.first_face, cl.n_faces, edge))
            return fail(MPM_ERR_INVALID, "pressure: cloth " + std::to_string(c) + " is in gas mode but its mesh is not closed and consistently "
                        "wound: the edge " + std::to_string(edge[0]) + " -> " + std::to_string(edge[1]) +
                        " does not occur exactly once with its reverse exactly once");
        if (!(mesh_volume(e->h_rest.data(), e->h_idx.data(), cl.first_face, cl.n_faces) > 0.0))
            return fail(MPM_ERR_INVALID, "pressure: cloth " + std::to_string(c) + " is in gas mode but its rest volume is not positive: "
                        "reverse the winding of its faces");
    }
    PressureTable t;
    if (n_cloths) {
        std::string why;
        if (!pressure_table(e->cloths, e->h_idx.data(), e->nf, P, PRESSURE_SLICE, t, why)) return fail(MPM_ERR_INVALID, why);
    } else {
        t.slice_off.assign(1, 0u);
    }
    // substeps that mpm_run_substeps deferred are owed with the table they were enqueued with
    if (int rc = settle(e)) return rc;
    return pressure_swap(e, t, n_cloths, per_cloth);
}

// The tear flags as a kernel of the feature behind `bit` (MPM_TEAR_CUTS_HINGES, MPM_TEAR_VENTS_GAS) is to see them in this
// launch: null unless mpm_set_tear_coupling has set the bit and the tear tables exist.  The pointer is not kept in a
// feature's own arguments -- tear_apply allocates and frees the array -- so every launch and every query takes a copy of
// its arguments and sets it there (as anchors_posed builds its own).  Null is the parent arithmetic of every kernel.
static const uint8_t* coupled_tear_flags(const mpm_engine* e, uint32_t bit) {
    return (e->tear_coupling & bit) != 0u && e->tear.on() ? e->tear.args.torn : nullptr;
}
static PressureVolumeArgs pressure_volume_args(const mpm_engine* e) {
    PressureVolumeArgs a = e->pressure.vol;
    a.torn = coupled_tear_flags(e, MPM_TEAR_VENTS_GAS);
    return a;
}
// (the damper's bkc likewise: the array belongs to mpm_set_shell_damping, null while no cloth has beta > 0)
static HingeArgs hinge_args(const mpm_engine* e) {
    HingeArgs a = e->shell.hinge;
    a.torn = coupled_tear_flags(e, MPM_TEAR_CUTS_HINGES);
    a.bkc = e->shell.d_bkc;
    return a;
}
static CreaseArgs crease_args(const mpm_engine* e) {
    CreaseArgs a = e->shell.cr;
    a.torn = coupled_tear_flags(e, MPM_TEAR_CUTS_HINGES);
    return a;
}

// V, E, g and the cap of every cloth from the current positions into Pressure::vol.state (stream-ordered; e->dp: no gate)
static int pressure_measure(mpm_engine* e) {
    mpm_engine::Pressure& ps = e->pressure;
    if (!ps.built) {   // (never set: the chunk list of all cloths and a table without rows)
        PressureTable t;
        t.slice_off.assign(1, 0u);
        if (int rc = pressure_swap(e, t, 0, nullptr)) return rc;
    }
    const PressureVolumeArgs va = pressure_volume_args(e);
    if (ps.n_all_chunks)
        hipLaunchKernelGGL(k_pressure_volume, dim3((unsigned)ps.n_all_chunks), dim3(256), 0, e->stream, e->dp, va, ps.n_gas_chunks);
    if (!e->cloths.empty()) hipLaunchKernelGGL(k_pressure_gauge, dim3((unsigned)e->cloths.size()), dim3(64), 0, e->stream, e->dp, va);
    HIP_TRY(hipGetLastError());
    return 0;
}
static int pressure_forces(mpm_engine* e, float* f_out) {
    if (e->pressure.on())
        if (int rc = pressure_measure(e)) return rc;
    return rows_eval(e, k_pressure_eval, e->pressure.args, f_out);
}
static int pressure_state(mpm_engine* e, mpm_cloth_pressure_state_t* out, size_t capacity, size_t* n_out) {
    const size_t nc = e->cloths.size();
    if (int rc = pressure_measure(e)) return rc;
    std::vector<mpm_cloth_pressure_state_t> rows(nc);
    if (nc) D2H(e, rows.data(), e->pressure.vol.state, nc * sizeof(mpm_cloth_pressure_state_t));
    return copy_out(rows, out, capacity, n_out);
}

// ---- shell bending about a curved rest shape (mpm_set_shell_bending, mpm_get_shell_bending, mpm_shell_hinges,
// mpm_shell_forces, mpm_shell_state, mpm_shell_max_stable_dt; mpm_shell.h) ----
// mpm_set_shell_bending: the numbers, the hinges and cbar on the host, the guard from the vertices' masses, psibar from
// the device (k_hinge_rest on the rest positions), the swap.  A failure changes nothing: the new buffers go, the table in
// force stays.
static int set_shell_bending(mpm_engine* e, size_t n_cloths, const mpm_cloth_shell_t* per_cloth, const float* rest_pos) {
    static_assert(sizeof(ClothShell) == sizeof(mpm_cloth_shell_t) && sizeof(ClothShell) == 8, "shell layouts differ");
    const ClothShell* P = reinterpret_cast<const ClothShell*>(per_cloth);
    const std::string refusal = shell_refusal(P, n_cloths);
    if (!refusal.empty()) return fail(MPM_ERR_INVALID, refusal);
    REQUIRE(e->np < (size_t)1 << 31, "shell bending: too many particles");
    if (rest_pos && n_cloths)
        for (size_t i = 0; i < 3 * e->nv; ++i) REQUIRE(std::isfinite(rest_pos[i]), "shell bending: rest_pos is not finite");
    // the shape that gives cbar, the guard's geometry and psibar: rest_pos where given and asked for, else the rest shape
    // in force (the mesh as added until mpm_set_rest_shape)
    std::vector<float> shape(e->h_rest.begin(), e->h_rest.begin() + (long)(3 * e->nv));
    for (size_t c = 0; c < n_cloths && rest_pos; ++c)
        if (P[c].rest == SHELL_REST_SHAPE) {
            const mpm_engine::Cloth& cl = e->cloths[c];
            std::copy(rest_pos + 3 * cl.first_vertex, rest_pos + 3 * (cl.first_vertex + cl.n_verts), shape.begin() + (long)(3 * cl.first_vertex));
        }
    ShellTable t;
    if (n_cloths) {
        std::string why;
        if (!shell_table(e->cloths, e->h_idx.data(), e->nf, P, shape.data(), SHELL_SLICE, t, why)) return fail(MPM_ERR_INVALID, why);
    } else {
        t.slice_off.assign(1, 0u);
    }
    const size_t n = t.kc.size();
    // substeps that mpm_run_substeps deferred are owed with the table they were enqueued with
    if (int rc = settle(e)) return rc;
    mpm_engine::Shell next;
    FreshArrays fresh(e);
    if (n) {
        std::vector<float> mass;
        if (int rc = vertex_masses(e, mass)) return rc;
        next.max_dt = stable_dt_limit(std::sqrt(max_row_rate(t.rate_sum.data(), t.row_vertex.size(), 1.0,
                                                             [&](size_t r) { return mass[(size_t)t.row_vertex[r]]; })));
        // (what mpm_set_shell_damping's guard needs per row: the row's rate as max_row_rate forms it, and its cloth)
        next.max_dt_elastic = next.max_dt;
        next.row_rate.assign(t.row_vertex.size(), 0.0);
        for (size_t r = 0; r < t.row_vertex.size(); ++r)
            if (t.rate_sum[r] > 0.0) {
                const double m = (double)mass[(size_t)t.row_vertex[r]];
                next.row_rate[r] = m > 0.0 ? 1.0 * t.rate_sum[r] / m : (double)INFINITY;
            }
        next.row_cloth.swap(t.row_cloth);
        next.cbar.swap(t.cbar);
        if (int rc = rows_upload(e, fresh, t, &next.args)) return rc;
        std::vector<int4> ids(n);
        std::vector<float2> par(n);
        const int nf = (int)e->nf;
        for (size_t h = 0; h < n; ++h) {
            ids[h] = make_int4(nf + t.ids4[4 * h], nf + t.ids4[4 * h + 1], nf + t.ids4[4 * h + 2], nf + t.ids4[4 * h + 3]);
            par[h] = make_float2(t.kc[h], 0.f);
        }
        int4* d_ids = nullptr;
        int2* d_faces = nullptr;
        float2* d_par = nullptr;
        float4* d_rec = nullptr;
        if (int rc = fresh.alloc(&d_ids, n, false)) return rc;
        if (int rc = fresh.alloc(&d_faces, n, false)) return rc;
        if (int rc = fresh.alloc(&d_par, n, false)) return rc;
        if (int rc = fresh.alloc(&d_rec, 4 * n, true)) return rc;
        H2D(e, d_ids, ids.data(), n * sizeof(int4));
        H2D(e, d_par, par.data(), n * sizeof(float2));
        // (faces A and B per hinge as global face ids, for the cut rule of mpm_set_tear_coupling; t.faces2 is [2 hinge])
        static_assert(sizeof(int2) == 2 * sizeof(int32_t), "int2 layout");
        H2D(e, d_faces, t.faces2.data(), n * sizeof(int2));
        next.hinge = HingeArgs{d_ids, d_par, d_rec, (int)n, d_faces, nullptr, (int)e->nf, nullptr};
        next.args.rec = d_rec;
        next.args.n_hinges = (int)n;
        // psibar: the hinge function on the device, once, on the rest positions -- the psi it writes (plane 0's .w)
        if (int rc = e->stage(shape.size() * 4)) return rc;
        H2D(e, e->d_stage, shape.data(), shape.size() * 4);
        hipLaunchKernelGGL(k_hinge_rest, rows_grid((int)n), dim3(256), 0, e->stream, next.hinge, (const float*)e->d_stage, nf, (int)e->nv);
        HIP_TRY(hipGetLastError());
        std::vector<float4> plane0(n);
        D2H(e, plane0.data(), d_rec, n * sizeof(float4));
        next.psibar.resize(n);
        for (size_t h = 0; h < n; ++h) {
            next.psibar[h] = P[t.hinge_cloth[h]].rest == SHELL_REST_FLAT ? 0.f : plane0[h].w;
            par[h].y = next.psibar[h];
        }
        H2D(e, d_par, par.data(), n * sizeof(float2));
        next.ids4.swap(t.ids4);
        next.kc.swap(t.kc);
        next.hinge_cloth.swap(t.hinge_cloth);
    } else {
        // (a synchronisation point either way: the kernels enqueued so far have read the old table)
        HIP_TRY(hipStreamSynchronize(e->stream));
    }
    if (n_cloths) next.set.assign(per_cloth, per_cloth + n_cloths);
    {   // the arrays of the table that was in force
        const mpm_engine::Shell& o = e->shell;
        rows_free(e, o.args);
        // (the crease parameters and state, and the damper's table and bkc (mpm_set_shell_damping), go with the hinge
        // table they belonged to: `next` has none)
        void* old[] = {(void*)o.hinge.ids, (void*)o.hinge.par, (void*)o.hinge.rec, (void*)o.cr.cr, (void*)o.hinge.faces, (void*)o.d_bkc};
        for (void* q : old) e->dfree(q);
    }
    e->shell = next;
    fresh.commit();
    return 0;
}

// the hinge records of the current positions into Shell::hinge.rec (stream-ordered; e->dp: no gate)
static int shell_measure(mpm_engine* e) {
    hipLaunchKernelGGL(k_hinge_eval<0>, rows_grid(e->shell.hinge.n), dim3(256), 0, e->stream, e->dp, hinge_args(e));
    HIP_TRY(hipGetLastError());
    return 0;
}
static int shell_forces(mpm_engine* e, float* f_out) {
    if (e->shell.on())
        if (int rc = shell_measure(e)) return rc;
    return rows_eval(e, k_hinge_gather_eval, e->shell.on() ? e->shell.args : ShellArgs{}, f_out);
}
// One float term per hinge from the device, added here per cloth in double in hinge order: a fixed order, no atomics
static int shell_state(mpm_engine* e, double* energy_per_cloth, float* psi_out, uint32_t* inactive_out) {
    const mpm_engine::Shell& sh = e->shell;
    const size_t n = sh.on() ? (size_t)sh.hinge.n : 0;
    std::fill(energy_per_cloth, energy_per_cloth + e->cloths.size(), 0.0);
    uint32_t inactive = 0;
    if (n) {
        if (int rc = shell_measure(e)) return rc;
        std::vector<float4> planes(3 * n);
        D2H(e, planes.data(), sh.hinge.rec, 3 * n * sizeof(float4));
        for (size_t h = 0; h < n; ++h) {
            energy_per_cloth[(size_t)sh.hinge_cloth[h]] += (double)planes[n + h].w;
            if (psi_out) psi_out[h] = planes[h].w;
            if (!(planes[2 * n + h].w > 0.f)) inactive += 1;
        }
    }
    if (inactive_out) *inactive_out = inactive;
    return 0;
}

// ---- hinge damping (mpm_set_shell_damping, mpm_get_shell_damping, mpm_shell_damping_forces, mpm_shell_damping_state;
// mpm_shell.h HINGE DAMPING) ----
// Puts the table (one per cloth, or none) in force: bkc = float(beta k cbar) per hinge, formed in double and rounded once,
// and the damped guard.  The arrays exist while some cloth has beta > 0; otherwise they are freed and the engine launches
// what it launched before, with the elastic guard to the bit.  The caller has checked the numbers and settled the owed
// substeps.  A failure changes nothing.
static int set_shell_damping(mpm_engine* e, size_t n_cloths, const mpm_cloth_shell_damping_t* per_cloth) {
    static_assert(sizeof(ClothShellDamping) == sizeof(mpm_cloth_shell_damping_t) && sizeof(ClothShellDamping) == 8, "shell damping layouts differ");
    mpm_engine::Shell& sh = e->shell;
    const size_t n = sh.kc.size();
    // (`given`: some cloth has beta > 0, the table is kept; `any`: such a cloth has a hinge, the arrays exist)
    bool given = false, any = false;
    for (size_t c = 0; c < n_cloths; ++c) given = given || per_cloth[c].beta > 0.f;
    std::vector<float> bkc(n, 0.f);
    for (size_t h = 0; given && h < n; ++h) {
        const size_t c = (size_t)sh.hinge_cloth[h];
        any = any || per_cloth[c].beta > 0.f;
        bkc[h] = (float)((double)per_cloth[c].beta * (double)sh.set[c].stiffness * sh.cbar[h]);
        if (!std::isfinite(bkc[h]))
            return fail(MPM_ERR_INVALID, "shell damping: hinge " + std::to_string(h) + " of cloth " + std::to_string(c) + ": beta k cbar is not a finite float");
    }
    float max_dt = sh.max_dt_elastic;
    if (any) {
        double W, G;
        shell_damped_rates(sh.row_rate, sh.row_cloth, reinterpret_cast<const ClothShellDamping*>(per_cloth), &W, &G);
        if (G > 0.0) max_dt = link_limit(W, G);
    }
    // (a synchronisation point: the kernels enqueued so far have read the old table)
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (any) {
        float* d_bkc = const_cast<float*>(sh.d_bkc);
        if (!d_bkc) {
            FreshArrays fresh(e);
            if (int rc = fresh.alloc(&d_bkc, n, false)) return rc;
            fresh.commit();
        }
        H2D(e, d_bkc, bkc.data(), n * sizeof(float));
        sh.d_bkc = d_bkc;
    } else {
        float* d_bkc = const_cast<float*>(sh.d_bkc);
        e->dfree(d_bkc);
        sh.d_bkc = nullptr;
    }
    if (given) sh.damping.assign(per_cloth, per_cloth + n_cloths);
    else sh.damping.clear();
    sh.max_dt = max_dt;
    return 0;
}
// the damping part's records of the current positions and velocities into Shell::hinge.rec (stream-ordered; no gate): the
// planes are free between substeps, which rewrite them before they read them
static int shell_damping_measure(mpm_engine* e) {
    hipLaunchKernelGGL(k_hinge_eval<2>, rows_grid(e->shell.hinge.n), dim3(256), 0, e->stream, e->dp, hinge_args(e));
    HIP_TRY(hipGetLastError());
    return 0;
}
static int shell_damping_forces(mpm_engine* e, float* f_out) {
    if (e->shell.on())
        if (int rc = shell_damping_measure(e)) return rc;
    return rows_eval(e, k_hinge_gather_eval, e->shell.on() ? e->shell.args : ShellArgs{}, f_out);
}
// One float term per hinge from the device, added here per cloth in double in hinge order: a fixed order, no atomics
static int shell_damping_state(mpm_engine* e, double* power_per_cloth, float* psidot_out) {
    const mpm_engine::Shell& sh = e->shell;
    const size_t n = sh.on() ? (size_t)sh.hinge.n : 0;
    std::fill(power_per_cloth, power_per_cloth + e->cloths.size(), 0.0);
    if (n) {
        if (int rc = shell_damping_measure(e)) return rc;
        std::vector<float4> planes(2 * n);
        D2H(e, planes.data(), sh.hinge.rec, 2 * n * sizeof(float4));
        for (size_t h = 0; h < n; ++h) {
            power_per_cloth[(size_t)sh.hinge_cloth[h]] += (double)planes[n + h].w;
            if (psidot_out) psidot_out[h] = planes[h].w;
        }
    }
    return 0;
}

// ---- creases: plastic shell hinges (mpm_set_creases, mpm_get_creases, mpm_set_crease_state, mpm_crease_state,
// mpm_crease_measure, mpm_crease_hinge; mpm_shell.h) ----
// the psibar in force per hinge: hinge.par[h].y while the crease tables exist, else the rest value
static int crease_current(mpm_engine* e, std::vector<float>& out) {
    const mpm_engine::Shell& sh = e->shell;
    out = sh.psibar;
    if (!sh.creasing()) return 0;
    std::vector<float2> par(out.size());
    D2H(e, par.data(), sh.hinge.par, par.size() * sizeof(float2));
    for (size_t h = 0; h < par.size(); ++h) out[h] = par[h].y;
    return 0;
}
static bool same_bits(float a, float b) { return std::memcmp(&a, &b, 4) == 0; }
// Puts the crease table `table` (one per cloth, or none: all elastic) in force and, with `replace`, the state: psibar[h]
// per hinge, or the rest values where psibar is null (ironing).  The tables exist while some cloth yields or some hinge's
// psibar differs from its rest value in bits; otherwise they are freed and the engine launches what it launched before.
// The caller has settled the owed substeps.  A failure changes nothing.
static int crease_apply(mpm_engine* e, std::vector<mpm_cloth_crease_t> table, bool replace, const float* psibar) {
    static_assert(sizeof(ClothCrease) == sizeof(mpm_cloth_crease_t) && sizeof(ClothCrease) == 16, "crease layouts differ");
    mpm_engine::Shell& sh = e->shell;
    const size_t n = sh.kc.size(), nc = e->cloths.size();
    std::vector<float> yep(3 * std::max<size_t>(nc, 1));
    for (size_t c = 0; c < nc; ++c) yep[3 * c] = 0.f, yep[3 * c + 1] = 0.f, yep[3 * c + 2] = 2.f;
    if (!table.empty()) {
        const std::string refusal = crease_params(reinterpret_cast<const ClothCrease*>(table.data()), table.size(), yep.data());
        if (!refusal.empty()) return fail(MPM_ERR_INVALID, refusal);
    }
    bool any = false;
    std::vector<float4> rec(n);
    for (size_t h = 0; h < n; ++h) {
        const float* q = &yep[3 * (size_t)sh.hinge_cloth[h]];
        rec[h] = make_float4(q[0], q[1], q[2], sh.psibar[h]);
        if (!(std::fabs(sh.psibar[h]) <= q[2]))
            return fail(MPM_ERR_INVALID, "creases: hinge " + std::to_string(h) + " of cloth " + std::to_string(sh.hinge_cloth[h]) +
                                             ": its rest |psibar| is above 2 sin(max_angle / 2)");
        any = any || q[0] > 0.f;
    }
    std::vector<float> state;
    if (replace) {
        state = sh.psibar;
        for (size_t h = 0; psibar && h < n; ++h) {
            const std::string at = "crease state: hinge " + std::to_string(h);
            if (!std::isfinite(psibar[h])) return fail(MPM_ERR_INVALID, at + ": psibar is not finite");
            if (!(std::fabs(psibar[h]) <= rec[h].z)) return fail(MPM_ERR_INVALID, at + ": |psibar| is above its cloth's 2 sin(max_angle / 2)");
            state[h] = psibar[h];
        }
    } else if (int rc = crease_current(e, state)) return rc;
    for (size_t h = 0; h < n; ++h) any = any || !same_bits(state[h], sh.psibar[h]);
    // (a synchronisation point: the kernels enqueued so far have read the old tables)
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (any && !sh.creasing()) {
        FreshArrays fresh(e);
        float4* d_cr = nullptr;
        if (int rc = fresh.alloc(&d_cr, n, false)) return rc;
        sh.cr = CreaseArgs{sh.hinge.ids, const_cast<float2*>(sh.hinge.par), d_cr, (int)n, sh.hinge.faces, nullptr, sh.hinge.n_faces};
        fresh.commit();
    }
    if (sh.creasing()) {
        if (replace) {
            std::vector<float2> par(n);
            for (size_t h = 0; h < n; ++h) par[h] = make_float2(sh.kc[h], state[h]);
            H2D(e, sh.cr.par, par.data(), n * sizeof(float2));
        }
        if (any) {
            H2D(e, const_cast<float4*>(sh.cr.cr), rec.data(), n * sizeof(float4));
        } else {   // (every psibar is its rest value again, to the bit: what k_hinge read before there were creases)
            float4* d_cr = const_cast<float4*>(sh.cr.cr);
            e->dfree(d_cr);
            sh.cr = CreaseArgs{};
        }
    }
    sh.crease.swap(table);
    return 0;
}
// mpm_crease_state: the psibar in force, and per cloth the hinges whose psibar is not the rest value's bits
static int crease_state(mpm_engine* e, float* psibar_out, uint32_t* creased_per_cloth, size_t capacity, size_t* n_out) {
    std::vector<float> cur;
    if (int rc = crease_current(e, cur)) return rc;
    std::vector<uint32_t> count(e->cloths.size(), 0u);
    for (size_t h = 0; h < cur.size(); ++h) {
        if (psibar_out) psibar_out[h] = cur[h];
        if (!same_bits(cur[h], e->shell.psibar[h])) count[(size_t)e->shell.hinge_cloth[h]] += 1u;
    }
    return copy_out(count, creased_per_cloth, capacity, n_out);
}
// mpm_crease_measure: one launch of k_crease_eval on the current state, in hinge order; while the tables do not exist,
// with a record array of its own in which no hinge yields
static int crease_measure(mpm_engine* e, float* psi_out, float* dpsi_out, float* next_out) {
    const mpm_engine::Shell& sh = e->shell;
    const size_t n = sh.kc.size();
    if (n == 0) return 0;
    CreaseArgs a = crease_args(e);
    // (the staging buffer: the records where they are made here, 16 bytes per hinge, then three float outputs)
    if (int rc = e->stage(28 * n)) return rc;
    if (!sh.creasing()) {
        std::vector<float4> rec(n);
        for (size_t h = 0; h < n; ++h) rec[h] = make_float4(0.f, 0.f, 2.f, sh.psibar[h]);
        float4* d_cr = (float4*)e->d_stage;
        H2D(e, d_cr, rec.data(), n * sizeof(float4));
        a = CreaseArgs{sh.hinge.ids, const_cast<float2*>(sh.hinge.par), d_cr, (int)n, sh.hinge.faces, a.torn, sh.hinge.n_faces};
    }
    float* d_out = (float*)e->d_stage + 4 * n;
    hipLaunchKernelGGL(k_crease_eval, rows_grid((int)n), dim3(256), 0, e->stream, e->dp, a, d_out, d_out + n, d_out + 2 * n);
    HIP_TRY(hipGetLastError());
    if (psi_out) D2H(e, psi_out, d_out, 4 * n);
    if (dpsi_out) D2H(e, dpsi_out, d_out + n, 4 * n);
    if (next_out) D2H(e, next_out, d_out + 2 * n, 4 * n);
    return 0;
}
// host code only: the device functions of the kernels, compiled for the host
static int crease_hinge_host(size_t n, const float* x12, const float* psibar, const float* y, const float* eta, const float* P,
                             float* psi_out, float* dpsi_out, float* psibar_out, uint8_t* yields_out) {
    for (size_t i = 0; i < n; ++i) {
        const float* x = x12 + 12 * i;
        float psi, dpsi;
        bool yields;
        const bool on = shell_angle(x, x + 3, x + 6, x + 9, &psi, &dpsi);
        const float next = crease_return(psi, dpsi, on, psibar[i], y[i], eta[i], P[i], &yields);
        if (psi_out) psi_out[i] = psi;
        if (dpsi_out) dpsi_out[i] = dpsi;
        if (psibar_out) psibar_out[i] = next;
        if (yields_out) yields_out[i] = yields ? 1 : 0;
    }
    return 0;
}

// ---- stiffness-proportional damping (mpm_set_damping, mpm_get_damping, mpm_damping_forces, mpm_damping_max_stable_dt,
// mpm_damping_face_records; mpm_damping.h) ----
// mpm_damping_max_stable_dt from what the engine holds: the membrane row sums and vertex masses of the last
// mpm_set_damping, the rows of the bending table in force.  Host only; cannot fail.  Also says whether k_bend_damp has a
// row to work on (a cloth with beta_bending > 0 and bending stiffness > 0).
static void damping_limit(mpm_engine* e) {
    mpm_engine::Damping& dm = e->damp;
    dm.max_dt = INFINITY;
    dm.bend_rows = false;
    if (!dm.any()) return;
    std::vector<double> D(e->nv, 0.0);
    if (dm.membrane()) D = dm.D_membrane;
    if (e->bend.on())
        for (size_t r = 0; r < e->bend.row_vertex.size(); ++r) {
            const size_t v = (size_t)e->bend.row_vertex[r];
            const float beta = dm.beta_vertex[v];
            if (!(beta > 0.f)) continue;
            dm.bend_rows = true;
            D[v] += (double)beta * e->bend.abs_sum[r];
        }
    dm.max_dt = stable_dt_limit(max_row_rate(D.data(), e->nv, 1.0, [&](size_t i) { return dm.mass[i]; }));
}
// Puts the coefficients `d` (checked; one per cloth, or none) in force: k_damp's tables, k_bend_damp's coefficient per
// vertex (it reads the bending table in force) and the stability limit.  The caller has settled the owed substeps.  A
// failure changes nothing.
static int damping_apply(mpm_engine* e, std::vector<mpm_cloth_damping_t> d) {
    const size_t nc = d.size();
    bool membrane = false, bending = false;
    for (size_t c = 0; c < nc; ++c) {
        membrane = membrane || d[c].membrane > 0.f;
        bending = bending || d[c].bending > 0.f;
    }
    mpm_engine::Damping next;
    FreshArrays fresh(e);
    if (membrane || bending) {
        std::vector<float4> coef(std::max<size_t>(nc, 1), make_float4(0.f, 0.f, 0.f, 0.f));
        std::vector<int> cloth_of_face(e->nf, 0);
        next.beta_vertex.assign(e->nv, 0.f);
        for (size_t c = 0; c < nc; ++c) {
            const mpm_engine::Cloth& cl = e->cloths[c];
            float mu, lambda;
            cloth_lame(e, c, &mu, &lambda);
            coef[c] = make_float4(mu, lambda, d[c].membrane, 0.f);
            std::fill(cloth_of_face.begin() + (long)cl.first_face, cloth_of_face.begin() + (long)(cl.first_face + cl.n_faces), (int)c);
            std::fill(next.beta_vertex.begin() + (long)cl.first_vertex, next.beta_vertex.begin() + (long)(cl.first_vertex + cl.n_verts),
                      d[c].bending);
        }
        // every particle's q[0].w in original order: a vertex's mass as ParticleToGrid forms it (x DP::M.density, both floats),
        // a face's rest volume (a multi-material engine holds the mass there: / the cloth's density)
        std::vector<float> w, mass;
        if (int rc = vertex_masses(e, mass, &w)) return rc;
        next.mass.assign(mass.begin(), mass.end());
        if (membrane) {
            // sum_j |D_ij| of the membrane's damping matrix at the rest shape, per vertex (Gershgorin)
            std::vector<float> dminv(e->nf * 4);
            int* iota = nullptr;
            if (int rc = device_iota(e, &iota)) return rc;
            if (int rc = gather_to_host<F_DMINV>(e, dminv.data(), e->nf, iota)) return rc;
            next.D_membrane.assign(e->nv, 0.0);
            for (size_t f = 0; f < e->nf; ++f) {
                const float4 c = coef[(size_t)cloth_of_face[f]];
                if (!(c.z > 0.f)) continue;
                const double Dm0 = dminv[4 * f], Dm1 = dminv[4 * f + 1], Dm3 = dminv[4 * f + 3];
                const double vol = std::fabs((double)w[f]) / (e->multi_mat ? (double)e->h_rho_of_pid[f] : 1.0);
                const double g[3] = {std::hypot(Dm0, Dm1 + Dm3), std::hypot(Dm0, Dm1), std::fabs(Dm3)};   // |columns of grad_N|
                const double s = (double)c.z * vol * (2.0 * (double)c.x + 2.0 * (double)c.y) * (g[0] + g[1] + g[2]);
                for (int k = 0; k < 3; ++k) next.D_membrane[(size_t)e->h_idx[3 * f + k]] += s * g[k];
            }
            float4* d_coef = nullptr;
            int* d_cloth = nullptr;
            if (int rc = fresh.alloc(&d_coef, coef.size(), false)) return rc;
            if (int rc = fresh.alloc(&d_cloth, cloth_of_face.size(), false)) return rc;
            H2D(e, d_coef, coef.data(), coef.size() * sizeof(float4));
            if (!cloth_of_face.empty()) H2D(e, d_cloth, cloth_of_face.data(), cloth_of_face.size() * sizeof(int));
            next.args = DampArgs{d_coef, d_cloth};
        }
        if (bending) {
            if (int rc = fresh.alloc(&next.d_beta_vertex, e->nv, false)) return rc;
            H2D(e, next.d_beta_vertex, next.beta_vertex.data(), e->nv * sizeof(float));
        }
    }
    // (a synchronisation point: the kernels enqueued so far have read the old tables)
    HIP_TRY(hipStreamSynchronize(e->stream));
    {
        float4* o_coef = const_cast<float4*>(e->damp.args.coef);
        int* o_cloth = const_cast<int*>(e->damp.args.cloth_of_face);
        e->dfree(o_coef);
        e->dfree(o_cloth);
        e->dfree(e->damp.d_beta_vertex);
    }
    next.d.swap(d);
    e->damp = next;
    fresh.commit();
    damping_limit(e);
    return 0;
}

static int damping_forces(mpm_engine* e, float* f_out) {
    std::memset(f_out, 0, e->nv * 12);
    const bool hinges = e->bend.on() && e->damp.bending();
    if (!e->damp.membrane() && !hinges) return 0;
    // the face records in original face order, behind them the bending rows in original vertex order
    const size_t n_rec = e->nf * 9, n_all = n_rec + e->nv * 3;
    if (int rc = e->stage(n_all * 4)) return rc;
    HIP_TRY(hipMemsetAsync(e->d_stage, 0, n_all * 4, e->stream));
    if (e->damp.membrane() && e->nf)
        hipLaunchKernelGGL(k_damp_eval, dim3((unsigned)((e->nf + 255) / 256)), dim3(256), 0, e->stream, e->dp, e->damp.args,
                           (float*)e->d_stage);
    if (hinges)
        hipLaunchKernelGGL(k_bend_damp_eval, rows_grid(e->bend.args.n_rows), dim3(256), 0, e->stream, e->dp, e->bend.args,
                           (const float*)e->damp.d_beta_vertex, (float*)e->d_stage + n_rec);
    HIP_TRY(hipGetLastError());
    std::vector<float> h(n_all);
    D2H(e, h.data(), e->d_stage, n_all * 4);
    // a vertex's records in ascending original face id, as k_vforce sums them; then the bending row, as k_bend_damp adds it
    for (size_t f = 0; f < e->nf; ++f)
        for (int c = 0; c < 3; ++c) {
            float* o = f_out + 3 * (size_t)e->h_idx[3 * f + c];
            for (int k = 0; k < 3; ++k) o[k] += -h[9 * f + 3 * c + k];
        }
    for (size_t i = 0; i < e->nv * 3; ++i) f_out[i] += h[n_rec + i];
    return 0;
}

// host code only: the device function of the kernels, compiled for the host
static int damping_face_records(size_t n_faces, const float* dminv3, const float* vol, const float* mu, const float* lambda,
                                const float* beta, const float* x9, const float* v9, float* rec9_out) {
    for (size_t f = 0; f < n_faces; ++f) {
        float x[3][3], v[3][3], rec[3][3];
        std::memcpy(x, x9 + 9 * f, sizeof x);
        std::memcpy(v, v9 + 9 * f, sizeof v);
        damp_face(dminv3[3 * f], dminv3[3 * f + 1], dminv3[3 * f + 2], vol[f], mu[f], lambda[f], beta[f], x, v, rec);
        std::memcpy(rec9_out + 9 * f, rec, sizeof rec);
    }
    return 0;
}

// ---- woven cloth (mpm_set_weave, mpm_get_weave, mpm_weave_axes, mpm_weave_forces, mpm_weave_strain, mpm_weave_energy,
// mpm_weave_max_stable_dt, mpm_weave_face_records, mpm_weave_face_axes; mpm_weave.h) ----
// Puts the constants `w` (checked; one per cloth, or none) and the directions in force: k_weave's three tables, the
// ranges of k_weave_energy and the stability limit.  The caller has settled the owed substeps.  A failure changes nothing.
static int weave_apply(mpm_engine* e, std::vector<mpm_cloth_weave_t> w, const float* face_dirs) {
    const size_t nc = w.size();
    std::vector<float4> coef(std::max<size_t>(nc, 1), make_float4(0.f, 0.f, 0.f, 0.f));
    bool any = false;
    for (size_t c = 0; c < nc; ++c) {
        float k[4];
        weave_coefficients(w[c].E_warp, w[c].E_weft, w[c].nu, w[c].G, k);
        coef[c] = make_float4(k[0], k[1], k[2], k[3]);
        any = any || k[0] != 0.f || k[1] != 0.f || k[2] != 0.f || k[3] != 0.f;
    }
    mpm_engine::Weave next;
    FreshArrays fresh(e);
    if (any) {
        std::vector<int> cloth_of_face(e->nf, 0);
        std::vector<int2> ranges(nc);
        next.axis.assign(2 * e->nf, 0.f);
        for (size_t c = 0; c < nc; ++c) {
            const mpm_engine::Cloth& cl = e->cloths[c];
            ranges[c] = make_int2((int)cl.first_face, (int)(cl.first_face + cl.n_faces));
            std::fill(cloth_of_face.begin() + (long)cl.first_face, cloth_of_face.begin() + (long)(cl.first_face + cl.n_faces), (int)c);
            const float4 k = coef[c];
            if (k.x == 0.f && k.y == 0.f && k.z == 0.f && k.w == 0.f) continue;
            for (size_t f = cl.first_face; f < cl.first_face + cl.n_faces; ++f) {
                float X[3][3];
                for (int j = 0; j < 3; ++j) std::memcpy(X[j], &e->h_rest[(size_t)e->h_idx[3 * f + j] * 3], 12);
                const float* d = w[c].warp_dir;
                if (face_dirs && (face_dirs[3 * f] != 0.f || face_dirs[3 * f + 1] != 0.f || face_dirs[3 * f + 2] != 0.f))
                    d = face_dirs + 3 * f;
                if (!weave_face_axis(X, d, &next.axis[2 * f]))
                    return fail(MPM_ERR_INVALID, "weave: face " + std::to_string(f) + " (cloth " + std::to_string(c) +
                                                     "): the warp direction is zero or within 1e-3 of the face's rest normal");
            }
        }
        // Gershgorin's row sums of the weave's stiffness at the rest shape, per vertex, over the vertices' masses
        std::vector<float> wq, mass;
        if (int rc = vertex_masses(e, mass, &wq)) return rc;
        std::vector<float> dminv(e->nf * 4);
        int* iota = nullptr;
        if (int rc = device_iota(e, &iota)) return rc;
        if (int rc = gather_to_host<F_DMINV>(e, dminv.data(), e->nf, iota)) return rc;
        std::vector<double> K(e->nv, 0.0);
        for (size_t f = 0; f < e->nf; ++f) {
            const float4 c = coef[(size_t)cloth_of_face[f]];
            const float k4[4] = {c.x, c.y, c.z, c.w};
            const double kmax = weave_kmax(k4);
            if (!(kmax > 0.0)) continue;
            const double Dm0 = dminv[4 * f], Dm1 = dminv[4 * f + 1], Dm3 = dminv[4 * f + 3];
            const double vol = std::fabs((double)wq[f]) / (e->multi_mat ? (double)e->h_rho_of_pid[f] : 1.0);
            const double g[3] = {std::hypot(Dm0, Dm1 + Dm3), std::hypot(Dm0, Dm1), std::fabs(Dm3)};   // |columns of grad_N|
            const double s = vol * kmax * (g[0] + g[1] + g[2]);
            for (int k = 0; k < 3; ++k) K[(size_t)e->h_idx[3 * f + k]] += s * g[k];
        }
        next.max_dt = stable_dt_limit(std::sqrt(max_row_rate(K.data(), e->nv, 1.0, [&](size_t i) { return mass[i]; })));
        float4* d_coef = nullptr;
        int* d_cloth = nullptr;
        float2* d_axis = nullptr;
        int2* d_ranges = nullptr;
        if (int rc = fresh.alloc(&d_coef, coef.size(), false)) return rc;
        if (int rc = fresh.alloc(&d_cloth, std::max<size_t>(cloth_of_face.size(), 1), false)) return rc;
        if (int rc = fresh.alloc(&d_axis, std::max<size_t>(e->nf, 1), false)) return rc;
        if (int rc = fresh.alloc(&d_ranges, ranges.size(), false)) return rc;
        H2D(e, d_coef, coef.data(), coef.size() * sizeof(float4));
        if (e->nf) {
            H2D(e, d_cloth, cloth_of_face.data(), cloth_of_face.size() * sizeof(int));
            H2D(e, d_axis, next.axis.data(), next.axis.size() * sizeof(float));
        }
        H2D(e, d_ranges, ranges.data(), ranges.size() * sizeof(int2));
        next.args = WeaveArgs{d_coef, d_cloth, d_axis};
        next.d_ranges = d_ranges;
    }
    // (a synchronisation point: the kernels enqueued so far have read the old tables)
    HIP_TRY(hipStreamSynchronize(e->stream));
    {
        float4* o_coef = const_cast<float4*>(e->weave.args.coef);
        int* o_cloth = const_cast<int*>(e->weave.args.cloth_of_face);
        float2* o_axis = const_cast<float2*>(e->weave.args.axis);
        int2* o_ranges = const_cast<int2*>(e->weave.d_ranges);
        e->dfree(o_coef);
        e->dfree(o_cloth);
        e->dfree(o_axis);
        e->dfree(o_ranges);
    }
    next.w.swap(w);
    e->weave = next;
    fresh.commit();
    return 0;
}

// mpm_weave_forces (f_out, rec_out), mpm_weave_strain (strain_out), mpm_weave_energy (per_cloth, capacity, n_out, total;
// `total` non-null selects it): one launch of k_weave_eval on the current state, by original face id; zeros while off.
static int weave_eval(mpm_engine* e, float* f_out, float* rec_out, float* strain_out, double* per_cloth, size_t capacity,
                      size_t* n_out, double* total) {
    const size_t nf = e->nf, nc = e->cloths.size();
    if (f_out) std::memset(f_out, 0, e->nv * 12);
    if (rec_out) std::memset(rec_out, 0, nf * 36);
    if (strain_out) std::memset(strain_out, 0, nf * 12);
    if (total) {
        std::fill(per_cloth, per_cloth + std::min(capacity, nc), 0.0);
        if (n_out) *n_out = nc;
        *total = 0.0;
    }
    if (!e->weave.on() || nf == 0) return 0;
    // records [9 nf], strains [3 nf], energies [nf] as floats, then (8-byte aligned) one double per cloth
    const size_t n_float = 13 * nf, off_sums = (n_float * 4 + 7) / 8 * 8;
    if (int rc = e->stage(off_sums + nc * 8)) return rc;
    HIP_TRY(hipMemsetAsync(e->d_stage, 0, off_sums + nc * 8, e->stream));
    float* d = (float*)e->d_stage;
    hipLaunchKernelGGL(k_weave_eval, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, e->stream, e->dp, e->weave.args, d, d + 9 * nf,
                       d + 12 * nf);
    if (total)
        hipLaunchKernelGGL(k_weave_energy, dim3((unsigned)nc), dim3(256), 0, e->stream, (const float*)(d + 12 * nf), e->weave.d_ranges,
                           (double*)((char*)e->d_stage + off_sums));
    HIP_TRY(hipGetLastError());
    if (total) {
        std::vector<double> rows(nc);
        D2H(e, rows.data(), (char*)e->d_stage + off_sums, nc * 8);
        std::copy(rows.begin(), rows.begin() + (long)std::min(capacity, nc), per_cloth);
        for (double r : rows) *total += r;
        return 0;
    }
    if (strain_out) {
        D2H(e, strain_out, d + 9 * nf, nf * 12);
        return 0;
    }
    std::vector<float> own;
    float* h = rec_out;
    if (!h) {
        own.resize(9 * nf);
        h = own.data();
    }
    D2H(e, h, d, nf * 36);
    // a vertex's records in ascending original face id, as k_vforce sums them
    for (size_t f = 0; f < nf; ++f)
        for (int c = 0; c < 3; ++c) {
            float* o = f_out + 3 * (size_t)e->h_idx[3 * f + c];
            for (int k = 0; k < 3; ++k) o[k] += -h[9 * f + 3 * c + k];
        }
    return 0;
}

// host code only: the device function of the kernels, compiled for the host
static int weave_face_records(size_t n, const float* dminv3, const float* vol, const float* coef4, const float* cs2, const float* x9,
                              float* rec9_out, float* strain3_out, float* energy_out) {
    for (size_t f = 0; f < n; ++f) {
        float x[3][3], rec[3][3], strain[3], energy;
        std::memcpy(x, x9 + 9 * f, sizeof x);
        weave_face(dminv3[3 * f], dminv3[3 * f + 1], dminv3[3 * f + 2], vol[f], coef4 + 4 * f, cs2[2 * f], cs2[2 * f + 1], x, rec,
                   strain, &energy);
        if (rec9_out) std::memcpy(rec9_out + 9 * f, rec, sizeof rec);
        if (strain3_out) std::memcpy(strain3_out + 3 * f, strain, sizeof strain);
        if (energy_out) energy_out[f] = energy;
    }
    return 0;
}
// host code only: the axis function of weave_apply
static int weave_face_axes(size_t n, const float* rest_x9, const float* dir3, float* cs2_out, int32_t* first_bad_out) {
    int32_t bad = -1;
    for (size_t f = 0; f < n; ++f) {
        float X[3][3];
        std::memcpy(X, rest_x9 + 9 * f, sizeof X);
        if (!weave_face_axis(X, dir3 + 3 * f, cs2_out + 2 * f)) {
            cs2_out[2 * f] = cs2_out[2 * f + 1] = 0.f;
            if (bad < 0) bad = (int32_t)f;
        }
    }
    if (first_bad_out) *first_bad_out = bad;
    if (bad >= 0)
        return fail(MPM_ERR_INVALID, "weave: face " + std::to_string(bad) + ": the direction is zero or within 1e-3 of the face's rest normal");
    return 0;
}

// ---- tearing cloth (mpm_set_tearing, mpm_get_tearing, mpm_set_torn_faces, mpm_tear_state, mpm_tear_measure,
// mpm_tear_face; mpm_tear.h) ----
// the torn faces of every cloth, counted on the device (zeros while the tables do not exist)
static int tear_counts(mpm_engine* e, std::vector<uint32_t>& n) {
    const size_t nc = e->cloths.size();
    n.assign(nc, 0u);
    if (!e->tear.on() || nc == 0) return 0;
    hipLaunchKernelGGL(k_tear_count, dim3((unsigned)nc), dim3(256), 0, e->stream, (const uint8_t*)e->tear.args.torn, e->tear.d_ranges,
                       e->tear.d_count);
    HIP_TRY(hipGetLastError());
    D2H(e, n.data(), e->tear.d_count, nc * sizeof(uint32_t));
    return 0;
}
// the feature of cloth c that does not compose with tearing (hinges across a torn face, a hole in a pressurised cloth:
// out of scope), or null; of several the first in the order of mpm_features.h
// (mpm_set_tear_coupling lifts two of them: shell bending with MPM_TEAR_CUTS_HINGES, gas mode with MPM_TEAR_VENTS_GAS;
// quadratic bending and constant pressure stay refused whatever the mask)
static bool tear_couples_shell(const mpm_engine* e) { return (e->tear_coupling & MPM_TEAR_CUTS_HINGES) != 0u; }
static bool tear_couples_pressure(const mpm_engine* e, uint32_t mode) {
    return (e->tear_coupling & MPM_TEAR_VENTS_GAS) != 0u && mode == MPM_PRESSURE_GAS;
}
static const char* tear_conflict(const mpm_engine* e, size_t c) {
    if (c < e->bend.k.size() && e->bend.k[c] > 0.f) return FEATURES[F_BENDING].phrase;
    if (c < e->pressure.set.size() && e->pressure.set[c].mode != MPM_PRESSURE_OFF && !tear_couples_pressure(e, e->pressure.set[c].mode))
        return FEATURES[F_PRESSURE].phrase;
    if (c < e->shell.set.size() && e->shell.set[c].stiffness > 0.f && !tear_couples_shell(e)) return FEATURES[F_SHELL].phrase;
    return nullptr;
}
// mpm_set_bending, mpm_set_shell_bending, mpm_set_pressure: refused for a cloth c with wants(c) that has a tear limit or
// a torn face
template <class Wants>
static int tear_refuses(mpm_engine* e, size_t n_cloths, const char* call, Wants wants) {
    if (!e->tear.on()) return 0;
    bool any = false;
    for (size_t c = 0; c < n_cloths; ++c) any = any || wants(c);
    if (!any) return 0;
    if (int rc = settle(e)) return rc;   // (the substeps still owed may tear)
    std::vector<uint32_t> n;
    if (int rc = tear_counts(e, n)) return rc;
    for (size_t c = 0; c < n_cloths && c < n.size(); ++c)
        if (wants(c) && (e->tear.limit(c) || n[c] != 0u))
            return fail(MPM_ERR_INVALID, std::string(call) + ": cloth " + std::to_string(c) +
                                             " has a tear limit or a torn face (mpm_set_tearing, mpm_set_torn_faces): hinges "
                                             "and pressure across torn faces are not available");
    return 0;
}
// Puts the limits `t` (checked; one per cloth, or none) in force, and the flags `torn` if given (n_faces bytes by
// original id; null: the flags stay as they are).  The tables exist while some cloth has a limit or some face is
// flagged; otherwise they are freed and the engine launches what it launched before.  The caller has settled the owed
// substeps.  A failure changes nothing.
static int tear_apply(mpm_engine* e, std::vector<mpm_cloth_tear_t> t, const uint8_t* torn) {
    const size_t nc = e->cloths.size(), nf = e->nf;
    std::vector<float> lim(std::max<size_t>(nc, 1), 0.f), L(std::max<size_t>(nc, 1), 0.f);
    for (size_t c = 0; c < nc && c < t.size(); ++c) lim[c] = t[c].stretch_limit;
    std::vector<size_t> first(nc), count(nc);
    for (size_t c = 0; c < nc; ++c) {
        first[c] = e->cloths[c].first_face;
        count[c] = e->cloths[c].n_faces;
    }
    std::vector<int> cloth_of_face(std::max<size_t>(nf, 1), 0), ranges(2 * std::max<size_t>(nc, 1), 0);
    if (!tear_tables(nc, first.data(), count.data(), lim.data(), nf, L.data(), cloth_of_face.data(), ranges.data()))
        return fail(MPM_ERR_INVALID, "tearing: a stretch_limit is neither 0 nor a finite number > 1");
    bool any = false;
    for (size_t c = 0; c < nc; ++c) any = any || L[c] > 0.f;
    std::vector<uint8_t> flags;
    if (torn) {
        flags.resize(nf);
        for (size_t f = 0; f < nf; ++f) {
            flags[f] = torn[f] != 0 ? 1 : 0;
            any = any || flags[f] != 0;
        }
    } else if (!any) {
        std::vector<uint32_t> n;
        if (int rc = tear_counts(e, n)) return rc;
        for (uint32_t k : n) any = any || k != 0u;
    }
    // (a synchronisation point: the kernels enqueued so far have read the old tables)
    HIP_TRY(hipStreamSynchronize(e->stream));
    if (!any || nf == 0 || nc == 0) {
        mpm_engine::Tear& o = e->tear;
        float* o_L = const_cast<float*>(o.args.L);
        int* o_cloth = const_cast<int*>(o.args.cloth_of_face);
        int2* o_ranges = const_cast<int2*>(o.d_ranges);
        e->dfree(o_L);
        e->dfree(o_cloth);
        e->dfree(o.args.torn);
        e->dfree(o_ranges);
        e->dfree(o.d_count);
        o = mpm_engine::Tear{};
        o.t.swap(t);
        return 0;
    }
    if (!e->tear.on()) {
        mpm_engine::Tear next;
        FreshArrays fresh(e);
        float* d_L = nullptr;
        int* d_cloth = nullptr;
        uint8_t* d_torn = nullptr;
        int2* d_ranges = nullptr;
        if (int rc = fresh.alloc(&d_L, nc, false)) return rc;
        if (int rc = fresh.alloc(&d_cloth, nf, false)) return rc;
        if (int rc = fresh.alloc(&d_torn, nf, true)) return rc;
        if (int rc = fresh.alloc(&d_ranges, nc, false)) return rc;
        if (int rc = fresh.alloc(&next.d_count, nc, true)) return rc;
        H2D(e, d_cloth, cloth_of_face.data(), nf * sizeof(int));
        H2D(e, d_ranges, ranges.data(), nc * sizeof(int2));
        H2D(e, d_L, L.data(), nc * sizeof(float));
        if (torn) H2D(e, d_torn, flags.data(), nf);
        next.args = TearArgs{d_L, d_cloth, d_torn};
        next.d_ranges = d_ranges;
        next.t.swap(t);
        e->tear = next;
        fresh.commit();
        return 0;
    }
    H2D(e, const_cast<float*>(e->tear.args.L), L.data(), nc * sizeof(float));
    if (torn) H2D(e, e->tear.args.torn, flags.data(), nf);
    e->tear.t.swap(t);
    return 0;
}
// mpm_set_tearing: the limits are checked by the entry point
static int set_tearing(mpm_engine* e, size_t n_cloths, const mpm_cloth_tear_t* t) {
    for (size_t c = 0; c < n_cloths; ++c)
        if (t[c].stretch_limit > 0.f)
            if (const char* other = tear_conflict(e, c))
                return fail(MPM_ERR_INVALID, "mpm_set_tearing: cloth " + std::to_string(c) + " has " + other + ", which tearing does not compose with");
    // substeps that mpm_run_substeps deferred are owed with the limits they were enqueued with
    if (int rc = settle(e)) return rc;
    return tear_apply(e, std::vector<mpm_cloth_tear_t>(t, t + n_cloths), nullptr);
}
// mpm_set_torn_faces: scissors / restore
static int set_torn_faces(mpm_engine* e, const uint8_t* torn) {
    for (size_t c = 0; c < e->cloths.size(); ++c) {
        const mpm_engine::Cloth& cl = e->cloths[c];
        bool cut = false;
        for (size_t f = cl.first_face; f < cl.first_face + cl.n_faces; ++f) cut = cut || torn[f] != 0;
        if (cut)
            if (const char* other = tear_conflict(e, c))
                return fail(MPM_ERR_INVALID, "mpm_set_torn_faces: cloth " + std::to_string(c) + " has " + other + ", which tearing does not compose with");
    }
    if (int rc = settle(e)) return rc;
    return tear_apply(e, e->tear.t, torn);
}
// mpm_tear_state: the flags and the count per cloth (k_tear_count)
static int tear_state(mpm_engine* e, uint8_t* torn_out, uint32_t* count_per_cloth, size_t capacity, size_t* n_out) {
    std::vector<uint32_t> n;
    if (int rc = tear_counts(e, n)) return rc;
    if (count_per_cloth) std::copy(n.begin(), n.begin() + (long)std::min(capacity, n.size()), count_per_cloth);
    if (n_out) *n_out = n.size();
    if (torn_out && e->nf) {
        if (e->tear.on()) D2H(e, torn_out, e->tear.args.torn, e->nf);
        else std::memset(torn_out, 0, e->nf);
    }
    return 0;
}
// mpm_tear_measure: one launch of k_tear_eval on the current state, by original face id
static int tear_measure(mpm_engine* e, float* mq_out, uint8_t* would_fail_out) {
    const size_t nf = e->nf;
    if (nf == 0) return 0;
    if (int rc = e->stage(9 * nf)) return rc;
    HIP_TRY(hipMemsetAsync(e->d_stage, 0, 9 * nf, e->stream));
    float* d_mq = (float*)e->d_stage;
    uint8_t* d_fail = (uint8_t*)e->d_stage + 8 * nf;
    hipLaunchKernelGGL(k_tear_eval, dim3((unsigned)((nf + 255) / 256)), dim3(256), 0, e->stream, e->dp, e->tear.args, d_mq, d_fail);
    HIP_TRY(hipGetLastError());
    if (mq_out) D2H(e, mq_out, d_mq, 8 * nf);
    if (would_fail_out) D2H(e, would_fail_out, d_fail, nf);
    return 0;
}
// host code only: the device function of the kernels, compiled for the host
static int tear_faces(size_t n, const float* dminv3, const float* x9, const float* L, float* mq_out, uint8_t* fails_out) {
    for (size_t f = 0; f < n; ++f) {
        float x[3][3], mq[2];
        std::memcpy(x, x9 + 9 * f, sizeof x);
        const bool fails = tear_face(dminv3[3 * f], dminv3[3 * f + 1], dminv3[3 * f + 2], L[f], x, mq);
        if (mq_out) std::memcpy(mq_out + 2 * f, mq, sizeof mq);
        if (fails_out) fails_out[f] = fails ? 1 : 0;
    }
    return 0;
}

// ---- tearing composed with shell bending and gas (mpm_set_tear_coupling, mpm_get_tear_coupling, mpm_shell_cut_hinges,
// mpm_pressure_vented, mpm_mesh_hinge_faces; mpm_shell.h CUT HINGES, mpm_pressure.h VENTED GAS) ----
// mpm_set_tear_coupling: the mask is checked by the entry point and the owed substeps are settled.  A bit may not be
// cleared while some cloth holds the combination it permits: a tear limit or a torn face (counted on the device, as
// tear_refuses does) together with shell k > 0 (MPM_TEAR_CUTS_HINGES) or gas mode (MPM_TEAR_VENTS_GAS).
static int set_tear_coupling(mpm_engine* e, uint32_t mask) {
    const uint32_t cleared = e->tear_coupling & ~mask;
    if (cleared != 0u && e->tear.on()) {
        std::vector<uint32_t> n;
        if (int rc = tear_counts(e, n)) return rc;
        for (size_t c = 0; c < e->cloths.size(); ++c) {
            if (!(e->tear.limit(c) || n[c] != 0u)) continue;
            const bool shell = (cleared & MPM_TEAR_CUTS_HINGES) != 0u && c < e->shell.set.size() && e->shell.set[c].stiffness > 0.f;
            const bool gas = (cleared & MPM_TEAR_VENTS_GAS) != 0u && c < e->pressure.set.size() && e->pressure.set[c].mode == MPM_PRESSURE_GAS;
            if (shell || gas)
                return fail(MPM_ERR_INVALID, "mpm_set_tear_coupling: cloth " + std::to_string(c) +
                                                 " has a tear limit or a torn face (mpm_set_tearing, mpm_set_torn_faces) and " +
                                                 (shell ? "shell bending (mpm_set_shell_bending)" : "gas pressure (mpm_set_pressure)") +
                                                 ": " + (shell ? "MPM_TEAR_CUTS_HINGES" : "MPM_TEAR_VENTS_GAS") +
                                                 " cannot be cleared while it does");
        }
    }
    e->tear_coupling = mask;
    return 0;
}
// mpm_shell_cut_hinges: the hinge records of the current positions and flags (k_hinge_eval), then plane 3's .w per hinge
static int shell_cut_hinges(mpm_engine* e, uint8_t* cut_out, uint32_t* cut_per_cloth, size_t capacity, size_t* n_out) {
    const mpm_engine::Shell& sh = e->shell;
    const size_t n = sh.on() ? (size_t)sh.hinge.n : 0;
    std::vector<uint32_t> count(e->cloths.size(), 0u);
    if (n) {
        if (int rc = shell_measure(e)) return rc;
        std::vector<float4> plane3(n);
        D2H(e, plane3.data(), sh.hinge.rec + 3 * n, n * sizeof(float4));
        for (size_t h = 0; h < n; ++h) {
            const bool cut = plane3[h].w > 0.f;
            if (cut_out) cut_out[h] = cut ? 1 : 0;
            if (cut) count[(size_t)sh.hinge_cloth[h]] += 1u;
        }
    }
    return copy_out(count, cut_per_cloth, capacity, n_out);
}
// mpm_pressure_vented: volumes and gauges anew (pressure_measure), then the words k_pressure_volume left per chunk of
// the list of all cloths, ORed per cloth; a cloth is vented only in gas mode
static int pressure_vented_cloths(mpm_engine* e, uint8_t* vented_per_cloth, size_t capacity, size_t* n_out) {
    const size_t nc = e->cloths.size();
    std::vector<uint8_t> vented(nc, 0);
    if (coupled_tear_flags(e, MPM_TEAR_VENTS_GAS) && e->pressure.gas()) {
        if (int rc = pressure_measure(e)) return rc;
        const mpm_engine::Pressure& ps = e->pressure;
        std::vector<uint32_t> words((size_t)ps.n_all_chunks);
        std::vector<int4> chunks((size_t)ps.n_all_chunks);
        if (ps.n_all_chunks) {
            D2H(e, words.data(), ps.vol.vent + ps.n_gas_chunks, words.size() * sizeof(uint32_t));
            D2H(e, chunks.data(), ps.vol.chunks + ps.n_gas_chunks, chunks.size() * sizeof(int4));
        }
        for (size_t k = 0; k < words.size(); ++k) {
            const size_t c = (size_t)chunks[k].x;
            if (words[k] != 0u && c < ps.set.size() && ps.set[c].mode == MPM_PRESSURE_GAS) vented[c] = 1;
        }
    }
    return copy_out(vented, vented_per_cloth, capacity, n_out);
}
// host only: faces A and B of every hinge of mesh_hinges, cloth-local ids
static int mesh_hinge_faces(const int32_t* indices, size_t n_faces, int32_t* faces2, size_t capacity, size_t* n_out) {
    std::vector<ShellHinge> H;
    mesh_hinges(indices, n_faces, H);
    for (size_t h = 0; h < std::min(capacity, H.size()); ++h) {
        faces2[2 * h] = H[h].face_a;
        faces2[2 * h + 1] = H[h].face_b;
    }
    if (n_out) *n_out = H.size();
    return 0;
}

// ---- the rest shape apart from the pose (mpm_set_rest_shape, mpm_get_rest_shape, mpm_rest_shape_check; mpm_rest.h) ----
// host code only: the first face (or -1) whose rest edge e0 = xb - xa or rest area |e0 x e1| is zero, in double from the
// float positions -- the two numbers Finalize divides by (the rotations' q2 and det Dm).  No conditioning threshold:
// Finalize has none.  A non-finite coordinate makes its faces bad (the comparisons are false for a NaN).
static int32_t rest_shape_first_bad_face(const float* rest_pos, const int32_t* indices, size_t n_faces) {
    for (size_t f = 0; f < n_faces; ++f) {
        const float *a = rest_pos + 3 * (size_t)indices[3 * f], *b = rest_pos + 3 * (size_t)indices[3 * f + 1],
                    *c = rest_pos + 3 * (size_t)indices[3 * f + 2];
        const double e0[3] = {(double)b[0] - a[0], (double)b[1] - a[1], (double)b[2] - a[2]};
        const double e1[3] = {(double)c[0] - a[0], (double)c[1] - a[1], (double)c[2] - a[2]};
        const double n[3] = {e0[1] * e1[2] - e0[2] * e1[1], e0[2] * e1[0] - e0[0] * e1[2], e0[0] * e1[1] - e0[1] * e1[0]};
        const double l2 = e0[0] * e0[0] + e0[1] * e0[1] + e0[2] * e0[2], n2 = n[0] * n[0] + n[1] * n[1] + n[2] * n[2];
        if (!(l2 > 0.0 && l2 < INFINITY) || !(n2 > 0.0 && n2 < INFINITY)) return (int32_t)f;
    }
    return -1;
}
static int rest_shape_check(const float* rest_pos, size_t n_verts, const int32_t* indices, size_t n_faces, int32_t* first_bad_face_out) {
    if (first_bad_face_out) *first_bad_face_out = -1;
    for (size_t i = 0; i < 3 * n_faces; ++i)
        REQUIRE(indices[i] >= 0 && (size_t)indices[i] < n_verts, "triangle index out of range");
    const int32_t bad = rest_shape_first_bad_face(rest_pos, indices, n_faces);
    if (first_bad_face_out) *first_bad_face_out = bad;
    if (bad >= 0)
        return fail(MPM_ERR_INVALID, "rest shape: face " + std::to_string(bad) + ": its first edge or its area is zero or not finite");
    for (size_t i = 0; i < 3 * n_verts; ++i) REQUIRE(std::isfinite(rest_pos[i]), "rest shape: a coordinate is not finite");
    return 0;
}
// mpm_set_rest_shape: the checks on the host in double, the owed substeps, then k_rest_faces and k_rest_vertices on the
// current particle order and the fixed-point scales from the new masses.  rest_pos null: the positions as added.  A
// refusal enqueues nothing: the rest state in force stays.
static int set_rest_shape(mpm_engine* e, const float* rest_pos) {
    // (a table in force whose host side caches something derived from the rest positions, Dm^-1, the volumes or the masses --
    // FeatureRow::caches_rest, mpm_features.h: the caller clears it, sets the rest shape and sets it again)
    if (const Feature other = rest_shape_blocker(feature_state(e)); other != F_NONE)
        return fail(MPM_ERR_INVALID, std::string("mpm_set_rest_shape: the engine has ") + FEATURES[other].phrase +
                                         ", which holds values derived from the rest shape: clear it, set the rest shape, set it again");
    const float* R = rest_pos ? rest_pos : e->h_pos.data();
    for (size_t i = 0; i < 3 * e->nv; ++i) REQUIRE(std::isfinite(R[i]), "mpm_set_rest_shape: a coordinate is not finite");
    const int32_t bad = rest_shape_first_bad_face(R, e->h_idx.data(), e->nf);
    if (bad >= 0)
        return fail(MPM_ERR_INVALID, "mpm_set_rest_shape: face " + std::to_string(bad) + ": its first rest edge or its rest area is zero");
    // substeps that mpm_run_substeps deferred are owed with the rest state they were enqueued with
    if (int rc = settle(e)) return rc;
    const size_t nv = e->nv, nf = e->nf, np = e->np;
    // staging: the rest positions, behind them the quarter volumes by original face id, then the densities by original id
    const size_t off_quarter = 3 * nv, off_rho = off_quarter + nf, n_float = off_rho + (e->multi_mat ? np : 0);
    if (int rc = e->stage(std::max<size_t>(n_float, 1) * 4)) return rc;
    float* d = (float*)e->d_stage;
    if (nv) H2D(e, d, R, 3 * nv * 4);
    if (e->multi_mat) H2D(e, d + off_rho, e->h_rho_of_pid.data(), np * 4);
    const RestArgs a{d, d + off_quarter, e->multi_mat ? d + off_rho : nullptr};
    if (nf) hipLaunchKernelGGL(k_rest_faces, dim3(e->g_nf), dim3(256), 0, e->stream, e->dp, a);
    if (nv) hipLaunchKernelGGL(k_rest_vertices, dim3(e->g_nv), dim3(256), 0, e->stream, e->dp, a);
    HIP_TRY(hipGetLastError());
    // (a synchronisation point: it reads the new masses back)
    if (int rc = set_fixed_point_scales(e)) return rc;
    e->h_rest.assign(R, R + 3 * nv);
    e->rest_set = rest_pos != nullptr;
    return 0;
}

// ---- the per-cloth report (mpm_measure, mpm_face_strain, mpm_cloth_energy_density; mpm_measure.h) ----
// The chunk table: every cloth's faces, then every cloth's vertices, in runs of at most MEASURE_CHUNK original ids that
// never straddle a cloth.  Built once; the vertex chunks' rows of the bending table follow mpm_set_bending.
static int measure_ready(mpm_engine* e) {
    mpm_engine::Measure& ms = e->measure;
    const size_t nc = e->cloths.size();
    if (!ms.built) {
        std::vector<int4> chunks, ranges(nc, make_int4(0, 0, 0, 0));
        const int nfg = e->dp.NfG;
        for (int pass = 0; pass < 2; ++pass) {
            for (size_t c = 0; c < nc; ++c) {
                const mpm_engine::Cloth& cl = e->cloths[c];
                const int first = pass == 0 ? (int)cl.first_face : nfg + (int)cl.first_vertex;
                const int end = first + (int)(pass == 0 ? cl.n_faces : cl.n_verts);
                (pass == 0 ? ranges[c].x : ranges[c].z) = (int)chunks.size();
                for (int b = first; b < end; b += MEASURE_CHUNK) chunks.push_back(make_int4((int)c, b, std::min(end, b + MEASURE_CHUNK), -1));
                (pass == 0 ? ranges[c].y : ranges[c].w) = (int)chunks.size();
            }
            if (pass == 0) ms.n_face_chunks = (int)chunks.size();
        }
        ms.n_vertex_chunks = (int)chunks.size() - ms.n_face_chunks;
        FreshArrays fresh(e);
        int4 *d_chunks = nullptr, *d_ranges = nullptr;
        mpm_cloth_measure_t *d_rows = nullptr, *d_out = nullptr;
        if (int rc = fresh.alloc(&d_chunks, chunks.size(), false)) return rc;
        if (int rc = fresh.alloc(&d_ranges, nc, false)) return rc;
        if (int rc = fresh.alloc(&d_rows, chunks.size(), true)) return rc;
        if (int rc = fresh.alloc(&d_out, nc, true)) return rc;
        if (nc) H2D(e, d_ranges, ranges.data(), nc * sizeof(int4));
        fresh.commit();
        ms.d_chunks = d_chunks; ms.d_ranges = d_ranges; ms.d_rows = d_rows; ms.d_out = d_out;
        ms.chunks.swap(chunks);
        ms.rows_stale = true;
        ms.built = true;
    }
    if (ms.rows_stale || ms.k_seen != e->bend.k) {
        // row of the bending table of every cloth's first vertex: the table holds the cloths with k > 0, in cloth order
        std::vector<int> row0(nc, -1);
        int r = 0;
        for (size_t c = 0; c < nc && e->bend.on(); ++c)
            if (c < e->bend.k.size() && e->bend.k[c] > 0.f) {
                row0[c] = r;
                r += (int)e->cloths[c].n_verts;
            }
        if (r != (e->bend.on() ? e->bend.args.n_rows : 0)) return fail(MPM_ERR_INTERNAL, "mpm_measure: the bending table does not match the cloths");
        for (int k = ms.n_face_chunks; k < (int)ms.chunks.size(); ++k) {
            int4& ch = ms.chunks[(size_t)k];
            const int base = e->dp.NfG + (int)e->cloths[(size_t)ch.x].first_vertex;
            ch.w = row0[(size_t)ch.x] < 0 ? -1 : row0[(size_t)ch.x] + (ch.y - base);
        }
        if (!ms.chunks.empty()) H2D(e, ms.d_chunks, ms.chunks.data(), ms.chunks.size() * sizeof(int4));
        ms.k_seen = e->bend.k;
        ms.rows_stale = false;
    }
    return 0;
}
static MeasureArgs measure_args(const mpm_engine* e) {
    const mpm_engine::Measure& ms = e->measure;
    MeasureArgs a{};
    a.chunks = ms.d_chunks;
    a.n_face_chunks = ms.n_face_chunks;
    a.n_vertex_chunks = ms.n_vertex_chunks;
    a.rows = ms.d_rows;
    a.mats = e->multi_mat ? e->d_cloth_mat : nullptr;
    a.bend = e->bend.args;
    a.torn = e->tear.args.torn;
    return a;
}

static int measure_cloths(mpm_engine* e, mpm_cloth_measure_t* per_cloth, size_t capacity, size_t* n_cloths_out,
                          mpm_cloth_measure_t* total) {
    if (int rc = measure_ready(e)) return rc;
    const size_t nc = e->cloths.size();
    const MeasureArgs a = measure_args(e);
    // at most three launches: face chunks, vertex chunks, one workgroup per cloth
    if (a.n_face_chunks) hipLaunchKernelGGL(k_measure_faces, dim3((unsigned)a.n_face_chunks), dim3(256), 0, e->stream, e->dp, a);
    if (a.n_vertex_chunks) hipLaunchKernelGGL(k_measure_vertices, dim3((unsigned)a.n_vertex_chunks), dim3(256), 0, e->stream, e->dp, a);
    std::vector<mpm_cloth_measure_t> rows(nc);
    if (nc) {
        hipLaunchKernelGGL(k_measure_final, dim3((unsigned)nc), dim3(256), 0, e->stream, a, (const int4*)e->measure.d_ranges,
                           e->measure.d_out);
        HIP_TRY(hipGetLastError());
        D2H(e, rows.data(), e->measure.d_out, nc * sizeof(mpm_cloth_measure_t));
    }
    std::copy(rows.begin(), rows.begin() + (long)std::min(capacity, nc), per_cloth);
    if (n_cloths_out) *n_cloths_out = nc;
    if (total) {
        mpm_cloth_measure_t t{};
        t.stretch_min = INFINITY;
        t.normal_min = INFINITY;
        double* ts = reinterpret_cast<double*>(&t);
        for (const mpm_cloth_measure_t& r : rows) {
            const double* rs = reinterpret_cast<const double*>(&r);
            for (int k = 0; k < MEASURE_SUMS; ++k) ts[k] += rs[k];
            t.stretch_max = std::max(t.stretch_max, r.stretch_max);
            t.stretch_min = std::min(t.stretch_min, r.stretch_min);
            t.normal_min = std::min(t.normal_min, r.normal_min);
            t.speed_max = std::max(t.speed_max, r.speed_max);
            t.faces += r.faces;
            t.vertices += r.vertices;
        }
        *total = t;
    }
    return 0;
}

static int face_strain(mpm_engine* e, float* out) {
    if (e->nf == 0) return 0;
    if (int rc = measure_ready(e)) return rc;
    const MeasureArgs a = measure_args(e);
    const size_t bytes = e->nf * 16;
    if (int rc = e->stage(bytes)) return rc;
    HIP_TRY(hipMemsetAsync(e->d_stage, 0, bytes, e->stream));
    hipLaunchKernelGGL(k_measure_face_strain, dim3((unsigned)a.n_face_chunks), dim3(256), 0, e->stream, e->dp, a, (float*)e->d_stage);
    HIP_TRY(hipGetLastError());
    D2H(e, out, e->d_stage, bytes);
    return 0;
}

// host code only: the device function of the kernels, compiled for the host
static int cloth_energy_densities(const mpm_cloth_material_t* m, size_t n, const float* F, double* out) {
    float mu, lambda;   // (as mpm_finalize forms them, in float)
    lame(m->youngs_modulus, m->poisson_ratio, &mu, &lambda);
    for (size_t i = 0; i < n; ++i) {
        const float* f = F + 9 * i;
        const double d1[3] = {(double)f[0], (double)f[3], (double)f[6]}, d2[3] = {(double)f[1], (double)f[4], (double)f[7]};
        const double d3[3] = {(double)f[2], (double)f[5], (double)f[8]};
        cloth_energy_density(mu, lambda, m->K, m->gamma, d1, d2, d3, out + 6 * i);
    }
    return 0;
}
