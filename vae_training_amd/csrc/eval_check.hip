// Host only: the one refusal list of the evaluation entry points (eval_check.h), the adapters of the nine description structs and
// the small checks they and the training entry points of api.hip share, the Hessian entry points' further buffer checks, and the
// training entry points' own list.  No kernels (lanczos_dev.h for the two caps the Hessian checks print).
#include "eval_check.h"
#include "lanczos_dev.h"

namespace vaek {

// ---- one adapter per description: the head every struct has, then what this one has and lacks ---------------------------------------
// false: NULL, or another header's size -- the fields behind struct_size stay unread
template <class T>
static bool desc_head(EvalDesc* e, const char* name, const T* d) {
    e->name = name; e->given = d != nullptr; e->want = sizeof(T);
    if (!d) return false;
    e->struct_size = d->struct_size;
    if (d->struct_size != (int32_t)sizeof(T)) return false;
    e->n = d->n; e->rows = d->rows; e->state_stride = d->state_stride;
    e->out = d->out; e->out_stride = d->out_stride;
    return true;
}

// the two event descriptions: both streams and sample_eps always read, no explicit rows (an event always draws)
template <class T>
static EvalDesc describe_event(const char* name, const T* d, bool out_doubles) {
    EvalDesc e{};
    if (!desc_head(&e, name, d)) return e;
    e.x_seeds = d->x_seeds; e.x_steps = d->x_steps; e.x_need = Need::ALWAYS;
    e.z_seeds = d->z_seeds; e.z_steps = d->z_steps; e.z_need = Need::ALWAYS;
    e.sample_eps = d->sample_eps; e.eps_need = Need::ALWAYS;
    e.a_stride = d->a_stride; e.out_doubles = out_doubles;
    return e;
}
EvalDesc describe(const vaek_stats_event* d) { return describe_event("vaek_stats_event", d, false); }
EvalDesc describe(const vaek_spectrum_event* d) { return describe_event("vaek_spectrum_event", d, true); }

EvalDesc describe(const vaek_log_likelihood* d) {
    EvalDesc e{};
    if (!desc_head(&e, "vaek_log_likelihood", d)) return e;
    e.x_seeds = d->x_seeds; e.x_steps = d->x_steps; e.x_need = Need::DRAWING;
    e.z_seeds = d->z_seeds; e.z_steps = d->z_steps; e.z_need = Need::ALWAYS;      // no sample_eps
    e.a_stride = d->a_stride;
    e.rows_name = "x"; e.rows_ptr = d->x; e.rows_stride = d->x_stride; e.rows_dim = 'D';
    return e;
}

// the descriptions of the exact calls and of the sampled Hessian's: x rows, no z_seeds / z_steps, no sample_eps, records of doubles
template <class T>
static EvalDesc describe_exact(const char* name, const T* d) {
    EvalDesc e{};
    if (!desc_head(&e, name, d)) return e;
    e.x_seeds = d->x_seeds; e.x_steps = d->x_steps; e.x_need = Need::DRAWING;
    e.a_stride = d->a_stride; e.out_doubles = true;
    e.rows_name = "x"; e.rows_ptr = d->x; e.rows_stride = d->x_stride; e.rows_dim = 'D';
    return e;
}
EvalDesc describe(const vaek_exact_log_likelihood* d) { return describe_exact("vaek_exact_log_likelihood", d); }
EvalDesc describe(const vaek_elbo_hvp* d) { return describe_exact("vaek_elbo_hvp", d); }
EvalDesc describe(const vaek_elbo_hessian* d) { return describe_exact("vaek_elbo_hessian", d); }
// the sampled calls: the exact calls' head; samples, z_seeds / z_steps and xi are read by their unit (xi == NULL is what draws them)
EvalDesc describe(const vaek_sampled_elbo_hvp* d) { return describe_exact("vaek_sampled_elbo_hvp", d); }
EvalDesc describe(const vaek_sampled_elbo_hessian* d) { return describe_exact("vaek_sampled_elbo_hessian", d); }

EvalDesc describe(const vaek_decoder_jacobian* d) {
    EvalDesc e{};
    if (!desc_head(&e, "vaek_decoder_jacobian", d)) return e;
    e.z_seeds = d->z_seeds; e.z_steps = d->z_steps; e.z_need = Need::DRAWING;      // no x_seeds / x_steps, sample_eps or a_stride: latent rows
    e.out_doubles = true;
    e.rows_name = "z"; e.rows_ptr = d->z; e.rows_stride = d->z_stride; e.rows_dim = 'L';
    return e;
}

// ---- the list ------------------------------------------------------------------------------------------------------------------------
static int check_present(const char* who, const void* p, const char* field, Need need, bool explicit_rows) {
    if (p || need == Need::ABSENT || (need == Need::DRAWING && explicit_rows)) return VAEK_OK;
    set_error("%s: %s is NULL%s", who, field, need == Need::DRAWING ? " (drawing mode reads it)" : "");
    return VAEK_ERR_INVALID;
}

// explicit rows of `width` floats each: stride 0 (one set shared) or at least a replica's rows
static int check_rows_stride(const char* who, const char* name, char dim, int64_t stride, int32_t rows, int width) {
    if (stride < 0 || (stride > 0 && stride < (int64_t)rows * width)) {
        set_error("%s: %s_stride %lld: need 0 (shared rows) or >= rows * %c = %lld", who, name, (long long)stride, dim, (long long)rows * width);
        return VAEK_ERR_INVALID;
    }
    return VAEK_OK;
}

int check_eval(const char* who, const vaek_ctx* ctx, const float* params, const EvalDesc& d, const EvalRules& r) {
    if (!d.given) { set_error("%s: null description", who); return VAEK_ERR_INVALID; }
    if (int rc = check_struct_size(who, d.name, d.struct_size, d.want)) return rc;
    if (!ctx || !params) { set_error("%s: null context or params", who); return VAEK_ERR_INVALID; }
    if (!r.covered) { set_error("%s: %s", who, r.needs); return VAEK_ERR_INVALID; }
    if (int rc = check_replica_count(who, d.n)) return rc;
    if (int rc = check_row_count(who, d.rows, r.rows_min, r.rows_cap, r.rows_query)) return rc;
    const bool ex = d.explicit_rows();
    if (int rc = check_present(who, d.x_seeds, "x_seeds", d.x_need, ex)) return rc;
    if (int rc = check_present(who, d.x_steps, "x_steps", d.x_need, ex)) return rc;
    if (int rc = check_present(who, d.z_seeds, "z_seeds", d.z_need, ex)) return rc;
    if (int rc = check_present(who, d.z_steps, "z_steps", d.z_need, ex)) return rc;
    if (int rc = check_present(who, d.sample_eps, "sample_eps", d.eps_need, ex)) return rc;
    if (int rc = check_present(who, d.out, "out", Need::ALWAYS, ex)) return rc;
    if (d.state_stride < ctx->P) {
        set_error("%s: state_stride %lld < P = %lld (vaek_param_count)", who, (long long)d.state_stride, (long long)ctx->P);
        return VAEK_ERR_INVALID;
    }
    if (d.out_stride < r.records * r.record_len) {
        set_error("%s: out_stride %lld < %d x record length %lld (%s)", who, (long long)d.out_stride, r.records, (long long)r.record_len, r.record_query);
        return VAEK_ERR_INVALID;
    }
    if (d.out_doubles)
        if (int rc = check_aligned8(who, "out", (uintptr_t)d.out)) return rc;
    if (ex) {
        if (int rc = check_rows_stride(who, d.rows_name, d.rows_dim, d.rows_stride, d.rows, d.rows_dim == 'D' ? ctx->D : ctx->L)) return rc;
    } else if (r.draws) {
        if (int rc = check_dataset_draw(who, ctx, r.kind, r.A, r.dd, r.did, r.pad, d.a_stride, r.x_tag)) return rc;
    }
    if (r.has_z_tag)
        if (int rc = check_tag(who, r.z_tag)) return rc;
    if (r.ws_align && (!r.workspace || ((uintptr_t)r.workspace & (uintptr_t)(r.ws_align - 1)) != 0)) {
        set_error("%s: workspace is NULL or not %d-byte aligned (%s)", who, r.ws_align, r.ws_query);
        return VAEK_ERR_INVALID;
    }
    return VAEK_OK;
}

void fill_rows_source(BatchArgs* gen, long long* a_stride_out, const vaek_ctx* ctx, int rows, bool explicit_rows, int32_t kind, const float* A,
                      int32_t dd, int32_t did, int32_t pad, float var_added, uint32_t x_tag, int64_t a_stride) {
    if (explicit_rows) {
        fill_draw_args(gen, ctx, rows, 2, nullptr, 0, 0, 0, 0.f, 0);
    } else {
        *a_stride_out = a_stride;
        fill_draw_args(gen, ctx, rows, kind, A, dd, did, pad, var_added, x_tag);
    }
}

// ---- the counted quantities ------------------------------------------------------------------------------------------------------------
int check_replica_count(const char* who, int32_t n, int cap, const char* cap_query) {
    if (n < 1 || n > cap) {
        set_error("%s: %d replicas, need 1 .. %d (%s)", who, n, cap, cap_query);
        return VAEK_ERR_INVALID;
    }
    return VAEK_OK;
}

int check_row_count(const char* who, int32_t rows, int rows_min, int rows_cap, const char* rows_query) {
    if (rows < rows_min || rows > rows_cap) {
        set_error("%s: %d rows, need %d .. %d (%s)", who, rows, rows_min, rows_cap, rows_query);
        return VAEK_ERR_INVALID;
    }
    return VAEK_OK;
}

int check_sample_count(const char* who, int32_t samples) {
    if (samples < 1 || samples > kLogLikMaxSamples) {
        set_error("%s: %d samples, need 1 .. %d (vaek_log_likelihood_max_samples)", who, samples, kLogLikMaxSamples);
        return VAEK_ERR_INVALID;
    }
    return VAEK_OK;
}

int check_column_count(const char* who, int32_t n, int32_t rows, int32_t per_row, const char* unit, int cap, const char* cap_query) {
    const long long columns = (long long)n * rows * per_row;
    if (columns > cap) {
        set_error("%s: %d replicas x %d rows x %d %s = %lld columns, at most %d (%s)", who, n, rows, per_row, unit, columns, cap, cap_query);
        return VAEK_ERR_INVALID;
    }
    return VAEK_OK;
}

// ---- the in-kernel dataset draw --------------------------------------------------------------------------------------------------------
int check_dataset_draw(const char* who, const vaek_ctx* ctx, int32_t kind, const float* A, int32_t dd, int32_t did, int32_t pad,
                       int64_t a_stride, uint32_t x_tag, bool empty_did) {
    if (a_stride < 0) { set_error("%s: a_stride %lld < 0", who, (long long)a_stride); return VAEK_ERR_INVALID; }
    if (kind < 0 || kind > 2) { set_error("%s: kind %d outside 0 .. 2", who, kind); return VAEK_ERR_INVALID; }
    if (kind != 2 && !A) { set_error("%s: A is NULL (only kind 2 has no matrix)", who); return VAEK_ERR_INVALID; }
    if (dd < 1 || dd > 16 || did > 16 || (kind == 0 && did < 1 && !empty_did) || pad < 0) {
        set_error("%s: dd = %d, did = %d, pad = %d: need 1 <= dd <= 16, did <= 16, pad >= 0", who, dd, did, pad);
        return VAEK_ERR_INVALID;
    }
    if (dd + pad + (kind == 1 ? 1 : 0) != ctx->D) {
        set_error("%s: dataset dimension %d != context data_dim %d", who, dd + pad + (kind == 1 ? 1 : 0), ctx->D);
        return VAEK_ERR_INVALID;
    }
    return check_tag(who, x_tag);
}

void fill_draw_args(BatchArgs* g, const vaek_ctx* ctx, int rows, int32_t kind, const float* A, int32_t dd, int32_t did, int32_t pad,
                    float var_added, uint32_t x_tag, int64_t row0, uint64_t seed, const int32_t* step_dev) {
    g->kind = kind; g->A = kind == 2 ? nullptr : A; g->dd = dd; g->did = did; g->pad = pad;
    g->noise_std = var_added > 0.f ? sqrtf(var_added) : 0.f;
    g->rows = rows; g->row0 = row0; g->D = ctx->D; g->L = ctx->L; g->tag = x_tag;
    g->seed = seed; g->step_dev = step_dev;
}

// ---- the small checks, also the train-loop entry points' -------------------------------------------------------------------------------
int check_struct_size(const char* who, const char* name, int32_t got, size_t want) {
    if (got != (int32_t)want) {
        set_error("%s: %s.struct_size %d != %d (header / library mismatch)", who, name, got, (int)want);
        return VAEK_ERR_INVALID;
    }
    return VAEK_OK;
}

int check_x_stride(const char* who, const vaek_ctx* ctx, int64_t x_stride, int32_t rows) {
    return check_rows_stride(who, "x", 'D', x_stride, rows, ctx->D);
}

int check_tag(const char* who, uint32_t tag) {
    if (tag >= 0x40000000u) { set_error("%s: a tag >= 2^30", who); return VAEK_ERR_INVALID; }
    return VAEK_OK;
}

int check_aligned8(const char* who, const char* what, uintptr_t addrs) {
    if ((addrs & 7u) != 0) { set_error("%s: %s is not 8-byte aligned", who, what); return VAEK_ERR_INVALID; }
    return VAEK_OK;
}

// ---- the Hessian entry points' further arguments (13 .. 15 of eval_check.h) -----------------------------------------------------------
int check_doubles(const char* who, const char* what, const void* ptr, int64_t stride, int64_t len, bool shared_ok) {
    if (!ptr) { set_error("%s: %s is NULL", who, what); return VAEK_ERR_INVALID; }
    if (int rc = check_aligned8(who, what, (uintptr_t)ptr)) return rc;
    const bool shared = stride == 0 && shared_ok;
    if (stride < 0 || (!shared && stride < len)) {
        set_error("%s: %s stride %lld < its length %lld%s", who, what, (long long)stride, (long long)len, shared_ok ? " (0: shared)" : "");
        return VAEK_ERR_INVALID;
    }
    return VAEK_OK;
}

// do the n replicas' spans of two buffers of doubles, each `len` at `stride`, share a byte?
static bool doubles_overlap(const double* p, int64_t stride, int64_t len, const double* q, int64_t qstride, int64_t qlen, int n) {
    const uintptr_t a0 = (uintptr_t)p, a1 = a0 + sizeof(double) * (size_t)((n - 1) * stride + len);
    const uintptr_t b0 = (uintptr_t)q, b1 = b0 + sizeof(double) * (size_t)((n - 1) * qstride + qlen);
    return a0 < b1 && b0 < a1;
}

int check_sampled_columns(const char* who, int32_t n, int32_t rows, int32_t samples, int cap_log2, int call_cap, const char* call_cap_query) {
    if (int rc = check_sample_count(who, samples)) return rc;
    if ((long long)rows * samples > 1 << cap_log2) {
        set_error("%s: %d rows x %d samples = %lld columns per replica, at most %d (rows * samples <= 2^%d; %s bounds n * rows * samples)", who,
                  rows, samples, (long long)rows * samples, 1 << cap_log2, cap_log2, call_cap_query);
        return VAEK_ERR_INVALID;
    }
    return check_column_count(who, n, rows, samples, "samples", call_cap, call_cap_query);
}

int check_sample_source(const char* who, const SampleSource& x, int32_t rows, int L) {
    if (x.xi) {
        const int64_t len = (int64_t)rows * x.samples * L;
        if (x.xi_stride < 0 || (x.xi_stride > 0 && x.xi_stride < len)) {
            set_error("%s: xi_stride %lld: need 0 (shared samples) or >= rows * samples * L = %lld", who, (long long)x.xi_stride, (long long)len);
            return VAEK_ERR_INVALID;
        }
    } else if (!x.z_seeds || !x.z_steps) {
        set_error("%s: %s is NULL (xi == NULL draws the samples and reads it)", who, x.z_seeds ? "z_steps" : "z_seeds");
        return VAEK_ERR_INVALID;
    }
    return VAEK_OK;
}

int check_hvp_buffers(const char* who, int32_t n, int64_t P, int32_t nvec, const double* v, int64_t v_stride, const double* hv, int64_t hv_stride,
                      const double* grad, int64_t grad_stride, bool refuse_overlap) {
    if (nvec < 0 || nvec > kHvpMaxVectors) {
        set_error("%s: %d vectors, need 0 .. %d (vaek_elbo_hvp_max_vectors)", who, nvec, kHvpMaxVectors);
        return VAEK_ERR_INVALID;
    }
    if (nvec > 0) {                                                     // nvec = 0: v and hv may be NULL and are not touched
        if (int rc = check_doubles(who, "v", v, v_stride, nvec * P, true)) return rc;
        if (int rc = check_doubles(who, "hv", hv, hv_stride, nvec * P, false)) return rc;
        if (refuse_overlap && doubles_overlap(v, v_stride, nvec * P, hv, hv_stride, nvec * P, n)) {
            set_error("%s: v and hv overlap: a direction is read by launches that follow the store of an earlier product", who);
            return VAEK_ERR_INVALID;
        }
    }
    if (grad)
        if (int rc = check_doubles(who, "grad", grad, grad_stride, P, false)) return rc;
    return VAEK_OK;
}

int check_lanczos_buffers(const char* who, int64_t P, int32_t steps, const double* v0, int64_t v0_stride, const double* basis, int64_t basis_stride) {
    if (steps < 1 || steps > kLanczosMaxSteps) {
        set_error("%s: %d steps, need 1 .. %d (vaek_elbo_hessian_max_steps)", who, steps, kLanczosMaxSteps);
        return VAEK_ERR_INVALID;
    }
    if (int rc = check_doubles(who, "v0", v0, v0_stride, P, true)) return rc;
    return check_doubles(who, "basis", basis, basis_stride, steps * P, false);
}

// ---- the training entry points (the order is in eval_check.h) -------------------------------------------------------------------------
int check_train_state(const char* who, const vaek_ctx* ctx, const float* params, const float* grads, const float* m, const float* v,
                      const int32_t* step_dev, int32_t n_steps, bool moments) {
    if (!ctx) { set_error("%s: null context", who); return VAEK_ERR_INVALID; }
    if (int rc = moments ? check_given(who, "params", params, "grads", grads, "m", m, "v", v, "step_dev", step_dev)
                         : check_given(who, "params", params, "grads", grads, "step_dev", step_dev)) return rc;
    if (n_steps < 0) { set_error("%s: n_steps %d < 0", who, n_steps); return VAEK_ERR_INVALID; }
    return VAEK_OK;
}

int check_replicas(const char* who, const vaek_ctx* ctx, const float* params, const float* grads, const float* m, const float* v,
                   const int32_t* step_dev, int32_t n_steps, const vaek_replicas* rep, const vaek_trajectory* traj, const ReplicaRules& r) {
    if (!rep) { set_error("%s: null description", who); return VAEK_ERR_INVALID; }
    if (int rc = check_struct_size(who, "vaek_replicas", rep->struct_size, sizeof(vaek_replicas))) return rc;
    if (traj)
        if (int rc = check_struct_size(who, "vaek_trajectory", traj->struct_size, sizeof(vaek_trajectory))) return rc;
    if (int rc = check_train_state(who, ctx, params, grads, m, v, step_dev, n_steps)) return rc;
    if (!r.covered) { set_error("%s: %s", who, r.needs); return VAEK_ERR_INVALID; }
    if (int rc = check_replica_count(who, rep->n, r.cap, r.cap_query)) return rc;
    // (stride4: every replica's parameters then have the base pointer's 16-byte alignment and take the load form a solo call would)
    if (rep->state_stride < ctx->P || (r.stride4 && rep->state_stride % 4 != 0)) {
        set_error("%s: state_stride %lld: need >= P = %lld (vaek_param_count)%s", who, (long long)rep->state_stride, (long long)ctx->P,
                  r.stride4 ? " and a multiple of 4" : "");
        return VAEK_ERR_INVALID;
    }
    if (rep->grads_stride < ctx->P + kExtra) {
        set_error("%s: grads_stride %lld < grad_len = %lld (vaek_grad_len)", who, (long long)rep->grads_stride, (long long)(ctx->P + kExtra));
        return VAEK_ERR_INVALID;
    }
    if (r.reads_seeds && !rep->seeds) { set_error("%s: seeds is NULL", who); return VAEK_ERR_INVALID; }
    if (rep->a_stride < 0) { set_error("%s: a_stride %lld < 0", who, (long long)rep->a_stride); return VAEK_ERR_INVALID; }
    if (rep->loss_hist && rep->loss_hist_cap < 1) {
        set_error("%s: loss_hist given with loss_hist_cap %lld < 1", who, (long long)rep->loss_hist_cap);
        return VAEK_ERR_INVALID;
    }
    return VAEK_OK;
}

int check_train_draw(const char* who, const vaek_ctx* ctx, int32_t kind, const float* A, int32_t dd, int32_t did, int32_t pad, float var_added,
                     int64_t row0, uint64_t seed, const int32_t* step_dev, uint32_t tag, BatchArgs* gen) {
    if (int rc = check_dataset_draw(who, ctx, kind, A, dd, did, pad, 0, tag, true)) return rc;
    *gen = BatchArgs{};
    fill_draw_args(gen, ctx, ctx->B, kind, A, dd, did, pad, var_added, tag, row0, seed, step_dev);
    return VAEK_OK;
}

}  // namespace vaek
