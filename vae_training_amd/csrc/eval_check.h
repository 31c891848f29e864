// The host-side checks of the thirteen vaek_*_replicas evaluation entry points, once (eval_check.hip; no kernels).  An entry point copies
// its description into an EvalDesc (describe), states what it adds in an EvalRules and calls check_eval; its own refusals (samples,
// columns, rank_tol) follow in its unit, those of the six Hessian entry points through the helpers below: 13. samples and columns (the
// four sampled calls), 14. the samples' source: xi_stride, else z_seeds / z_steps (the same four), 15. nvec, v, hv, their overlap (the
// sampled calls only), grad -- or steps, v0, basis.  check_eval refuses, in this order and with the first that fails:
//    1. a NULL description                          7. a NULL seeds / steps / sample_eps array the mode needs, a NULL out
//    2. a struct_size of another header             8. state_stride < P, out_stride below the record(s)
//    3. a NULL context or params                    9. an out that is not 8-byte aligned, where the records are doubles
//    4. a context the entry does not cover         10. the rows source: explicit rows' stride, else the dataset draw with x_tag
//    5. n outside 1 .. the replica cap             11. z_tag
//    6. rows outside the entry's range             12. a NULL or misaligned workspace
// Every message starts with the entry point's name and gives the field, its value, the bound and the query function that returns it.
#pragma once
#include "vaek_internal.h"

namespace vaek {

constexpr int kLogLikMaxRows = 4096;         // rows per call and ...
constexpr int kLogLikMaxSamples = 1024;      // ... samples per row: they bound one launch on a shared machine -- caps, not tuned values

// the dataset arguments of an in-kernel draw under tag x_tag, as `who` refuses them: a_stride, kind, A, dd / did / pad, dimension, tag
// (empty_did: a linear_gaussian dataset of did < 1 latent dimensions passes, as it always has in the training calls)
int check_dataset_draw(const char* who, const vaek_ctx* ctx, int32_t kind, const float* A, int32_t dd, int32_t did, int32_t pad,
                       int64_t a_stride, uint32_t x_tag, bool empty_did = false);
// ... and the BatchArgs of that draw: kind, A, dd, did, pad, noise_std, tag, rows, D, L, and the stream a training kernel draws from
// (row0, seed, step_dev; an evaluation kernel puts in its own); the pointers are the kernel's
void fill_draw_args(BatchArgs* g, const vaek_ctx* ctx, int rows, int32_t kind, const float* A, int32_t dd, int32_t did, int32_t pad,
                    float var_added, uint32_t x_tag, int64_t row0 = 0, uint64_t seed = 0, const int32_t* step_dev = nullptr);

// Hidden: the library's dynamic symbol list gains nothing.  (The two above were exported before this block existed, as every vaek::
// function is -- the library is built without -fvisibility=hidden -- and stay so.)
#pragma GCC visibility push(hidden)

enum class Need : uint8_t { ABSENT, DRAWING, ALWAYS };      // a field the description lacks / reads in drawing mode only / always reads

// The normalised head of a description.  `given` false: the caller passed NULL; a struct_size that differs from `want` leaves
// everything behind it unread (another header's struct may end earlier).
struct EvalDesc {
    const char* name; bool given; int32_t struct_size; size_t want;
    int32_t n, rows; int64_t state_stride;
    const uint64_t* x_seeds; const uint32_t* x_steps; Need x_need;
    const uint64_t* z_seeds; const uint32_t* z_steps; Need z_need;
    const float* sample_eps; Need eps_need;
    int64_t a_stride;
    const char* rows_name; const float* rows_ptr; int64_t rows_stride; char rows_dim;      // explicit rows: "x" of width 'D', "z" of 'L'; none: NULL
    const void* out; int64_t out_stride; bool out_doubles;
    bool explicit_rows() const { return rows_ptr != nullptr; }
};
EvalDesc describe(const vaek_stats_event* d);
EvalDesc describe(const vaek_log_likelihood* d);
EvalDesc describe(const vaek_spectrum_event* d);
EvalDesc describe(const vaek_exact_log_likelihood* d);
EvalDesc describe(const vaek_elbo_hvp* d);
EvalDesc describe(const vaek_elbo_hessian* d);
EvalDesc describe(const vaek_sampled_elbo_hvp* d);
EvalDesc describe(const vaek_sampled_elbo_hessian* d);
EvalDesc describe(const vaek_decoder_jacobian* d);

// What an entry point adds to the list.  A `_query` is the name of the function a message points to.
struct EvalRules {
    bool covered; const char* needs;                                 // the entry's predicate and the sentence for when it fails
    int rows_min; int rows_cap; const char* rows_query;
    int records; int64_t record_len; const char* record_query;      // out_stride >= records * record_len
    bool draws; int32_t kind; const float* A; int32_t dd, did, pad; uint32_t x_tag;      // a dataset draw takes part (drawing mode)
    bool has_z_tag; uint32_t z_tag;
    const void* workspace; int ws_align; const char* ws_query;      // ws_align 0: the call has no workspace
};
int check_eval(const char* who, const vaek_ctx* ctx, const float* params, const EvalDesc& d, const EvalRules& r);

// the BatchArgs of the rows and the kernel's a_stride: explicit rows draw nothing (the sphere's kind, which has no matrix, and
// *a_stride_out left alone), else a_stride and the real draw
void fill_rows_source(BatchArgs* gen, long long* a_stride_out, const vaek_ctx* ctx, int rows, bool explicit_rows, int32_t kind, const float* A,
                      int32_t dd, int32_t did, int32_t pad, float var_added, uint32_t x_tag, int64_t a_stride);

// One range check per counted quantity, for a call and for its workspace query alike
int check_replica_count(const char* who, int32_t n, int cap = resident_max_replicas(), const char* cap_query = "vaek_train_loop_max_replicas");
int check_row_count(const char* who, int32_t rows, int rows_min, int rows_cap, const char* rows_query);
int check_sample_count(const char* who, int32_t samples);                                                      // 1 .. kLogLikMaxSamples
// n * rows * per_row columns (`unit`: what per_row counts) against `cap`
int check_column_count(const char* who, int32_t n, int32_t rows, int32_t per_row, const char* unit, int cap, const char* cap_query);

int check_struct_size(const char* who, const char* name, int32_t got, size_t want);      // a descriptor `name` of another header's size
int check_x_stride(const char* who, const vaek_ctx* ctx, int64_t x_stride, int32_t rows); // explicit rows: 0 (shared) or >= rows * D
int check_tag(const char* who, uint32_t tag);                                             // >= 2^30
int check_aligned8(const char* who, const char* what, uintptr_t addrs);                   // `addrs`: the outputs `what` names, ORed

// ---- 13 .. 15: what the six Hessian entry points check behind check_eval ---------------------------------------------------------------
// a buffer `what` of `len` doubles per replica at `stride`: NULL, alignment, stride (shared_ok: 0 means one buffer for all replicas)
int check_doubles(const char* who, const char* what, const void* ptr, int64_t stride, int64_t len, bool shared_ok);
// the samples of a sampled call and where they come from: explicit xi, or (xi == NULL) drawn from z_seeds / z_steps
struct SampleSource { int32_t samples; const uint64_t* z_seeds; const uint32_t* z_steps; const float* xi; int64_t xi_stride; };
// read from a vaek_sampled_elbo_hvp / vaek_sampled_elbo_hessian, or all zero where check_eval is going to refuse the description unread
template <class T>
SampleSource sample_source(const EvalDesc& d, const T* s) {
    const bool read = d.given && d.struct_size == (int32_t)d.want;
    return read ? SampleSource{s->samples, s->z_seeds, s->z_steps, s->xi, s->xi_stride} : SampleSource{};
}
// 13: samples, rows * samples against the unit's per-replica cap 2^cap_log2, n * rows * samples against its per-call cap; for a call
// and for its workspace query alike
int check_sampled_columns(const char* who, int32_t n, int32_t rows, int32_t samples, int cap_log2, int call_cap, const char* call_cap_query);
// 14: xi_stride where xi is given, else z_seeds / z_steps
int check_sample_source(const char* who, const SampleSource& x, int32_t rows, int L);
// 15, an HVP call (hp: vaek_elbo_hvp or vaek_sampled_elbo_hvp): nvec, then v, hv and, where refuse_overlap, their overlap (nvec > 0),
// then grad where given
int check_hvp_buffers(const char* who, int32_t n, int64_t P, int32_t nvec, const double* v, int64_t v_stride, const double* hv, int64_t hv_stride,
                      const double* grad, int64_t grad_stride, bool refuse_overlap);
template <class T>
int check_hvp_buffers(const char* who, const T* hp, int64_t P, bool refuse_overlap) {
    return check_hvp_buffers(who, hp->n, P, hp->nvec, hp->v, hp->v_stride, hp->hv, hp->hv_stride, hp->grad, hp->grad_stride, refuse_overlap);
}
// 15, a Lanczos call (hs: vaek_elbo_hessian or vaek_sampled_elbo_hessian): steps, then v0, then basis
int check_lanczos_buffers(const char* who, int64_t P, int32_t steps, const double* v0, int64_t v0_stride, const double* basis, int64_t basis_stride);
template <class T>
int check_lanczos_buffers(const char* who, const T* hs, int64_t P) {
    return check_lanczos_buffers(who, P, hs->steps, hs->v0, hs->v0_stride, hs->basis, hs->basis_stride);
}

// ---- the training entry points of api.hip ----------------------------------------------------------------------------------------------
// The seven whose batches a generator feeds (vaek_train_step_gen, vaek_train_steps_gen, vaek_train_loop_gen[_traj],
// vaek_train_loop_gen_replicas[_traj], vaek_train_step_gen_replicas) refuse in this order, with the first that fails:
//    1. a NULL vaek_replicas                                      6. the vaek_replicas fields: n, state_stride, grads_stride, seeds,
//    2. its struct_size, then a given vaek_trajectory's              a_stride, loss_hist_cap -- a message each
//    3. a NULL context                                            7. the vaek_trajectory fields
//    4. a NULL params / grads / m / v / step_dev, n_steps < 0     8. the entry's own pointers and aliasing rules
//    5. a context the entry does not cover                        9. the dataset draw
//                                                                10. the workspace
// An entry without a description starts at 3; the four calls that are handed their batches run 3 and 4, then their own checks.
// the first NULL of (name, pointer) pairs, named
inline int check_given(const char*) { return VAEK_OK; }
template <class... Rest>
int check_given(const char* who, const char* name, const void* p, Rest... rest) {
    if (!p) { set_error("%s: %s is NULL", who, name); return VAEK_ERR_INVALID; }
    return check_given(who, rest...);
}
// 3 and 4 (moments false: a call without m and v)
int check_train_state(const char* who, const vaek_ctx* ctx, const float* params, const float* grads, const float* m, const float* v,
                      const int32_t* step_dev, int32_t n_steps = 0, bool moments = true);
// 1 .. 6 of the two replica calls; a `_query` is the name of the function a message points to
struct ReplicaRules { bool covered; const char* needs; int cap; const char* cap_query; bool stride4, reads_seeds; };
int check_replicas(const char* who, const vaek_ctx* ctx, const float* params, const float* grads, const float* m, const float* v,
                   const int32_t* step_dev, int32_t n_steps, const vaek_replicas* rep, const vaek_trajectory* traj, const ReplicaRules& r);
// 9 for the calls whose kernel draws its own batches of ctx->B rows: the dataset arguments checked and made into the kernel's BatchArgs
int check_train_draw(const char* who, const vaek_ctx* ctx, int32_t kind, const float* A, int32_t dd, int32_t did, int32_t pad, float var_added,
                     int64_t row0, uint64_t seed, const int32_t* step_dev, uint32_t tag, BatchArgs* gen);
#pragma GCC visibility pop

}  // namespace vaek
