/*
 * vaek.h -- C ABI of the MI355X-native ELBO train-step library (libvaek.so).
 *
 * The reference (virajmehta/vae-training) is pure Python on JAX/Flax and has no FFI; the
 * "native kernels" it runs are the XLA programs behind the calls cited on each entry point
 * below (paths relative to /root/reference).  This header is therefore the boundary a
 * maintainer would bind from Python with ctypes to replace
 *     VAE.train_step   networks.py:87-101   (forward + ELBO + backward + Adam, one jitted fn)
 *     VAE.loss         networks.py:103-113  (forward + ELBO, eval twin)
 *     VAE.apply        networks.py:61-84    (model(batch, z1, z2[, sampling=True]))
 *
 * Conventions
 *   - every function returns 0 on success, a negative vaek_status otherwise; it never throws
 *     and never aborts.  vaek_last_error() returns a thread-local message for the last failure.
 *   - every device buffer is owned by the caller (PyTorch-ROCm tensors on the Python side);
 *     the library receives raw device pointers and a hipStream_t (passed as void*), launches
 *     asynchronously on that stream and never synchronises or allocates after ctx_create
 *     (vaek_comm_* excepted: it maps peer memory once at init).
 *   - matrices are row-major; Dense kernels are [in, out] exactly as flax.nn.Dense stores
 *     them; all floating-point buffers are float32 unless a name says bf16.
 *   - parameters, gradients and both Adam moments each live in ONE flat float32 buffer with
 *     the fixed leaf order
 *         Encoder/FC0/kernel, Encoder/FC0/bias, ..., Decoder/FC0/kernel, ...,
 *         [SigDecoder/FC0/kernel, ...,]  epsilon_p (L),  [epsilon (1)]
 *     (names as in networks.py:67-78 and vae.py:73-80).  The gradient buffer has
 *     vaek_grad_len() = P + 4 floats: [P] = loss, [P+1] = mean Dkl, [P+2] = mean mse, [P+3] = 0,
 *     so that a data-parallel sum of the buffer also yields the global loss.
 *   - one host thread per context; one process per GPU for data parallelism.
 */
#ifndef VAEK_H
#define VAEK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VAEK_VERSION 100 /* 0.1.0 */
#define VAEK_MAX_HIDDEN 8

typedef enum vaek_status {
    VAEK_OK = 0,
    VAEK_ERR_INVALID = -1,   /* bad argument / unsupported configuration */
    VAEK_ERR_HIP = -2,       /* a HIP runtime call failed                 */
    VAEK_ERR_NO_DEVICE = -3, /* no usable gfx950 device                   */
    VAEK_ERR_WORKSPACE = -4, /* workspace too small / misaligned          */
    VAEK_ERR_COMM = -5       /* peer-to-peer communicator failure         */
} vaek_status;

/* Activation codes of vaek_dense_fwd / vaek_dense_bwd_dx. */
enum { VAEK_ACT_NONE = 0, VAEK_ACT_RELU = 1 };

/* Compute dtype of the Dense GEMMs (ELBO, reductions and Adam are always float32). */
enum { VAEK_F32 = 0, VAEK_BF16 = 1 };

/* What VAE.partial binds at vae.py:57-59 plus the batch geometry. */
typedef struct vaek_config {
    int32_t struct_size;                  /* = sizeof(vaek_config), ABI guard                      */
    int32_t batch;                        /* rows handed to this rank per step (B_local)           */
    int32_t data_dim;                     /* D = prod(dataset.shape), vae.py:51                    */
    int32_t latent_dim;                   /* L, vae.py:50                                          */
    int32_t n_enc_hidden;                 /* encoder_layer_sizes without the appended L, vae.py:53 */
    int32_t enc_hidden[VAEK_MAX_HIDDEN];
    int32_t n_dec_hidden;                 /* layer_sizes without the appended D, vae.py:54         */
    int32_t dec_hidden[VAEK_MAX_HIDDEN];
    int32_t sigmoid_decoder;              /* dataset_name == "sigmoid": SigDecoder + Decoder, networks.py:75-78 */
    int32_t tunable_eps;                  /* -tdv: epsilon is a (1,) parameter times eps_cli, networks.py:70-71 */
    float   eps_cli;                      /* -e/--epsilon, run.py:31                               */
    int32_t dtype;                        /* VAEK_F32 | VAEK_BF16                                  */
    int32_t device;                       /* HIP device ordinal                                    */
    int32_t world;                        /* data-parallel ranks (1 = single GPU)                  */
    int32_t rank;
    int64_t global_batch;                 /* divisor of loss.mean() (networks.py:98); 0 -> batch*world */
    int32_t force_generic;                /* 1: never pick the fused small-model kernels (tests)   */
    int32_t reserved[7];
} vaek_config;

typedef struct vaek_ctx vaek_ctx;

/* ---- library ---------------------------------------------------------------------------- */
int vaek_version(void);
const char* vaek_last_error(void);

/* ---- context: replaces VAE.partial(...) + init_by_shape shape inference, vae.py:57-60 ---- */
int vaek_ctx_create(const vaek_config* cfg, vaek_ctx** out);
int vaek_ctx_destroy(vaek_ctx* ctx);
/* P = number of trainable floats; grad_len = P + 4 (see conventions). */
int vaek_param_count(const vaek_ctx* ctx, int64_t* P);
int vaek_grad_len(const vaek_ctx* ctx, int64_t* n);
/* Leaf table of the flat layout: n_leaves, then per leaf its offset and (rows, cols);
 * a bias / epsilon_p / epsilon leaf has rows == 1.  name buffers are NUL-terminated. */
int vaek_leaf_count(const vaek_ctx* ctx, int32_t* n_leaves);
int vaek_leaf_info(const vaek_ctx* ctx, int32_t leaf, char* name, int32_t name_cap,
                   int64_t* offset, int32_t* rows, int32_t* cols);
/* Bytes of caller-owned scratch (256-byte aligned) every entry point taking `workspace` needs. */
int vaek_workspace_bytes(const vaek_ctx* ctx, size_t* bytes);
/* 1 if the fused small-model path is used for train_step/loss_eval, 0 for layer-by-layer. */
int vaek_uses_fused_path(const vaek_ctx* ctx, int32_t* fused);
/* Which form vaek_train_step takes for this context, chosen once at creation, NUL-terminated into name[cap]:
 * "linear" (fused linear VAE, D, L <= 32), "mlp1" (one hidden layer), "mlp3" (three hidden layers of 64 .. 256 units both
 * ways, D, L <= 32, float32, one decoder, batch <= 128), "linear_wide" (layer by layer with the fused wide linear decoder)
 * or "layers" (layer by layer).  The first three are whole-network paths: vaek_uses_fused_path reports 1 for them. */
int vaek_train_step_path(const vaek_ctx* ctx, char* name, int32_t cap);

/* ---- building blocks (also used by the layer-by-layer path of vaek_train_step) ----------- */
/* flax.nn.Dense + relu, networks.py:34-39: y[rows,n_out] = act(x[rows,n_in] @ w[n_in,n_out] + b). */
int vaek_dense_fwd(vaek_ctx* ctx, const float* x, const float* w, const float* b, float* y,
                   int32_t rows, int32_t n_in, int32_t n_out, int32_t act, void* stream);
/* dx[rows,n_in] = (dy[rows,n_out] @ w^T) * (act == RELU ? x_post > 0 : 1); x_post is the
 * layer's INPUT as produced by the previous layer's relu (may be NULL for ACT_NONE).
 * accumulate != 0 adds into dx instead of overwriting (the two decoders of networks.py:76-78). */
int vaek_dense_bwd_dx(vaek_ctx* ctx, const float* dy, const float* w, const float* x_post, float* dx,
                      int32_t rows, int32_t n_in, int32_t n_out, int32_t act, int32_t accumulate, void* stream);
/* dwb[(n_in+1), n_out]: rows 0..n_in-1 = x^T @ dy (kernel gradient), row n_in = column sums of
 * dy (bias gradient) -- i.e. exactly the [kernel | bias] slice of the flat gradient buffer.
 * Deterministic (split over the batch into workspace slabs, then summed in a fixed order). */
int vaek_dense_bwd_dw(vaek_ctx* ctx, const float* x, const float* dy, float* dwb,
                      int32_t rows, int32_t n_in, int32_t n_out, void* workspace, void* stream);
/* networks.py:94-98 on explicit tensors.  x_hat_lin = Decoder(samples) WITHOUT the z2 noise;
 * x_hat_sig = SigDecoder pre-sigmoid output or NULL.  Writes out4 = {loss, mean Dkl, mean mse,
 * dL/d eps} (means over `batch_total`), and if d_lin != NULL the gradients w.r.t. the two
 * decoder outputs (d_sig may alias x_hat_sig, d_lin may alias x_hat_lin). */
int vaek_elbo_fwd_bwd(vaek_ctx* ctx, const float* x, const float* x_hat_lin, const float* x_hat_sig,
                      const float* z2, const float* mu, const float* logvar_e, float eps,
                      float* d_lin, float* d_sig, float* out4, int32_t rows, int32_t data_dim,
                      int32_t latent_dim, int64_t batch_total, void* workspace, void* stream);
/* The same with eps = eps_param_dev[0] * eps_scale read ON THE DEVICE (the tunable decoder variance of networks.py:70-71 is a
 * parameter: no host read, so a step built from the block entry points can be captured into a hipGraph). */
int vaek_elbo_fwd_bwd_dev(vaek_ctx* ctx, const float* x, const float* x_hat_lin, const float* x_hat_sig,
                          const float* z2, const float* mu, const float* logvar_e, const float* eps_param_dev, float eps_scale,
                          float* d_lin, float* d_sig, float* out4, int32_t rows, int32_t data_dim,
                          int32_t latent_dim, int64_t batch_total, void* workspace, void* stream);
/* flax.optim.Adam.apply_gradient, networks.py:100 (beta1 .9, beta2 .999, eps 1e-8).
 * `step_dev` (device int32, may be NULL) holds t of THIS update (1-based) when non-NULL,
 * otherwise `step` is used.  grad_scale multiplies the gradient first (1/world for means). */
int vaek_adam_step(vaek_ctx* ctx, float* params, const float* grads, float* m, float* v, int64_t n,
                   float lr, int32_t step, const int32_t* step_dev, float grad_scale, void* stream);

/* ---- the hot path ------------------------------------------------------------------------ */
/* VAE.train_step, networks.py:87-101, in place: reads params, x[B,D], z1[B,L], z2[B,D];
 * writes grads (vaek_grad_len floats; summed over ranks when the communicator is initialised),
 * updates params/m/v, increments *step_dev (device int32 Adam step counter), leaves the loss
 * in grads[P] (device; the reference keeps it un-synced too, vae.py:130).
 * Launches: linear VAEs with D, L <= 32 (the metric) run two kernels -- forward/backward/partial sums, then
 * reduction + Adam -- or ONE when the batch fits a workgroup (<= 256 rows, single GPU); one-hidden-layer MLPs and
 * three-hidden-layer MLPs at small batch (vaek_train_step_path "mlp1" / "mlp3") run two as well; any other MLP runs layer
 * by layer.  Asynchronous on `stream`, capturable into a hipGraph (no host-side state per step). */
int vaek_train_step(vaek_ctx* ctx, float* params, float* grads, float* m, float* v, int32_t* step_dev,
                    const float* x, const float* z1, const float* z2, float lr,
                    void* workspace, void* stream);
/* The two halves of vaek_train_step, for callers that all-reduce grads themselves (RCCL via
 * torch.distributed): grads_only leaves the LOCAL gradient sums (already divided by
 * global_batch) in grads and does not touch params; apply runs Adam on grads. */
int vaek_train_step_grads_only(vaek_ctx* ctx, const float* params, float* grads, int32_t* step_dev,
                               const float* x, const float* z1, const float* z2,
                               void* workspace, void* stream);
int vaek_train_step_apply(vaek_ctx* ctx, float* params, const float* grads, float* m, float* v,
                          const int32_t* step_dev, float lr, void* stream);
/* Bucketed variant for overlapping the data-parallel exchange with the rest of the backward pass
 * (layer-by-layer path): the flat gradient is final bucket by bucket, in backward order (decoder's last
 * layer first, encoder's first layer last, then the tail = epsilon_p, epsilon, loss slots).  Bucket i
 * covers grads[offset, offset + count) (vaek_bucket_info); ready_events[i] is a caller-owned hipEvent_t
 * (passed as void*) that the library records on `stream` the moment bucket i is complete, so a
 * communication stream can wait on it and all-reduce that slice while earlier layers are still in
 * their dW / dX GEMMs.  The fused small-model path has a single bucket. */
int vaek_bucket_count(const vaek_ctx* ctx, int32_t* n);
int vaek_bucket_info(const vaek_ctx* ctx, int32_t i, int64_t* offset, int64_t* count);
int vaek_train_step_grads_bucketed(vaek_ctx* ctx, const float* params, float* grads, int32_t* step_dev,
                                   const float* x, const float* z1, const float* z2, void* const* ready_events,
                                   void* workspace, void* stream);
/* VAE.loss, networks.py:103-113: out4 = {loss, mean Dkl, mean mse, eps}. */
int vaek_loss_eval(vaek_ctx* ctx, const float* params, const float* x, const float* z1, const float* z2,
                   float* out4, void* workspace, void* stream);
/* VAE.apply, networks.py:61-84.  sampling != 0: mu = 0, logvar_e = 0, samples = z1 and `eps`
 * is used as given (vae.py:199); otherwise x is encoded and eps comes from the parameters
 * (`eps` ignored).  x_hat[rows,D] includes the z2 noise; mu_out[rows,L] may be NULL. */
int vaek_forward(vaek_ctx* ctx, const float* params, const float* x, const float* z1, const float* z2,
                 int32_t sampling, float eps, float* x_hat, float* mu_out, int32_t rows,
                 void* workspace, void* stream);

/* ---- data-parallel exchange over xGMI (one-shot peer-to-peer all-reduce of the flat grads) -- */
/* The reference is single-device; this is the build's data-parallel addition.
 * Every rank calls vaek_comm_create (allocates ITS uncached exchange buffer -- the one allocation the
 * library makes after ctx_create -- and exports a 64-byte HIP IPC handle), the handles are
 * exchanged out of band (torch.distributed all_gather), and vaek_comm_init maps all peers.  After
 * that vaek_train_step sums gradients over ranks INSIDE its finalize kernel (tagged 8-byte granules
 * stored straight into every peer's buffer over xGMI; bounded spins).  Without a communicator and
 * world > 1 use vaek_train_step_grads_only + an RCCL all-reduce + vaek_train_step_apply. */
int vaek_comm_buffer_bytes(const vaek_ctx* ctx, size_t* bytes);
int vaek_comm_create(vaek_ctx* ctx, uint8_t handle_out[64]);
int vaek_comm_init(vaek_ctx* ctx, const uint8_t* all_handles /* world x 64 */);
int vaek_comm_destroy(vaek_ctx* ctx);
/* Stand-alone sum all-reduce of n floats in place through the communicator (n <= grad_len). */
int vaek_comm_allreduce(vaek_ctx* ctx, float* buf, int64_t n, void* stream);
/* Synchronous: *timed_out = 1 if any exchange on this rank ever gave up waiting for a peer. */
int vaek_comm_status(vaek_ctx* ctx, int32_t* timed_out);

/* ---- inputs of the hot path, generated on the device ---------------------- */
/* One Philox4x32-10 kernel replacing dataset.get_batch (datasets.py:75-84 sphere = kind 2, :183-195
 * linear_gaussian = kind 0 with A[dd][did], :240-249 sigmoid = kind 1 with A[dd]) and the latent draw
 * of model.py:225-228 split as vae.py:127-128 does (z1[rows,L], z2[rows,D]).  Row i of the call draws
 * from counter (row0 + i, block, step, tag) under key `seed`: reproducible, shardable by rows, and
 * graph-replayable when `step_dev` (the device Adam step counter) is given instead of step_host.
 * x may be NULL (latents only); z1 and z2 may both be NULL (dataset batch only, any D).  dd, did <= 16;
 * tag < 2^30. */
int vaek_make_batch(vaek_ctx* ctx, int32_t kind, const float* A, int32_t dd, int32_t did, int32_t pad, float var_added,
                    float* x, float* z1, float* z2, int32_t rows, int64_t row0, uint64_t seed,
                    const int32_t* step_dev, uint32_t step_host, uint32_t tag, void* stream);
/* The same draw for a loop that generates batch n+1 while step n trains (trainer.GraphLoop): the step is
 * counter[which] and the kernel ITSELF stores counter[which ^ 1] = step + 1 for the next launch, so a captured
 * launch needs no host argument and does not touch the Adam step counter a concurrently running train step is
 * incrementing.  The caller alternates `which` (0, 1, 0, ...) from launch to launch -- with two batch buffers that
 * is the buffer index -- and initialises counter[first which] to the first step.  Bit-identical to
 * vaek_make_batch(step_host = counter[which]). */
int vaek_make_batch_next(vaek_ctx* ctx, int32_t kind, const float* A, int32_t dd, int32_t did, int32_t pad, float var_added,
                         float* x, float* z1, float* z2, int32_t rows, int64_t row0, uint64_t seed,
                         int32_t* counter /* device int32[2] */, int32_t which, uint32_t tag, void* stream);
/* vaek_train_step on (x, z1, z2) AND vaek_make_batch_next into (x_next, z1_next, z2_next) -- the loop body of
 * model.py:221-222 with the draw for step n+1 taken off the critical path.  On the fused path the generator's work
 * items ride in the finalize launch (which by itself occupies 9 of 256 CUs): still two launches per step, one
 * stream, no cross-queue dependency; a batch that fits one workgroup (<= 256 rows, single GPU) is ONE launch, the draw on
 * its workgroups 1.. .  Elsewhere it is the two calls back to back.  Results are bit-identical to the
 * separate calls.  The next batch has ctx.batch rows and must not alias the current one. */
int vaek_train_step_gen(vaek_ctx* ctx, float* params, float* grads, float* m, float* v, int32_t* step_dev, const float* x,
                        const float* z1, const float* z2, float lr, void* workspace, int32_t kind, const float* A, int32_t dd,
                        int32_t did, int32_t pad, float var_added, float* x_next, float* z1_next, float* z2_next, int64_t row0,
                        uint64_t seed, int32_t* counter, int32_t which, uint32_t tag, void* stream);
/* N consecutive VAE.train_step's (the loop body of model.py:221-222 -> networks.py:87-101, N times) on N batches already
 * resident in HBM: xs / z1s / z2s are HOST arrays of n_steps device pointers (batch i = xs[i][B,D], z1s[i][B,L], z2s[i][B,D]).
 * On return (in stream order) params / m / v / *step_dev / grads are what n_steps calls of vaek_train_step on those batches
 * leave, to float32 summation-order tolerance -- NOT bitwise: the steps are evaluated through the batch's second-moment
 * matrix (csrc/linear_moments.hip), which takes the parameters off the streaming pass, so that the pass over batch n + 2,
 * the cross-workgroup sum of batch n + 1 and the Adam update of batch n run side by side -- as resident workgroup roles of one
 * persistent launch per 64 steps (arrival counters, bounded waits: vaek_train_steps_status), or where that form does not apply as
 * n_steps + 2 launches ordered by the stream alone.  The launches of one call are chained: each streams its own 64 batches, but
 * leaves its last batch to the next launch's reducers and its last four to the next launch's updater, so a later launch reduces and
 * updates from its first microsecond on and its roles end together; the call's last launch finishes every step, and nothing is
 * carried from one call to the next.  For that the workspace holds 68 batch slots (partial images, moment matrix, arrival
 * counters; batch n of a call uses slot n mod 68): 68 x (tiles x 6 or 10 KB) -- 95.3 MB at batch 65 536, D = 12, L = 20.
 * The persistent form covers L <= 32 with L + 2 D + 1 <= 48 and D <= 16, or with
 * 49 <= L + 2 D + 1 <= 64 (four 16-feature blocks); data parallelism and vaek_train_steps_gen need it.  Capturable into a hipGraph.  A context recognises a workspace whose arrival
 * counters it has initialised by the workspace's address.  Linear encoder / decoder, one decoder, float32, L + 2 D + 1 <= 64,
 * and, with world > 1, an initialised P2P communicator (vaek_comm_create / vaek_comm_init: the moment matrix is additive over the
 * ranks' shards and is exchanged inside the launch; every rank must make the same calls, and the Adam step counter must not restart
 * while the communicator lives): vaek_supports_train_steps says whether this context qualifies; others return VAEK_ERR_INVALID. */
int vaek_supports_train_steps(const vaek_ctx* ctx, int32_t* yes);
int vaek_train_steps(vaek_ctx* ctx, float* params, float* grads, float* m, float* v, int32_t* step_dev,
                     const float* const* xs, const float* const* z1s, const float* const* z2s, int32_t n_steps, float lr,
                     void* workspace, void* stream);
/* Synchronous (reads one word back): *gave_up != 0 if a bounded in-launch wait of vaek_train_steps' / vaek_train_steps_gen's persistent
 * form has expired in ANY launch since the last call of this function (the results since then are invalid).  The word is STICKY on
 * the device -- no launch clears it, and while it is set every wait of every later launch returns at once (the grid drains) -- and
 * this call is read-and-clear.  It says which wait came first: 0x80000000 | role << 28 (1 the updater, 2 a reducer, 3 a reducer
 * waiting for a peer rank's moments) | batch index within the launch << 16 | the arrival count it last saw. */
int vaek_train_steps_status(vaek_ctx* ctx, void* workspace, int32_t* gave_up);
/* The same N train steps with the batches DRAWN inside the launch: step k of the call (the one that takes *step_dev from t to
 * t + 1) trains on the batch vaek_make_batch(kind, A, dd, did, pad, var_added, rows = ctx.batch, row0, seed, step = t, tag)
 * would write -- the same Philox4x32-10 counters, Box-Muller and dataset maps (csrc/rng_dev.h), bit for bit -- but the batch
 * never exists in HBM: the streamers of the persistent launch draw each tile straight into LDS between the products of an
 * earlier tile.  This is the loop body of the reference, model.py:221-222 (dataset.get_batch -> vae.py:123-130 sample_latent,
 * VAE.train_step), N times per launch.  kind: 0 linear_gaussian, 2 sphere (a linear VAE on the sigmoid dataset has two decoders:
 * not covered).  Data parallel: every rank passes its own row0 (global row indices).  Capturable into a hipGraph (the RNG step
 * is the device-resident Adam counter).  Shapes: those of the persistent form (vaek_train_steps).  vaek_supports_train_steps_gen
 * says whether this context / dataset kind qualifies;
 * status as vaek_train_steps. */
int vaek_supports_train_steps_gen(const vaek_ctx* ctx, int32_t kind, int32_t* yes);
/* The two halves of ONE step of vaek_train_steps' launch-per-step form, for data parallelism over a HOST collective (no P2P
 * communicator needed): the second-moment matrix of a linear VAE's batch is additive over the ranks' row shards -- the loss of
 * networks.py:97-98 is a batch mean -- so every rank calls vaek_train_steps_moments on its shard (x, z1, z2 of ctx.batch rows ->
 * M, a float64 image of vaek_train_steps_moment_len doubles), the caller sums M over the ranks (torch.distributed all_reduce:
 * RCCL / gloo; every rank receives the same bits), and vaek_train_steps_update turns the summed M into loss, gradients and the Adam
 * update of networks.py:99-101 with the GLOBAL batch as divisor (ctx.global_batch): replicas stay bitwise identical.  With world
 * == 1 the pair is one train step.  *len == 0: this context is not a linear VAE the moment form covers. */
int vaek_train_steps_moment_len(const vaek_ctx* ctx, int64_t* len);
int vaek_train_steps_moments(vaek_ctx* ctx, const float* x, const float* z1, const float* z2, double* M, void* workspace, void* stream);
int vaek_train_steps_update(vaek_ctx* ctx, float* params, float* grads, float* m, float* v, int32_t* step_dev, const double* M, float lr,
                            void* workspace, void* stream);
int vaek_train_steps_gen(vaek_ctx* ctx, float* params, float* grads, float* m, float* v, int32_t* step_dev, int32_t kind, const float* A,
                         int32_t dd, int32_t did, int32_t pad, float var_added, int64_t row0, uint64_t seed, uint32_t tag, int32_t n_steps,
                         float lr, void* workspace, void* stream);
/* N consecutive train steps of a SMALL-BATCH linear VAE as a plain loop inside ONE workgroup (csrc/linear_resident.hip) -- the
 * loop body of the reference, model.py:221-222, at its own batch size (run.py:14: 100 rows), for the linear VAEs the moment form
 * above does not cover: two decoders (the sigmoid dataset, sigmoid_vae_padding_expts.sh), a one-decoder model with
 * L + 2 D + 1 > 64, a batch too small for the moment form.  Arguments and meaning are those of vaek_train_steps_gen: step k of the
 * call takes *step_dev from t to t + 1 and trains on exactly the batch vaek_make_batch(kind, A, dd, did, pad, var_added,
 * rows = ctx.batch, row0, seed, step = t, tag) would write (the same Philox counters and csrc/rng_dev.h maps, bit for bit).  On
 * return, in stream order, params / m / v / *step_dev are what n_steps calls of vaek_train_step on those batches leave (float32
 * tolerance, as between any two of this library's paths), grads is the LAST step's gradient buffer (vaek_grad_len floats, loss slots
 * included) and the ring of vaek_set_loss_history holds every step's loss at (t - 1) % cap.  Parameters and both Adam moments are
 * read from HBM once per launch and written once, at its end; a launch runs at most vaek_train_loop_steps_per_launch() = 1024
 * steps (a cap that bounds one launch to milliseconds, not a tuned value) and a longer call is several launches on the stream, each
 * starting from memory alone.  One workgroup: no counters, no waits, hence no status to poll.  Asynchronous, allocates nothing,
 * capturable into a hipGraph (the RNG step is the device-resident Adam counter); nothing is carried from call to call except the
 * caller's buffers.
 * vaek_supports_train_loop_gen: float32, no hidden layers, one OR two decoders, D, L <= 32 (a matrix-core variant exists),
 * world == 1, 1 <= batch <= 256, force_generic == 0 -- decided once in vaek_ctx_create -- and kind 0, 1 or 2.  The call also needs
 * dd, did <= 16.  Everything else returns VAEK_ERR_INVALID.  WORKSPACE: where the kernel's LDS has no room for the batch next to
 * its operand image (large D and L with a large batch) the batch is staged in the workspace, so vaek_workspace_bytes of a
 * qualifying context may be up to 96 KB larger than before this entry point existed. */
int vaek_supports_train_loop_gen(const vaek_ctx* ctx, int32_t kind, int32_t* yes);
int vaek_train_loop_gen(vaek_ctx* ctx, float* params, float* grads, float* m, float* v, int32_t* step_dev, int32_t kind, const float* A,
                        int32_t dd, int32_t did, int32_t pad, float var_added, int64_t row0, uint64_t seed, uint32_t tag, int32_t n_steps,
                        float lr, void* workspace, void* stream);
int vaek_train_loop_steps_per_launch(void);
/* The same loop for N INDEPENDENT models of the context's shape in one launch: workgroup r trains replica r (a sweep over dataset
 * seeds, learning rates, initialisations -- the reference's experiment scripts are all sweeps -- where one vaek_train_loop_gen
 * launch keeps 1 of the MI355X's 256 CUs busy).  The loop has no cross-workgroup state, so the replica form adds no counter, no wait
 * and no atomic: nothing to poll.  Replica r owns
 *   params + r * state_stride, m + r * state_stride, v + r * state_stride   (vaek_param_count floats each; state_stride >= P),
 *   grads + r * grads_stride                                                (vaek_grad_len floats; grads_stride >= grad_len),
 *   step_dev[r], seeds[r], lrs[r] (lrs == NULL: the scalar `lr` for every replica),
 *   A + r * a_stride (a_stride == 0: one matrix shared by all; A may be NULL for kind 2),
 *   loss_hist + r * loss_hist_cap: the loss of Adam step t at [(t - 1) % loss_hist_cap] (loss_hist == NULL: no ring).
 * Every array is a caller-owned DEVICE buffer (seeds, lrs and A are only read); floats between two replicas where a stride exceeds
 * the length are not touched; strides need no alignment beyond a float's.  kind, dd, did, pad, var_added, row0, tag, n_steps and
 * the context (shape, batch, epsilon) are shared by the launch.
 * DEFINING PROPERTY: for every r, what the call leaves in replica r's params, m, v, grads, step_dev[r] and ring is BITWISE what
 * vaek_train_loop_gen leaves when called alone on those buffers with seed = seeds[r], lr = lrs[r], replica r's A and the same
 * shared arguments (the ring of vaek_set_loss_history standing in for replica r's): the same code on the same inputs.
 * The ring of vaek_set_loss_history is NOT written by this call.  Asynchronous on `stream`, allocates nothing, does not
 * synchronise, capturable into a hipGraph; more than vaek_train_loop_steps_per_launch() steps are several launches, each starting
 * from HBM alone.  Covers exactly the contexts and kinds vaek_supports_train_loop_gen accepts.
 * vaek_train_loop_max_replicas() = 1024: four rounds of 256 workgroups on 256 CUs -- a cap that bounds the length of one launch on
 * a shared machine, not a tuned value.  n above the CU count is legal: workgroups are independent, the extra ones queue.
 * WORKSPACE: the call's OWN buffer of vaek_train_loop_replicas_workspace_bytes(ctx, n) bytes, 16-byte aligned: n times the staged
 * batch where the kernel's LDS has no room for it, else 0 bytes and `workspace` may be NULL.  It is NOT the buffer of
 * vaek_workspace_bytes, which this entry point neither needs nor changes.
 * VAEK_ERR_INVALID (with a message): n < 1 or n > the cap, state_stride < P, grads_stride < grad_len, NULL seeds, a_stride < 0, a
 * ring with loss_hist_cap < 1, a missing or misaligned workspace where one is needed, dd or did > 16, kind outside 0 .. 2, an
 * unsupported context, a wrong struct_size.  n_steps == 0 returns VAEK_OK and touches nothing. */
typedef struct vaek_replicas {
    int32_t struct_size;                  /* = sizeof(vaek_replicas), ABI guard                    */
    int32_t n;                            /* replicas = workgroups of the launch                   */
    int64_t state_stride;                 /* floats between two replicas' params (and m, and v)    */
    int64_t grads_stride;                 /* floats between two replicas' grads                    */
    const uint64_t* seeds;                /* device [n]: RNG seed per replica                      */
    const float* lrs;                     /* device [n] or NULL: learning rate per replica         */
    int64_t a_stride;                     /* floats between two replicas' A; 0 = shared            */
    float* loss_hist;                     /* device [n][loss_hist_cap] or NULL                     */
    int64_t loss_hist_cap;
} vaek_replicas;
int vaek_train_loop_max_replicas(void);
int vaek_train_loop_replicas_workspace_bytes(const vaek_ctx* ctx, int32_t n, size_t* bytes);
int vaek_train_loop_gen_replicas(vaek_ctx* ctx, float* params, float* grads, float* m, float* v, int32_t* step_dev,
                                 const vaek_replicas* rep, int32_t kind, const float* A, int32_t dd, int32_t did, int32_t pad,
                                 float var_added, int64_t row0, uint32_t tag, int32_t n_steps, float lr, void* workspace, void* stream);
/* TRAJECTORY RING of the resident loop: parameter and gradient records written INSIDE the launch (csrc/linear_resident.hip).  The
 * resident loop keeps params, m and v on chip for up to 1024 steps and stores grads at a launch's last step only; a caller who
 * studies training dynamics (the reference's params_and_gradients list and its Correlation Ratio, vae.py:143-179, :203-209) had
 * to cut the loop to see the model.  With a vaek_trajectory the workgroup stores, at every Adam step t with t % every == 0 (t is
 * 1-based: the value *step_dev takes AFTER the step), one record of vaek_trajectory_record_len = 2 P + 4 floats, BEFORE that step's
 * Adam update:
 *   [0, P)         the parameters step t's gradient was evaluated at -- the state after t - 1 steps;
 *   [P, 2 P + 4)   the gradient buffer of step t exactly as `grads` would hold it if the call ended at step t (vaek_grad_len floats:
 *                  loss / mean Dkl / mean mse / 0 slots included).
 * SLOT RULE: the record of step t goes to buf (+ r * replica_stride for replica r) + ((t / every - 1) % cap) * record_stride.  The
 * slot depends on the global step alone, so placement is the same across the 1024-step launch boundary inside a call, across
 * calls, after a resume from a checkpoint (*step_dev != 0) and under graph replay (t comes from the device-resident counter).  A
 * ring of cap records keeps the last cap of them; slots no recorded step of this call maps to keep their contents; floats between
 * two records or two rings, where a stride exceeds the length, are not touched.  The ring is written with per-lane vector stores
 * and never read by the launch; no counter, no wait, no atomic is added.
 * vaek_train_loop_gen_traj / vaek_train_loop_gen_replicas_traj take the arguments of vaek_train_loop_gen /
 * vaek_train_loop_gen_replicas and a vaek_trajectory; traj == NULL is the plain call.  They cover exactly the contexts and kinds
 * vaek_supports_train_loop_gen accepts, with the same workspace rules; asynchronous, allocate nothing, do not synchronise,
 * capturable.  Profile labels linear_resident_traj / linear_resident_replicas_traj (the untraced launches keep theirs).
 * DEFINING PROPERTY (bitwise, from the same start state and arguments): (a) the traced call leaves in params, m, v, grads,
 * step_dev and the loss ring exactly what the untraced entry leaves; (b) for every recorded step t, record[0:P] equals the params
 * an untraced call ending after t - 1 steps leaves and record[P:2P+4] the grads an untraced call ending after t steps leaves;
 * (c) replica r's ring equals the ring of vaek_train_loop_gen_traj run alone on replica r's slices with seeds[r], lrs[r], its A.
 * VAEK_ERR_INVALID (with a message, every buffer untouched): every < 1, cap < 1, NULL buf, record_stride < the record length,
 * replica_stride < cap * record_stride in the replica form, a wrong struct_size, and everything the untraced entry refuses.
 * n_steps == 0 returns VAEK_OK and touches nothing. */
typedef struct vaek_trajectory {
    int32_t struct_size;     /* = sizeof(vaek_trajectory), ABI guard */
    int32_t every;           /* >= 1: Adam steps t with t % every == 0 are recorded */
    float*  buf;             /* device; replica r's ring starts at buf + r * replica_stride */
    int64_t cap;             /* records per ring; step t -> slot (t / every - 1) % cap */
    int64_t record_stride;   /* floats between two records, >= vaek_trajectory_record_len */
    int64_t replica_stride;  /* floats between two replicas' rings, >= cap * record_stride; ignored by the solo entry */
} vaek_trajectory;
int vaek_trajectory_record_len(const vaek_ctx* ctx, int64_t* floats);
int vaek_train_loop_gen_traj(vaek_ctx* ctx, float* params, float* grads, float* m, float* v, int32_t* step_dev, int32_t kind, const float* A,
                             int32_t dd, int32_t did, int32_t pad, float var_added, int64_t row0, uint64_t seed, uint32_t tag, int32_t n_steps,
                             float lr, void* workspace, void* stream, const vaek_trajectory* traj);
int vaek_train_loop_gen_replicas_traj(vaek_ctx* ctx, float* params, float* grads, float* m, float* v, int32_t* step_dev,
                                      const vaek_replicas* rep, int32_t kind, const float* A, int32_t dd, int32_t did, int32_t pad,
                                      float var_added, int64_t row0, uint32_t tag, int32_t n_steps, float lr, void* workspace, void* stream,
                                      const vaek_trajectory* traj);
/* STATS EVENT of a replica sweep in one launch (csrc/linear_stats.hip): what the reference's compute_stats() does for one model at
 * every n_print step (model.py:153-168) -- draw `rows` real rows and `rows` latent rows, VAE.loss on them (networks.py:103-113),
 * sample a fake batch from the SAME latents (networks.py:62-65, vae.py:191-201) and score it (datasets.py score_batch) -- for N
 * models of the context's shape: workgroup r evaluates model r.  On the host one such event is two vaek_make_batch launches,
 * vaek_forward, vaek_loss_eval (both layer by layer), a chain of torch ops and several read-backs PER MODEL; here it is one launch
 * for the sweep, and nothing of a batch ever exists in HBM.  No cross-workgroup state: no counter, no wait, no atomic, no status.
 * Replica r reads params + r * state_stride (vaek_param_count floats; never written), A + r * a_stride (a_stride == 0: one matrix
 * shared; A may be NULL for kind 2), x_seeds[r], x_steps[r], z_seeds[r], z_steps[r], sample_eps[r], and
 *   - draws row i of the real batch exactly as vaek_make_batch(kind, A_r, dd, did, pad, var_added, rows, row0 = 0, x_seeds[r],
 *     step_host = x_steps[r], x_tag) writes x, and row i of the latents as vaek_make_batch(..., z_seeds[r], z_steps[r], z_tag)
 *     writes z1 / z2 (the same Philox counters and csrc/rng_dev.h maps, bit for bit);
 *   - evaluates mu = Encoder(x), samples = mu + exp(epsilon_p / 2) z1, x_hat = Decoder(samples) [+ sigmoid(SigDecoder(samples))]
 *     + z2 exp(eps / 2) with eps = params[epsilon] * eps_cli under tunable_eps, else eps_cli: loss, mean Dkl, mean mse as plain means
 *     over `rows` (what vaek_loss_eval returns on those draws);
 *   - samples fake = Decoder(z1) [+ sigmoid(SigDecoder(z1))] + z2 exp(sample_eps[r] / 2) (vaek_forward(sampling = 1, eps =
 *     sample_eps[r]) on those latents; the caller's current_epsilon: the PREVIOUS event's eps) and scores it:
 *       kind 0: mean sum_{c >= dd} fake^2;
 *       kind 1: mean sum_{c > dd} fake^2, then the manifold error as the reference's broadcast of (B,) against (B, 1) defines it: the
 *               mean over ALL pairs (i, j) of (fake[j, dd] - fake[i, :dd] . A)^2, from four float64 sums, never a B x B array;
 *       kind 2: mean (|fake[:, :dd]| - 1)^2, then mean sum_{c >= dd} fake^2.
 * RECORD of vaek_stats_record_len = 8 + L floats at out + r * out_stride, written with per-lane vector stores:
 *   [0] loss  [1] mean Dkl  [2] mean mse  [3] eps  [4], [5] the score values in the order above (a kind with one value: [5] = 0)
 *   [6], [7] 0  [8, 8 + L) epsilon_p, copied.
 * Floats between two records where out_stride exceeds the length are not touched; nothing but the records is written.
 * DEFINING PROPERTIES: per-element arithmetic is float32; every sum over rows is accumulated in float64, per thread over its rows
 * and across the workgroup in a fixed order.  So replica r's record is BITWISE what a call with n = 1 on replica r's slices
 * leaves, two runs are bitwise equal, and the record agrees with the host path (vaek_make_batch, vaek_loss_eval, vaek_forward,
 * score_batch) and the float64 oracle within the ELBO contract (1e-5 of |loss|; scores 1e-5 relative).
 * Independent of ctx.batch: `rows` is the event's own, 1 .. vaek_stats_event_max_rows() = 4096 (a cap that bounds one launch, not
 * a tuned value); n is 1 .. vaek_train_loop_max_replicas().  No workspace.  Asynchronous on `stream`, allocates nothing, does not
 * synchronise, capturable into a hipGraph.  Profile label linear_stats_replicas.
 * vaek_supports_stats_event: exactly the contexts and kinds vaek_supports_train_loop_gen accepts.
 * VAEK_ERR_INVALID (with a message, nothing touched): a NULL or unsupported context, NULL params or event, a wrong struct_size, n or
 * rows out of range, a NULL seeds, steps, sample_eps or out array, state_stride < P, out_stride < the record length, a_stride < 0,
 * NULL A for kind 0 or 1, dd or did > 16, dd + pad (+ 1 for kind 1) != data_dim, kind outside 0 .. 2, a tag >= 2^30. */
typedef struct vaek_stats_event {
    int32_t struct_size;                  /* = sizeof(vaek_stats_event), ABI guard                  */
    int32_t n;                            /* replicas = workgroups of the launch                    */
    int32_t rows;                         /* rows of the event, 1 .. vaek_stats_event_max_rows()    */
    int32_t reserved;
    int64_t state_stride;                 /* floats between two replicas' params, >= P              */
    const uint64_t* x_seeds;              /* device [n]: seed of the real batch                     */
    const uint32_t* x_steps;              /* device [n]: its RNG step                               */
    const uint64_t* z_seeds;              /* device [n]: seed of the latents                        */
    const uint32_t* z_steps;              /* device [n]: their RNG step                             */
    const float* sample_eps;              /* device [n]: eps of the sampling pass                   */
    int64_t a_stride;                     /* floats between two replicas' A; 0 = shared             */
    float* out;                           /* device: record r at out + r * out_stride               */
    int64_t out_stride;                   /* >= vaek_stats_record_len                               */
} vaek_stats_event;
int vaek_supports_stats_event(const vaek_ctx* ctx, int32_t kind, int32_t* yes);
int vaek_stats_record_len(const vaek_ctx* ctx, int64_t* floats);
int vaek_stats_event_max_rows(void);
int vaek_stats_event_replicas(vaek_ctx* ctx, const float* params, const vaek_stats_event* ev, int32_t kind, const float* A, int32_t dd,
                              int32_t did, int32_t pad, float var_added, uint32_t x_tag, uint32_t z_tag, void* stream);
/* IMPORTANCE-WEIGHTED LOG-LIKELIHOOD of N linear VAEs of the context's shape in one call (csrc/linear_loglik.hip): the stat the
 * reference reserves as `Average Log Likelihood` and never fills.  For replica r, over `rows` data rows x and `samples` = K
 * importance samples per row (xi_k ~ N(0, I_L)):
 *   z_k     = mu(x) + exp(epsilon_p / 2) * xi_k                                       mu = Encoder(x)
 *   log w_k = log p(x | z_k) + log p(z_k) - log q(z_k | x)
 *           = -1/2 [ |dec(z_k) - x|^2 e^{-eps} + D (eps + log 2 pi) ] + 1/2 sum_l ( xi_kl^2 - z_kl^2 + epsilon_p[l] )
 * with dec(z) = Decoder(z) [+ sigmoid(SigDecoder(z))] and eps = params[epsilon] * eps_cli under tunable_eps, else eps_cli.  There is
 * no decoder-noise term: this is the likelihood, not the one-sample loss of vaek_loss_eval (whose expectation is -ELBO + D / 2).
 * RECORD of vaek_log_likelihood_record_len() = 4 floats at out + r * out_stride, written with per-lane vector stores:
 *   [0] mean over rows of logsumexp_k(log w_k) - log K      the IWAE-K bound on log p(x): `Average Log Likelihood`
 *   [1] mean over rows of mean_k log w_k                    the K-sample ELBO estimate
 *   [2] mean over rows of (sum_k w_k)^2 / (K sum_k w_k^2)   the normalised effective sample size, in (0, 1]
 *   [3] eps as used.
 * Floats between two records where out_stride exceeds the length are not touched; nothing but the records and the workspace is
 * written.  Replica r reads params + r * state_stride (vaek_param_count floats; never written), z_seeds[r], z_steps[r] and
 *   - EXPLICIT ROWS (x != NULL): its rows from x + r * x_stride as [rows][D] floats (x_stride == 0: one set of rows shared by all
 *     replicas); kind, A, dd, did, pad, var_added, x_tag, x_seeds, x_steps and a_stride are ignored;
 *   - DRAWING MODE (x == NULL): row i exactly as vaek_make_batch(kind, A + r * a_stride, dd, did, pad, var_added, rows, row0 = 0,
 *     x_seeds[r], step_host = x_steps[r], x_tag) writes x (the same Philox counters and csrc/rng_dev.h maps, bit for bit).
 * BLOCK RULE of the samples: sample k of row i takes its L normals from Philox blocks q = k * ceil(L / 4) + j, j < ceil(L / 4), of
 * the latent stream vaek_make_batch draws z1 / z2 from under (z_seeds[r], z_steps[r], z_tag) -- normal l of the sample is element
 * l & 3 of block k * ceil(L / 4) + (l >> 2).  Sample 0 is therefore the z1 vaek_make_batch writes under the same seed, step and tag.
 * DEFINING PROPERTIES: per-sample arithmetic is float32, with an online log-sum-exp over k in k order; every sum over rows is
 * float64 in a fixed order (a binary tree per 256-row tile, then the tiles in tile order in a second launch: the partials cross a
 * launch boundary, nothing stored in a launch is read back in it; no atomic, counter or wait).  So replica r's record is BITWISE
 * what a call with n = 1 on replica r's slices leaves, two runs are bitwise equal, drawing mode equals explicit mode on the rows
 * vaek_make_batch writes, and the record does not depend on ctx.batch.  Slots [0], [1] agree with the float64 evaluation on the same
 * draws within the ELBO contract (1e-5 of |value|), slot [2] within 1e-5 relative.
 * rows is 1 .. vaek_log_likelihood_max_rows() = 4096 and samples 1 .. vaek_log_likelihood_max_samples() = 1024 (caps that bound the
 * length of one launch on a shared machine, not tuned values); n is 1 .. vaek_train_loop_max_replicas().  `workspace`: device memory
 * of vaek_log_likelihood_workspace_bytes(ctx, n, rows) bytes, 8-byte aligned, the call's own (not the context's), no need to clear.
 * Two launches per call whatever n is (profile labels linear_loglik_replicas, linear_loglik_finalize); asynchronous on `stream`,
 * allocates nothing, does not synchronise, capturable into a hipGraph.
 * vaek_supports_log_likelihood: float32, no hidden layers, one or two decoders, D, L <= 32 (D <= 28 with two decoders), kind
 * 0 .. 2 -- whatever ctx.batch, world and force_generic are: the call reads parameters only.
 * VAEK_ERR_INVALID (with a message, nothing touched): a NULL or unsupported context (hidden layers, bf16, a larger shape), NULL
 * params or description, a wrong struct_size, n, rows or samples out of range, a NULL z_seeds, z_steps or out, state_stride < P,
 * out_stride < 4, a NULL or misaligned workspace, z_tag >= 2^30; explicit rows: x_stride < 0 or 0 < x_stride < rows * D; drawing
 * mode: NULL x_seeds or x_steps, a_stride < 0, NULL A for kind 0 or 1, dd or did > 16, dd + pad (+ 1 for kind 1) != data_dim, kind
 * outside 0 .. 2, x_tag >= 2^30. */
typedef struct vaek_log_likelihood {
    int32_t struct_size;                  /* = sizeof(vaek_log_likelihood), ABI guard                   */
    int32_t n;                            /* replicas                                                   */
    int32_t rows;                         /* data rows, 1 .. vaek_log_likelihood_max_rows()             */
    int32_t samples;                      /* importance samples per row, 1 .. ..._max_samples()         */
    int64_t state_stride;                 /* floats between two replicas' params, >= P                  */
    const uint64_t* x_seeds;              /* device [n]: seed of the rows (drawing mode)                */
    const uint32_t* x_steps;              /* device [n]: their RNG step (drawing mode)                  */
    const uint64_t* z_seeds;              /* device [n]: seed of the samples                            */
    const uint32_t* z_steps;              /* device [n]: their RNG step                                 */
    int64_t a_stride;                     /* floats between two replicas' A; 0 = shared (drawing mode)  */
    float* out;                           /* device: record r at out + r * out_stride                   */
    int64_t out_stride;                   /* >= vaek_log_likelihood_record_len()                        */
    const float* x;                       /* device [rows][D] per replica: explicit rows; NULL = draw   */
    int64_t x_stride;                     /* floats between two replicas' rows; 0 = shared              */
} vaek_log_likelihood;
int vaek_supports_log_likelihood(const vaek_ctx* ctx, int32_t kind, int32_t* yes);
int vaek_log_likelihood_record_len(void);
int vaek_log_likelihood_max_rows(void);
int vaek_log_likelihood_max_samples(void);
int vaek_log_likelihood_workspace_bytes(const vaek_ctx* ctx, int32_t n, int32_t rows, size_t* bytes);
int vaek_log_likelihood_replicas(vaek_ctx* ctx, const float* params, const vaek_log_likelihood* ll, int32_t kind, const float* A, int32_t dd,
                                 int32_t did, int32_t pad, float var_added, uint32_t x_tag, uint32_t z_tag, void* workspace, void* stream);
/* IMPORTANCE-WEIGHTED LOG-LIKELIHOOD of N THREE-HIDDEN-LAYER MLP VAEs of the context's shape in one call (csrc/mlp3_loglik.hip).  The
 * estimator, the record (vaek_log_likelihood_record_len() = 4 floats, per-lane vector stores), the block rule of the samples, the two
 * row modes and the description struct are exactly vaek_log_likelihood_replicas'; Encoder and Decoder are the four-Dense relu stacks:
 *   mu = Encoder(x),  z_k = mu + exp(epsilon_p / 2) * xi_k,
 *   log w_k = -1/2 [ |Decoder(z_k) - x|^2 e^{-eps} + D (eps + log 2 pi) ] + 1/2 sum_l ( xi_kl^2 - z_kl^2 + epsilon_p[l] ).
 * FOUR launches per call whatever n is (profile labels mlp3_loglik_encode, mlp3_loglik_sample, mlp3_loglik_rows,
 * mlp3_loglik_finalize): rows -> mu; the flattened (row, k) pairs of a replica, a tile of contiguous columns per workgroup, -> log w
 * through matrix-core products (v_mfma_f32_16x16x4_f32, exact f32); per row the online log-sum-exp over k in k order (float32), the
 * three row values in float64 through a binary tree per 256-row tile; the tiles in tile order.  Nothing stored in a launch is read
 * back in it; no atomic, counter, wait or status word.  A column's arithmetic does not depend on its place in a tile, so replica r's
 * record is BITWISE what a call with n = 1 on its slices leaves, two runs are bitwise equal, drawing mode equals explicit mode on the
 * rows vaek_make_batch writes, and the record does not depend on ctx.batch.  Slots [0], [1] agree with the float64 evaluation on the
 * same draws within 1e-5 of |value|, slot [2] within 1e-5 relative (1e-4 on a single row), slot [3] within 1e-6.
 * rows is 1 .. vaek_log_likelihood_max_rows(), samples 1 .. vaek_log_likelihood_max_samples(), n 1 .. vaek_train_loop_max_replicas(),
 * and n * rows * samples <= vaek_mlp3_log_likelihood_max_columns() = 2^22 (a cap that bounds the workspace and the length of a call on
 * a shared machine, not a tuned value).  `workspace`: device memory of vaek_mlp3_log_likelihood_workspace_bytes(ctx, n, rows, samples)
 * bytes, 16-byte aligned, the call's own, no need to clear; it holds the rows, mu, log w and the tile partials.  The weights are read
 * one dword at a time: state_stride has no alignment rule.  Asynchronous on `stream`, allocates nothing, does not synchronise,
 * capturable into a hipGraph.
 * vaek_supports_mlp3_log_likelihood (decided once in vaek_ctx_create): float32, one decoder, exactly three hidden layers of 64 .. 256
 * units in the encoder and in the decoder (widths may differ between layers and stacks), D, L <= 32, kind 0 .. 2 -- whatever
 * ctx.batch, world and force_generic are: the call reads parameters only.  vaek_supports_log_likelihood stays false for these contexts.
 * VAEK_ERR_INVALID (message names vaek_mlp3_log_likelihood_replicas, nothing touched): the list of vaek_log_likelihood_replicas (with
 * "unsupported context" read as above and a 16-byte workspace alignment), plus n * rows * samples above the column cap.
 * vaek_mlp3_log_likelihood_workspace_bytes refuses arguments outside those ranges and leaves *bytes alone. */
int vaek_supports_mlp3_log_likelihood(const vaek_ctx* ctx, int32_t kind, int32_t* yes);
int vaek_mlp3_log_likelihood_max_columns(void);
int vaek_mlp3_log_likelihood_workspace_bytes(const vaek_ctx* ctx, int32_t n, int32_t rows, int32_t samples, size_t* bytes);
int vaek_mlp3_log_likelihood_replicas(vaek_ctx* ctx, const float* params, const vaek_log_likelihood* ll, int32_t kind, const float* A,
                                      int32_t dd, int32_t did, int32_t pad, float var_added, uint32_t x_tag, uint32_t z_tag,
                                      void* workspace, void* stream);
/* The STATS EVENT of N THREE-HIDDEN-LAYER MLP VAEs of the context's shape in one call (csrc/mlp3_stats.hip): vaek_stats_event_replicas
 * for the models of vaek_supports_mlp3_log_likelihood.  The description struct (vaek_stats_event), the draws, what is evaluated, the
 * score terms and the RECORD of vaek_stats_record_len = 8 + L floats (per-lane vector stores; floats between two records are not
 * touched) are exactly that call's; Encoder and Decoder are the four-Dense relu stacks:
 *   mu = Encoder(x),  samples = mu + exp(epsilon_p / 2) z1,  x_hat = Decoder(samples) + z2 exp(eps / 2),
 *   fake = Decoder(z1) + z2 exp(sample_eps[r] / 2).
 * TWO launches per call whatever n is (profile labels mlp3_stats_tile, mlp3_stats_finalize): a workgroup per tile of 32 rows of a
 * replica draws the rows and latents (the bits vaek_make_batch writes under (x_seeds[r], x_steps[r], x_tag) and (z_seeds[r],
 * z_steps[r], z_tag), row0 = 0), runs the encoder and then the decoder ONCE on 64 columns (samples | z1) through matrix-core products
 * (v_mfma_f32_16x16x4_f32, exact f32), evaluates each row in float32 and adds the seven row values in float64 through a binary tree
 * over the tile; the second launch adds the tiles in tile order and stores the records.  Nothing stored in a launch is read back in
 * it; no atomic, counter, wait or status word.  A row's arithmetic does not depend on its place in a tile, so replica r's record is
 * BITWISE what a call with n = 1 on its slices leaves, two runs are bitwise equal, and the record does not depend on ctx.batch or
 * state_stride.  It agrees with the float64 evaluation on the same draws and with the host path (vaek_make_batch, vaek_loss_eval,
 * vaek_forward(sampling), score_batch) within the ELBO contract: [0] .. [2] within 1e-5 of |loss|, [3] within 1e-6, a score within
 * 1e-5 of its own value, epsilon_p bitwise.
 * rows is 1 .. vaek_stats_event_max_rows() = 4096, n 1 .. vaek_train_loop_max_replicas().  `workspace`: device memory of
 * vaek_mlp3_stats_event_workspace_bytes(ctx, n, rows) bytes, 16-byte aligned, the call's own, no need to clear; it holds the tile
 * partials only.  The weights are read one dword at a time: state_stride has no alignment rule.  Asynchronous on `stream`, allocates
 * nothing, does not synchronise, capturable into a hipGraph.
 * vaek_supports_mlp3_stats_event: vaek_supports_mlp3_log_likelihood's predicate (decided once in vaek_ctx_create): float32, one
 * decoder, exactly three hidden layers of 64 .. 256 units in the encoder and in the decoder, D, L <= 32, kind 0 .. 2 -- whatever
 * ctx.batch, world and force_generic are: the call reads parameters only.  vaek_supports_stats_event and vaek_stats_event_replicas keep
 * refusing these contexts.
 * VAEK_ERR_INVALID (message names vaek_mlp3_stats_event_replicas, nothing touched): the list of vaek_stats_event_replicas (with
 * "unsupported context" read as above), plus a NULL or misaligned workspace.  vaek_mlp3_stats_event_workspace_bytes refuses n or rows
 * outside those ranges (checked before the context: they are no context's) and leaves *bytes alone. */
int vaek_supports_mlp3_stats_event(const vaek_ctx* ctx, int32_t kind, int32_t* yes);
int vaek_mlp3_stats_event_workspace_bytes(const vaek_ctx* ctx, int32_t n, int32_t rows, size_t* bytes);
int vaek_mlp3_stats_event_replicas(vaek_ctx* ctx, const float* params, const vaek_stats_event* ev, int32_t kind, const float* A,
                                   int32_t dd, int32_t did, int32_t pad, float var_added, uint32_t x_tag, uint32_t z_tag,
                                   void* workspace, void* stream);
/* COVARIANCE SPECTRA of generated and real rows (csrc/cov_spectrum.hip): the stat the reference reserves as `EigenValues` and never
 * fills -- cov_hat = jnp.cov(batch.T) of a batch and eigh of it, the "learnt eigenvalue" on generated rows and the "ground truth
 * eigenvalue" on real ones (datasets.py:113-125).  ONE workgroup of 256 threads turns one set of `rows` float32 rows of D = data_dim
 * <= 32 columns into one RECORD of vaek_cov_spectrum_record_len = D^2 + 2 D + 4 doubles, written with per-lane vector stores:
 *   [0, D) the eigenvalues of C, ascending (eigh's order)      [D, 2 D) the column means m
 *   [2 D, 2 D + D^2) C, row-major, exactly symmetric           then: sweeps run, final off_F, |C|_F, rows.
 * Doubles between two records where a stride exceeds the length are not touched; nothing but the records is written.
 * SUMMATION RULE: the column sums S1 and the D x D second-moment matrix S2 of ALL rows are accumulated in float64 on the matrix cores
 * (v_mfma_f64_16x16x4_f64, k over the rows, four per instruction, 256 rows staged in LDS at a time, the accumulators kept across the
 * tiles, the column sums from a ones operand, rows past `rows` zero rows).  A product x_i x_j is the exact float64 product of two
 * float32 values and every matrix element is ONE accumulation chain over the rows in row order: no tile partials, no workspace, no
 * second launch, no atomic, counter or wait.  m = S1 / rows, C = (S2 - rows m m^T) / (rows - 1) (ddof = 1), the upper triangle
 * computed and mirrored.
 * SOLVE RULE: cyclic Jacobi in float64 on C, D padded to even, round-robin ordering (D / 2 disjoint rotations per round, D - 1
 * rounds per sweep; a round takes its angles from the current matrix and then forms A <- J^T A J, each new element from its four
 * sources, for i <= j, mirrored).  A rotation with a_pq == 0 is skipped; t = 1 / (2 theta) where theta = (a_qq - a_pp) / (2 a_pq) is
 * too large to square.  off_F is the root of the sum of the off-diagonal squares themselves.  The solve stops when off_F <= 2^-43
 * |C|_F or after vaek_cov_spectrum_max_sweeps() = 32 sweeps (a cap that bounds one launch, not a tuned value; a caller checks the
 * reported off_F).  Ranks come from counting, ties break by index.  Nothing is clamped: a tiny negative eigenvalue of a
 * rank-deficient set is reported as it is.
 * vaek_cov_spectrum_rows: EXPLICIT rows.  Set s of n reads x + s * x_stride as [rows][D] floats (x_stride == 0: one set shared) and
 * stores its record at out + s * out_stride; one launch of n workgroups, profile label cov_spectrum_rows; n is 1 ..
 * vaek_cov_spectrum_max_sets() = 2 * vaek_train_loop_max_replicas().  vaek_supports_cov_spectrum: any context with data_dim <= 32,
 * whatever its architecture, dtype, batch or world are: the call reads rows only.
 * vaek_spectrum_event_replicas: the FUSED EVENT of N linear VAEs of the context's shape, one launch with grid (n, 2), profile label
 * spectrum_event_replicas.  `ev` has the fields of vaek_stats_event with a double* out.  Replica r's two records go to out + r *
 * out_stride (FAKE side) and + record_len (REAL side), out_stride >= 2 * record_len.  The real side draws row i exactly as
 * vaek_make_batch(kind, A + r * a_stride, dd, did, pad, var_added, rows, row0 = 0, x_seeds[r], step_host = x_steps[r], x_tag) writes
 * x; the fake side draws latent row i exactly as vaek_make_batch(..., z_seeds[r], z_steps[r], z_tag) writes z1 / z2 and forms
 * fake = Decoder(z1) [+ sigmoid(SigDecoder(z1))] + z2 exp(sample_eps[r] / 2) in float32 (vaek_forward(sampling = 1, eps =
 * sample_eps[r]) on those latents) from params + r * state_stride (never written).  Nothing of a row ever exists in HBM.
 * vaek_supports_spectrum_event: exactly vaek_supports_log_likelihood's predicate (float32, no hidden layers, one or two decoders,
 * D, L <= 32, D <= 28 with two decoders, kind 0 .. 2, any batch and world).
 * DEFINING PROPERTIES: the three row sources feed one accumulate and solve text through the same row -> tile-slot assignment, so a
 * record depends on the rows' bits only.  (i) Replica or set r's record is BITWISE what a call with n = 1 on its slices leaves;
 * (ii) two runs are bitwise equal; (iii) the fused event's REAL record is bitwise what vaek_cov_spectrum_rows leaves on the x that
 * vaek_make_batch writes under the same seed, step and tag; (iv) the fused event does not depend on ctx.batch.  C and m agree with
 * the float64 covariance of the identical rows within 1e-11 of max_k(C_kk + m_k^2) (its root for m); the eigenvalues agree with a
 * LAPACK solve of the stored C within off_F + 64 D 2^-53 |C|_F.
 * Both calls: rows is 2 .. vaek_stats_event_max_rows() = 4096 (one row has no ddof = 1 covariance); `out` is 8-byte aligned; no
 * workspace; asynchronous on `stream`, allocate nothing, do not synchronise, capturable into a hipGraph.
 * VAEK_ERR_INVALID (message names the function, nothing touched): NULL arguments, a wrong struct_size, n or rows out of range,
 * 0 < x_stride < rows * D or a negative stride, out_stride below the record length (two records for the event), a misaligned out, an
 * unsupported context, state_stride < P, a NULL seeds, steps or sample_eps array, a_stride < 0, NULL A for kind 0 or 1, dd or did
 * > 16, dd + pad (+ 1 for kind 1) != data_dim, kind outside 0 .. 2, a tag >= 2^30. */
typedef struct vaek_spectrum_event {
    int32_t struct_size;                  /* = sizeof(vaek_spectrum_event), ABI guard               */
    int32_t n;                            /* replicas: the launch has 2 n workgroups                */
    int32_t rows;                         /* rows of each side, 2 .. vaek_stats_event_max_rows()    */
    int32_t reserved;
    int64_t state_stride;                 /* floats between two replicas' params, >= P              */
    const uint64_t* x_seeds;              /* device [n]: seed of the real rows                      */
    const uint32_t* x_steps;              /* device [n]: their RNG step                             */
    const uint64_t* z_seeds;              /* device [n]: seed of the latents                        */
    const uint32_t* z_steps;              /* device [n]: their RNG step                             */
    const float* sample_eps;              /* device [n]: eps of the sampling pass                   */
    int64_t a_stride;                     /* floats between two replicas' A; 0 = shared             */
    double* out;                          /* device: fake record r at out + r * out_stride, real one behind it */
    int64_t out_stride;                   /* doubles, >= 2 * vaek_cov_spectrum_record_len           */
} vaek_spectrum_event;
int vaek_supports_cov_spectrum(const vaek_ctx* ctx, int32_t* yes);
int vaek_cov_spectrum_record_len(const vaek_ctx* ctx, int64_t* doubles);
int vaek_cov_spectrum_max_sets(void);
int vaek_cov_spectrum_max_sweeps(void);
int vaek_cov_spectrum_rows(vaek_ctx* ctx, const float* x, int32_t n, int32_t rows, int64_t x_stride, double* out, int64_t out_stride,
                           void* stream);
int vaek_supports_spectrum_event(const vaek_ctx* ctx, int32_t kind, int32_t* yes);
int vaek_spectrum_event_replicas(vaek_ctx* ctx, const float* params, const vaek_spectrum_event* ev, int32_t kind, const float* A, int32_t dd,
                                 int32_t did, int32_t pad, float var_added, uint32_t x_tag, uint32_t z_tag, void* stream);
/* EIGENVECTORS of those covariances and PRINCIPAL ANGLES between two of their eigenbases (csrc/cov_spectrum.hip): which directions
 * carry the variance, not only how many -- whether a generator's mass lies in the subspace the data lives in.
 * vaek_cov_eigen_rows and vaek_eigen_event_replicas are vaek_cov_spectrum_rows and vaek_spectrum_event_replicas with a longer RECORD
 * of vaek_cov_eigen_record_len = 2 D^2 + 2 D + 4 doubles: the spectrum record above, BITWISE and in its layout, then V row-major,
 * V[i * D + k] = component i of the eigenvector of eigenvalue k (the eigenvalues' ascending order, the same counting ranks, ties by
 * index).  SIGN: every eigenvector's component of largest magnitude is positive; a tie goes to the lowest row index.  Each Jacobi
 * round also forms V <- V J from the (c, s, mate) it publishes (V starts as I; V never feeds back into the matrix, so eigenvalues,
 * sweeps and off_F are those of the spectrum calls).  The event's records go to out + r * out_stride (fake) and + the eigen record
 * length (real), out_stride >= 2 * that length.  Same predicates (vaek_supports_cov_spectrum, vaek_supports_spectrum_event), same
 * ranges, same refusal lists, same properties (i) .. (iv); profile labels cov_eigen_rows and eigen_event_replicas.  C V = V diag(lambda)
 * holds within off_F + 256 D 2^-53 |C|_F in the Frobenius norm and max |V^T V - I| <= 4 D (sweeps + 1) 2^-53.
 * vaek_subspace_angles: pair p of n (1 .. vaek_cov_spectrum_max_sets(), one workgroup of 256 threads each) reads the EIGEN records at
 * a + p * a_stride and b + p * b_stride, written by an earlier launch.  U = the ka eigenvectors of a's largest eigenvalues, W = the kb
 * of b's, 1 <= kb <= ka <= D.  In float64: M = U^T W, R = W - U M formed explicitly, G = R^T R (i <= j, mirrored), and G's eigenvalues
 * by the SOLVE RULE above (the same device routine).  RECORD of vaek_subspace_record_len(kb) = kb + 4 doubles at out + p * out_stride:
 *   [0, kb) sin^2 of the principal angles, ascending, unclamped      [kb] |sin Theta|_F^2 = the sum of the squares of R's elements
 *   [kb + 1] sweeps run      [kb + 2] final off_F of G      [kb + 3] max(max |U^T U - I|, max |W^T W - I|).
 * No workspace, atomics, counters or waits; per-lane vector stores of the records only; pair p's record is bitwise the n = 1 call's.
 * Asynchronous, allocates nothing, capturable; profile label subspace_angles.  VAEK_ERR_INVALID (message, nothing touched): NULL
 * pointers, data_dim > 32, n, ka or kb out of range, a_stride or b_stride below the eigen record length, out_stride < kb + 4, an a, b
 * or out that is not 8-byte aligned. */
int vaek_cov_eigen_record_len(const vaek_ctx* ctx, int64_t* doubles);
int vaek_cov_eigen_rows(vaek_ctx* ctx, const float* x, int32_t n, int32_t rows, int64_t x_stride, double* out, int64_t out_stride,
                        void* stream);
int vaek_eigen_event_replicas(vaek_ctx* ctx, const float* params, const vaek_spectrum_event* ev, int32_t kind, const float* A, int32_t dd,
                              int32_t did, int32_t pad, float var_added, uint32_t x_tag, uint32_t z_tag, void* stream);
int vaek_subspace_record_len(int32_t kb);
int vaek_subspace_angles(vaek_ctx* ctx, const double* a, int64_t a_stride, const double* b, int64_t b_stride, int32_t n, int32_t ka,
                         int32_t kb, double* out, int64_t out_stride, void* stream);
/* EXACT LOG-LIKELIHOOD, EXACT ELBO and POSTERIOR GAP of N one-decoder linear VAEs of the context's shape in one launch
 * (csrc/cov_spectrum.hip).  Such a model is a linear-Gaussian latent-variable model, so nothing has to be estimated:
 *   p(x) = N(b_d, K^T K + e^{eps} I)      K = the Decoder kernel [L][D], b_d its bias, eps as in vaek_log_likelihood_replicas
 * and the ELBO of the diagonal-Gaussian encoder (kernel E [D][L], bias b_e, epsilon_p [L]) is closed form too; their difference is
 * KL(q(z | x) || p(z | x)) >= 0.  Parameters are float32; every quantity below is float64.  Per model r (ONE workgroup of 256 threads):
 *   G = K^T K (D x D; element (i, j) one chain over l in l order of exact float64 products of two float32 values, the upper triangle
 *   computed and mirrored), |G|_F, G = V diag(lambda) V^T by the SOLVE RULE of vaek_cov_spectrum_rows with eigenvectors (the same
 *   device routine, its ordering, 2^-43 stop and 32-sweep cap; G = 0 ends with 0 sweeps), s_i = max(lambda_i, 0) + e^{eps} (the one
 *   place that uses G being PSD), logdet = sum_i log s_i, T = sum_l e^{epsilon_p[l]} |K_l|^2.
 * Per row x (float32, widened):
 *   c = x - b_d, y = V^T c, quad = sum_i y_i^2 / s_i,          log p(x) = -1/2 (quad + logdet + D log 2 pi)
 *   mu = x E + b_e, r = mu K + b_d - x,
 *   ELBO(x) = -1/2 [ e^{-eps} (|r|^2 + T) + D (eps + log 2 pi) ] - 1/2 sum_l ( e^{epsilon_p[l]} + mu_l^2 - 1 - epsilon_p[l] )
 *   gap(x) = log p(x) - ELBO(x).
 * The D x D eigenvector form is used because trained decoders are rank-deficient (collapsed latent rows) and e^{eps} is small: V
 * from Jacobi is orthonormal whatever the rank, where the L x L (Woodbury) form subtracts nearly equal numbers and divides by e^{eps}.
 * RECORD of vaek_exact_log_likelihood_record_len = 10 + D doubles at out + r * out_stride, written with per-lane vector stores:
 *   [0] mean log p(x)      [1] mean ELBO      [2] mean gap      [3] eps as used      [4] logdet      [5] sweeps run
 *   [6] final off_F        [7] |G|_F          [8] (off_F + 64 D 2^-53 |G|_F) e^{-eps}: the bound on the relative error of the
 *   smallest s_i -- the conditioning of the evaluation, reported, not hidden                          [9] rows
 *   [10, 10 + D) the eigenvalues of K^T K, ascending, unclamped (counting ranks, ties by index).
 * row_out (optional; NULL: none): [rows][2] doubles per model at row_out + r * row_stride: log p(x_i), ELBO(x_i).  Doubles between
 * two records or two row blocks where a stride exceeds the length are not touched; nothing else is written.
 * Thread t takes rows 256 j + t in j order and keeps three private running sums (log p, ELBO, gap); one fixed binary tree per sum
 * adds the 256 threads'; a mean is a sum divided by rows.  No workspace, no second launch, no atomic, counter or wait.  So replica
 * r's record is BITWISE what a call with n = 1 on its slices leaves, two runs are bitwise equal, drawing mode equals explicit mode
 * on the rows vaek_make_batch writes, the record depends on neither ctx.batch nor row_out.
 * The two row modes are vaek_log_likelihood_replicas': EXPLICIT ROWS (x != NULL: x + r * x_stride as [rows][D] floats, x_stride == 0
 * shared) and DRAWING MODE (x == NULL: row i exactly as vaek_make_batch(kind, A + r * a_stride, dd, did, pad, var_added, rows,
 * row0 = 0, x_seeds[r], step_host = x_steps[r], x_tag) writes x).  rows is 1 .. vaek_log_likelihood_max_rows(), n 1 ..
 * vaek_train_loop_max_replicas().  Asynchronous on `stream`, allocates nothing, does not synchronise, capturable into a hipGraph;
 * profile label exact_loglik_replicas.
 * vaek_supports_exact_log_likelihood: vaek_supports_log_likelihood AND one decoder (the sigmoid second decoder has no closed form)
 * -- whatever ctx.batch, world and force_generic are.
 * VAEK_ERR_INVALID (message names vaek_exact_log_likelihood_replicas, nothing touched): a NULL or unsupported context (hidden
 * layers, bf16, a larger shape, two decoders), NULL params or description, a wrong struct_size, n or rows out of range, a NULL out,
 * state_stride < P, out_stride below the record length, an out or row_out that is not 8-byte aligned, row_stride < 2 * rows with a
 * row_out (0 included, unless n == 1); explicit rows: x_stride < 0 or 0 < x_stride < rows * D; drawing mode: NULL x_seeds or x_steps,
 * a_stride < 0, NULL A for kind 0 or 1, dd or did > 16, dd + pad (+ 1 for kind 1) != data_dim, kind outside 0 .. 2, x_tag >= 2^30. */
typedef struct vaek_exact_log_likelihood {
    int32_t struct_size;                  /* = sizeof(vaek_exact_log_likelihood), ABI guard             */
    int32_t n;                            /* replicas: the launch has n workgroups                      */
    int32_t rows;                         /* data rows, 1 .. vaek_log_likelihood_max_rows()             */
    int32_t reserved;
    int64_t state_stride;                 /* floats between two replicas' params, >= P                  */
    const uint64_t* x_seeds;              /* device [n]: seed of the rows (drawing mode)                */
    const uint32_t* x_steps;              /* device [n]: their RNG step (drawing mode)                  */
    int64_t a_stride;                     /* floats between two replicas' A; 0 = shared (drawing mode)  */
    double* out;                          /* device: record r at out + r * out_stride                   */
    int64_t out_stride;                   /* doubles, >= vaek_exact_log_likelihood_record_len           */
    const float* x;                       /* device [rows][D] per replica: explicit rows; NULL = draw   */
    int64_t x_stride;                     /* floats between two replicas' rows; 0 = shared              */
    double* row_out;                      /* device [rows][2] per replica, or NULL                      */
    int64_t row_stride;                   /* doubles between two replicas' row blocks, >= 2 * rows      */
} vaek_exact_log_likelihood;
int vaek_supports_exact_log_likelihood(const vaek_ctx* ctx, int32_t kind, int32_t* yes);
int vaek_exact_log_likelihood_record_len(const vaek_ctx* ctx, int64_t* doubles);
int vaek_exact_log_likelihood_replicas(vaek_ctx* ctx, const float* params, const vaek_exact_log_likelihood* ll, int32_t kind,
                                       const float* A, int32_t dd, int32_t did, int32_t pad, float var_added, uint32_t x_tag,
                                       void* stream);
/* HESSIAN OF THE EXACT ELBO of N one-decoder linear VAEs of the context's shape in one launch (csrc/elbo_hessian.hip): Hessian-vector
 * products, the exact gradient and a Lanczos spectrum of
 *   f(theta) = - mean_x ELBO(x),      ELBO(x) exactly as vaek_exact_log_likelihood_replicas defines it above,
 * the population training objective on the rows (it differs from the expectation of the training loss by the constant D / 2 of the z2
 * term).  theta is the parameter vector in the library's leaf order: E [D][L], b_e [L], K [L][D], b_d [D], epsilon_p = p [L] and, under
 * tunable_eps, epsilon = c [1]; P = vaek_param_count.  The float32 leaves are widened to float64 once and everything below is float64;
 * eps = c * eps_cli formed in FLOAT64 (eps_cli without tunable_eps), so f is a smooth function of c.  vaek_exact_log_likelihood_replicas
 * forms that product in float32: record [0] below is minus its record [1] to rounding wherever c * eps_cli is exact in float32 (c = 1,
 * the initial value), and to 2^-24 |eps| D / 2 otherwise.  Over `rows` float32 rows x, widened:
 *   S = (1 / rows) sum [x; 1][x; 1]^T  ((D + 1) x (D + 1))     U = [E; b_e]     C = [-I_D; b_d]     R = U K + C
 *   a = e^{-eps}     w = e^{p}     k2_l = |K_l|^2     Q = tr(R^T S R) + sum_l w_l k2_l
 *   f = 1/2 tr(U^T S U) + 1/2 sum_l (w_l - 1 - p_l) + 1/2 a Q + 1/2 D (eps + log 2 pi)                          G = a S R
 *   df/dU = S U + G K^T     df/dK = U^T G + a diag(w) K     df/db_d = last row of G
 *   df/dp_l = 1/2 (w_l - 1) + 1/2 a w_l k2_l                df/dc = eps_cli (D / 2 - a Q / 2)
 * and for a direction v = (dU, dK, db_d, dp, dc), with deps = eps_cli dc (0 without tunable_eps), dw = w dp, dC = [0; db_d]:
 *   dR = dU K + U dK + dC                                   dG = a S dR - deps G
 *   (Hv)_U = S dU + dG K^T + G dK^T
 *   (Hv)_K = dU^T G + U^T dG + a diag(w) dK + a diag(dw) K - deps a diag(w) K
 *   (Hv)_b_d = last row of dG
 *   (Hv)_p_l = 1/2 dw_l + 1/2 a dw_l k2_l + a w_l (K_l . dK_l) - 1/2 deps a w_l k2_l
 *   dQ = 2 tr(R^T S dR) + sum_l (dw_l k2_l + 2 w_l K_l . dK_l)            (Hv)_c = eps_cli (deps a Q / 2 - a dQ / 2).
 * H never exists as a matrix: f sees the rows through S alone, so a product is a handful of products of matrices of at most 33 x 32,
 * whatever `rows` is.  ONE workgroup of 256 threads per model, no workspace, no second launch, no atomic, counter or wait:
 *   S: the rows through the row sources and the row -> slot assignment of vaek_cov_spectrum_rows (thread t produces rows 256 j + t;
 *   sum x x^T and sum x on the float64 matrix cores, every element ONE chain over the rows in row order), so the results depend on the
 *   rows' bits only; the products: plain float64 fmas, thread t owning elements t, t + 256, .. of an output, every sum in index order,
 *   every sum over threads one fixed binary tree.
 * vaek_elbo_hvp_replicas: for replica r and i < nvec, hv + r * hv_stride + i * P <- H (v + r * v_stride + i * P) ([nvec][P] doubles per
 * replica, v_stride == 0: one set of directions shared by all replicas); grad (optional; NULL: none): the gradient, [P] doubles at grad
 * + r * grad_stride; RECORD of vaek_elbo_hvp_record_len() = 4 doubles at out + r * out_stride: [0] f  [1] |grad f|_2  [2] eps as used
 * [3] rows.  nvec is 0 .. vaek_elbo_hvp_max_vectors() = 64 (a cap on the length of a launch, not a tuned value); nvec = 0 gives the
 * gradient and the record only (v and hv are not read and may be NULL).  v and hv must NOT overlap: a direction is read again after
 * parts of its product are stored.  Unit vectors give columns of H, 64 a call.
 * vaek_elbo_hessian_lanczos_replicas: m = `steps` <= vaek_elbo_hessian_max_steps() = 32 Lanczos steps on H from the start vector v0 + r
 * * v0_stride ([P] doubles, v0_stride == 0: shared; normalised in the kernel), with FULL reorthogonalisation: step j forms w = H v_j,
 * applies classical Gram-Schmidt twice against v_1 .. v_j (alpha_j = the sum of what the two passes take out along v_j), beta_j = |w|,
 * v_{j+1} = w / beta_j.  BREAKDOWN -- beta_j <= 2^-40 max(|alpha_1 .. alpha_j|, beta_1 .. beta_{j-1}) -- ends the run; it is not an
 * error (it happens at small P and on symmetric models).  k = min(steps, P, the step of breakdown) steps are reported; v0 = 0 (or not
 * finite) gives k = 0.  The BASIS is an output: row j < k of basis + r * basis_stride ([steps][P] doubles, vaek_elbo_hessian_basis_doubles
 * = steps * P) holds v_{j+1}; rows >= k are not written.  The k x k tridiagonal T (alpha on, beta_1 .. beta_{k-1} beside the diagonal)
 * is solved by the SOLVE RULE of vaek_cov_spectrum_rows with eigenvectors (the same device routine, its 2^-43 stop and 32-sweep cap; an
 * odd k padded with a zero row and column, excluded by index; T may be indefinite).  Ritz value theta_i comes with rho_i = |beta_k
 * s_{k,i}|, s_{k,i} the last component of T's i-th eigenvector: in exact arithmetic an eigenvalue of H lies within rho_i of theta_i.
 * RECORD of vaek_elbo_hessian_record_len() = 12 + 4 * 32 = 140 doubles at out + r * out_stride:
 *   [0] f   [1] |grad f|_2   [2] k   [3] beta_k   [4] Jacobi sweeps   [5] off_F   [6] |T|_F   [7] rows   [8] eps as used
 *   [9] theta_max   [10] theta_min   [11] omega = max_{i < j < k} |v_i . v_j| of the stored basis, measured after the run
 *   [12, 44) theta ascending (counting ranks, ties by index)   [44, 76) rho in the same order   [76, 108) alpha_1 .. alpha_k
 *   [108, 140) beta_1 .. beta_k                                                                       (slots >= k are 0)
 * Both calls: replica r reads params + r * state_stride (never written) and its rows in the two modes of
 * vaek_exact_log_likelihood_replicas (EXPLICIT ROWS x != NULL, x_stride == 0 shared; DRAWING MODE x == NULL: row i as vaek_make_batch
 * writes x under (x_seeds[r], x_steps[r], x_tag)).  rows is 1 .. vaek_log_likelihood_max_rows() = 4096, n 1 ..
 * vaek_train_loop_max_replicas().  Doubles between two replicas' blocks where a stride exceeds the length are not touched; nothing but
 * the named outputs is written.  Replica r's outputs are BITWISE what a call with n = 1 on its slices leaves, two runs are bitwise
 * equal, drawing mode equals explicit mode on the rows vaek_make_batch writes, nothing depends on ctx.batch.  Asynchronous on `stream`,
 * allocates nothing, does not synchronise, capturable into a hipGraph; profile labels elbo_hvp_replicas / elbo_hessian_replicas.
 * vaek_supports_elbo_hessian: vaek_supports_exact_log_likelihood's predicate (float32, no hidden layers, ONE decoder, D, L <= 32) --
 * whatever ctx.batch, world and force_generic are.  NOT covered: two-decoder and MLP models (no closed form; two-decoder linear models
 * have vaek_sampled_elbo_hessian_lanczos_replicas below), bf16, D or L > 32, more than 32 steps, Ritz vectors.
 * VAEK_ERR_INVALID (message names the call, nothing touched): a NULL or unsupported context, NULL params or description, a wrong
 * struct_size, n or rows out of range, state_stride < P; explicit rows: x_stride < 0 or 0 < x_stride < rows * D; drawing mode: NULL
 * x_seeds or x_steps, a_stride < 0, NULL A for kind 0 or 1, dd or did > 16, dd + pad (+ 1 for kind 1) != data_dim, kind outside 0 .. 2,
 * x_tag >= 2^30; nvec outside 0 .. 64 or steps outside 1 .. 32; a NULL out, v0 or basis, a NULL v or hv with nvec > 0; a double buffer
 * (grad included, where given) that is not 8-byte aligned; out_stride below the record length, hv_stride < nvec * P, grad_stride < P,
 * basis_stride < steps * P, a v_stride or v0_stride that is neither 0 nor at least its length (nvec * P, P).
 * vaek_elbo_hessian_basis_doubles refuses an unsupported context and steps outside 1 .. 32 and leaves *doubles alone. */
typedef struct vaek_elbo_hvp {
    int32_t struct_size;                  /* = sizeof(vaek_elbo_hvp), ABI guard                         */
    int32_t n;                            /* replicas: the launch has n workgroups                      */
    int32_t rows;                         /* data rows, 1 .. vaek_log_likelihood_max_rows()             */
    int32_t nvec;                         /* directions per replica, 0 .. vaek_elbo_hvp_max_vectors()   */
    int64_t state_stride;                 /* floats between two replicas' params, >= P                  */
    const uint64_t* x_seeds;              /* device [n]: seed of the rows (drawing mode)                */
    const uint32_t* x_steps;              /* device [n]: their RNG step (drawing mode)                  */
    int64_t a_stride;                     /* floats between two replicas' A; 0 = shared (drawing mode)  */
    const float* x;                       /* device [rows][D] per replica: explicit rows; NULL = draw   */
    int64_t x_stride;                     /* floats between two replicas' rows; 0 = shared              */
    const double* v;                      /* device [nvec][P] per replica: the directions               */
    int64_t v_stride;                     /* doubles between two replicas' directions; 0 = shared       */
    double* hv;                           /* device [nvec][P] per replica: H v                          */
    int64_t hv_stride;                    /* doubles, >= nvec * P                                       */
    double* grad;                         /* device [P] per replica, or NULL                            */
    int64_t grad_stride;                  /* doubles, >= P                                              */
    double* out;                          /* device: record r at out + r * out_stride                   */
    int64_t out_stride;                   /* doubles, >= vaek_elbo_hvp_record_len()                     */
} vaek_elbo_hvp;
typedef struct vaek_elbo_hessian {
    int32_t struct_size;                  /* = sizeof(vaek_elbo_hessian), ABI guard                     */
    int32_t n;                            /* replicas: the launch has n workgroups                      */
    int32_t rows;                         /* data rows, 1 .. vaek_log_likelihood_max_rows()             */
    int32_t steps;                        /* Lanczos steps, 1 .. vaek_elbo_hessian_max_steps()          */
    int64_t state_stride;                 /* floats between two replicas' params, >= P                  */
    const uint64_t* x_seeds;              /* device [n]: seed of the rows (drawing mode)                */
    const uint32_t* x_steps;              /* device [n]: their RNG step (drawing mode)                  */
    int64_t a_stride;                     /* floats between two replicas' A; 0 = shared (drawing mode)  */
    const float* x;                       /* device [rows][D] per replica: explicit rows; NULL = draw   */
    int64_t x_stride;                     /* floats between two replicas' rows; 0 = shared              */
    const double* v0;                     /* device [P] per replica: the start vector                   */
    int64_t v0_stride;                    /* doubles between two replicas' start vectors; 0 = shared    */
    double* basis;                        /* device [steps][P] per replica: the Lanczos vectors (output)*/
    int64_t basis_stride;                 /* doubles, >= steps * P (vaek_elbo_hessian_basis_doubles)    */
    double* out;                          /* device: record r at out + r * out_stride                   */
    int64_t out_stride;                   /* doubles, >= vaek_elbo_hessian_record_len()                 */
} vaek_elbo_hessian;
int vaek_supports_elbo_hessian(const vaek_ctx* ctx, int32_t kind, int32_t* yes);
int vaek_elbo_hvp_max_vectors(void);
int vaek_elbo_hvp_record_len(void);
int vaek_elbo_hessian_max_steps(void);
int vaek_elbo_hessian_record_len(void);
int vaek_elbo_hessian_basis_doubles(const vaek_ctx* ctx, int32_t steps, int64_t* doubles);
int vaek_elbo_hvp_replicas(vaek_ctx* ctx, const float* params, const vaek_elbo_hvp* hp, int32_t kind, const float* A, int32_t dd,
                           int32_t did, int32_t pad, float var_added, uint32_t x_tag, void* stream);
int vaek_elbo_hessian_lanczos_replicas(vaek_ctx* ctx, const float* params, const vaek_elbo_hessian* hs, int32_t kind, const float* A,
                                       int32_t dd, int32_t did, int32_t pad, float var_added, uint32_t x_tag, void* stream);
/* HESSIAN OF THE SAMPLE-AVERAGE ELBO of N linear VAEs with ONE OR TWO decoders (csrc/sampled_hessian.hip): the ELBO of a model with the
 * sigmoid second decoder has no closed form in the moments of the rows, so fix the rows AND K latent samples xi_ik per row (common random
 * numbers): the Monte-Carlo ELBO is then a smooth deterministic function f_K of the parameters, and its gradient and Hessian-vector
 * products are exact derivatives of that function, forward-over-reverse differentiation written out by hand.  Nothing is
 * finite-differenced.  theta is the flat parameter vector in the leaf order E [D][L], b_e [L], K [L][D], b_d [D], with two decoders K_s
 * [L][D], b_s [D] (SigDecoder/FC0), then p = epsilon_p [L] and, under tunable_eps, c = epsilon [1]; P = vaek_param_count.  Leaves, rows
 * and samples are widened to float64 once and everything below is float64; eps = c * eps_cli in float64 as in vaek_elbo_hvp_replicas.
 * With N = rows * K columns (i, k), c0 = e^{-eps} / N, c1 = 1 / N, sd = e^{p / 2}, w = e^{p}:
 *   mu = x E + b_e     s = mu + sd xi     y = s K + b_d     u = s K_s + b_s     sg = sigmoid(u)     r = y [+ sg] - x
 *   f_K = sum_ik c1 |mu|^2 / 2 + 1/2 sum_l (w_l - 1 - p_l) + 1/2 sum_ik c0 |r|^2 + 1/2 D (eps + log 2 pi)
 * (the decoder noise z2 is integrated out: f_K uses the convention of the f of vaek_elbo_hvp_replicas, and for ONE decoder f_K = f
 * identically in theta whenever each row's samples have mean 0 and second moment I, e.g. the 2 L sigma points +- sqrt(L) e_l).
 *   g_y = c0 r     g_a = g_y sg'     g_s = g_y K^T + g_a K_s^T     g_mu = g_s + c1 mu          sg' = sg (1 - sg)   sg'' = sg' (1 - 2 sg)
 *   df/dE = sum x^T g_mu   df/db_e = sum g_mu   df/dK = sum s^T g_y   df/db_d = sum g_y   df/dK_s = sum s^T g_a   df/db_s = sum g_a
 *   df/dp_l = 1/2 (w_l - 1) + sum g_s,l (sd_l xi_l / 2)          df/dc = eps_cli (D / 2 - 1/2 sum c0 |r|^2)
 * and for a direction v = (dE, db_e, dK, db_d, dK_s, db_s, dp, dc) with deps = eps_cli dc (0 without tunable_eps):
 *   dmu = x dE + db_e     ds = dmu + dp sd xi / 2     dy = ds K + s dK + db_d     du = ds K_s + s dK_s + db_s     dr = dy + sg' du
 *   dg_y = c0 (dr - deps r)     dg_a = dg_y sg' + g_y sg'' du     dg_s = dg_y K^T + g_y dK^T + dg_a K_s^T + g_a dK_s^T     dg_mu = dg_s + c1 dmu
 *   (Hv)_E = sum x^T dg_mu   (Hv)_b_e = sum dg_mu   (Hv)_K = sum (ds^T g_y + s^T dg_y)   (Hv)_b_d = sum dg_y
 *   (Hv)_K_s = sum (ds^T g_a + s^T dg_a)   (Hv)_b_s = sum dg_a
 *   (Hv)_p_l = 1/2 w_l dp_l + sum (dg_s,l sd_l xi_l / 2 + g_s,l dp_l sd_l xi_l / 4)
 *   (Hv)_c = eps_cli sum c0 r . (deps r / 2 - dr).
 * COLUMN TILES: column q = i K + k; a workgroup of 256 threads takes 256 columns of one replica, 32 at a time, and stores ONE PARTIAL of
 * the P elements (and of f_K) into the workspace; the products (columns x D by D x L and back) and the contractions over the columns run
 * on v_mfma_f64_16x16x4_f64, and every element of a partial is ONE chain over the tile's columns in column order.  A second launch of n
 * workgroups adds the tiles' partials in tile order.  The partials cross a launch boundary: nothing stored in a launch is read back in it,
 * no atomic, counter, wait or spin.  ROWS: the two modes of vaek_elbo_hvp_replicas.  SAMPLES: xi != NULL: xi + r * xi_stride as
 * [rows * samples][L] floats (xi_stride == 0: shared); xi == NULL: sample k of row i by the BLOCK RULE of vaek_log_likelihood_replicas
 * under (z_seeds[r], z_steps[r], z_tag), so sample 0 of row i is the z1 vaek_make_batch writes.
 * vaek_sampled_elbo_hvp_replicas: vaek_elbo_hvp_replicas' outputs (hv, grad, the 4-double record f_K, |grad f_K|_2, eps, rows), the same
 * stride rules; v and hv must not overlap (refused); nvec = 0 .. 64, nvec = 0 gives the gradient and the record only.  LAUNCHES: 2 + 2 nvec.
 * vaek_sampled_elbo_hessian_lanczos_replicas: the Lanczos run of vaek_elbo_hessian_lanczos_replicas (full reorthogonalisation, classical
 * Gram-Schmidt twice, every dot one fixed tree, the same breakdown test, k = min(steps, P, breakdown), v0 = 0 or not finite: k = 0, basis
 * rows >= k not written, T solved by the SOLVE RULE with an odd k padded) with the recursion ACROSS launches: per step one tile launch and
 * one launch of n workgroups; a replica that is done leaves a flag in the workspace and later launches do nothing for it.  LAUNCHES: 3 + 2
 * steps.  RECORD of vaek_sampled_elbo_hessian_record_len() = 142 doubles: [0, 140) exactly the slots of vaek_elbo_hessian_record_len's
 * record, [140] K, [141] 1.0 with two decoders, else 0.0.
 * Both calls: rows 1 .. 4096, samples 1 .. vaek_log_likelihood_max_samples() = 1024, rows * samples <= 2^16 per replica and n * rows *
 * samples <= vaek_sampled_elbo_hessian_max_columns() = 2^22 (caps on the length of a launch, not tuned values).  The workspace of
 * vaek_sampled_elbo_hessian_workspace_bytes(ctx, n, rows, samples) bytes is the call's own, 16-byte aligned.  Replica r's outputs are
 * BITWISE what a call with n = 1 on its slices leaves, two runs are bitwise equal, drawing mode equals explicit mode on the bits
 * vaek_make_batch and the block rule produce, nothing depends on ctx.batch.  Doubles between two replicas' blocks are not touched.
 * Asynchronous on `stream`, allocates nothing, does not synchronise, capturable into a hipGraph.
 * vaek_supports_sampled_elbo_hessian: vaek_supports_log_likelihood's predicate (float32, no hidden layers, one OR two decoders, D, L <=
 * 32, D <= 28 with two, kind 0 .. 2), whatever ctx.batch, world and force_generic are.  NOT covered: MLP models, bf16, D or L > 32, Ritz
 * vectors, more than 32 steps, data parallelism.
 * VAEK_ERR_INVALID (message names the call, the field, its value, the bound and the query function; nothing touched): the list of
 * vaek_elbo_hvp_replicas / vaek_elbo_hessian_lanczos_replicas, plus samples or the column products out of range, 0 < xi_stride < rows *
 * samples * L or a negative one, NULL z_seeds or z_steps with xi == NULL, z_tag >= 2^30, overlapping v and hv, a NULL or misaligned
 * workspace (a short one cannot be detected). */
typedef struct vaek_sampled_elbo_hvp {
    int32_t struct_size;                  /* = sizeof(vaek_sampled_elbo_hvp), ABI guard                 */
    int32_t n;                            /* replicas                                                   */
    int32_t rows;                         /* data rows, 1 .. vaek_log_likelihood_max_rows()             */
    int32_t nvec;                         /* directions per replica, 0 .. vaek_elbo_hvp_max_vectors()   */
    int64_t state_stride;                 /* floats between two replicas' params, >= P                  */
    const uint64_t* x_seeds;              /* device [n]: seed of the rows (drawing mode)                */
    const uint32_t* x_steps;              /* device [n]: their RNG step (drawing mode)                  */
    int64_t a_stride;                     /* floats between two replicas' A; 0 = shared (drawing mode)  */
    const float* x;                       /* device [rows][D] per replica: explicit rows; NULL = draw   */
    int64_t x_stride;                     /* floats between two replicas' rows; 0 = shared              */
    const double* v;                      /* device [nvec][P] per replica: the directions               */
    int64_t v_stride;                     /* doubles between two replicas' directions; 0 = shared       */
    double* hv;                           /* device [nvec][P] per replica: H v                          */
    int64_t hv_stride;                    /* doubles, >= nvec * P                                       */
    double* grad;                         /* device [P] per replica, or NULL                            */
    int64_t grad_stride;                  /* doubles, >= P                                              */
    double* out;                          /* device: record r at out + r * out_stride                   */
    int64_t out_stride;                   /* doubles, >= vaek_elbo_hvp_record_len()                     */
    int32_t samples;                      /* K: samples per row, 1 .. vaek_log_likelihood_max_samples() */
    int32_t reserved;
    const uint64_t* z_seeds;              /* device [n]: seed of the samples (xi == NULL)               */
    const uint32_t* z_steps;              /* device [n]: their RNG step (xi == NULL)                    */
    const float* xi;                      /* device [rows * samples][L] per replica; NULL = draw        */
    int64_t xi_stride;                    /* floats between two replicas' samples; 0 = shared           */
} vaek_sampled_elbo_hvp;
typedef struct vaek_sampled_elbo_hessian {
    int32_t struct_size;                  /* = sizeof(vaek_sampled_elbo_hessian), ABI guard             */
    int32_t n;                            /* replicas                                                   */
    int32_t rows;                         /* data rows, 1 .. vaek_log_likelihood_max_rows()             */
    int32_t steps;                        /* Lanczos steps, 1 .. vaek_elbo_hessian_max_steps()          */
    int64_t state_stride;                 /* floats between two replicas' params, >= P                  */
    const uint64_t* x_seeds;              /* device [n]: seed of the rows (drawing mode)                */
    const uint32_t* x_steps;              /* device [n]: their RNG step (drawing mode)                  */
    int64_t a_stride;                     /* floats between two replicas' A; 0 = shared (drawing mode)  */
    const float* x;                       /* device [rows][D] per replica: explicit rows; NULL = draw   */
    int64_t x_stride;                     /* floats between two replicas' rows; 0 = shared              */
    const double* v0;                     /* device [P] per replica: the start vector                   */
    int64_t v0_stride;                    /* doubles between two replicas' start vectors; 0 = shared    */
    double* basis;                        /* device [steps][P] per replica: the Lanczos vectors (output)*/
    int64_t basis_stride;                 /* doubles, >= steps * P (vaek_elbo_hessian_basis_doubles)    */
    double* out;                          /* device: record r at out + r * out_stride                   */
    int64_t out_stride;                   /* doubles, >= vaek_sampled_elbo_hessian_record_len()         */
    int32_t samples;                      /* K: samples per row, 1 .. vaek_log_likelihood_max_samples() */
    int32_t reserved;
    const uint64_t* z_seeds;              /* device [n]: seed of the samples (xi == NULL)               */
    const uint32_t* z_steps;              /* device [n]: their RNG step (xi == NULL)                    */
    const float* xi;                      /* device [rows * samples][L] per replica; NULL = draw        */
    int64_t xi_stride;                    /* floats between two replicas' samples; 0 = shared           */
} vaek_sampled_elbo_hessian;
int vaek_supports_sampled_elbo_hessian(const vaek_ctx* ctx, int32_t kind, int32_t* yes);
int vaek_sampled_elbo_hessian_max_columns(void);
int vaek_sampled_elbo_hessian_record_len(void);
int vaek_sampled_elbo_hessian_workspace_bytes(const vaek_ctx* ctx, int32_t n, int32_t rows, int32_t samples, size_t* bytes);
int vaek_sampled_elbo_hvp_replicas(vaek_ctx* ctx, const float* params, const vaek_sampled_elbo_hvp* hp, int32_t kind, const float* A,
                                   int32_t dd, int32_t did, int32_t pad, float var_added, uint32_t x_tag, uint32_t z_tag, void* workspace,
                                   void* stream);
int vaek_sampled_elbo_hessian_lanczos_replicas(vaek_ctx* ctx, const float* params, const vaek_sampled_elbo_hessian* hs, int32_t kind,
                                               const float* A, int32_t dd, int32_t did, int32_t pad, float var_added, uint32_t x_tag,
                                               uint32_t z_tag, void* workspace, void* stream);
/* HESSIAN OF THE SAMPLE-AVERAGE ELBO of N THREE-HIDDEN-LAYER MLP VAEs (csrc/mlp3_hessian.hip): the f_K of the block above with the two
 * linear maps replaced by the four-Dense relu stacks of networks.py:26-44, Enc and Dec.  The two descriptions are the structs above,
 * unchanged, every field with the same meaning; theta is the flat parameter vector in the library's leaf order (Encoder FC0 kernel [D][h0],
 * bias, .. FC3, Decoder FC0 .. FC3, then p = epsilon_p [L] and, under tunable_eps, c = epsilon [1]).  With N = rows * K columns q = i K + k,
 * c0 = e^{-eps} / N, c1 = 1 / N, sd = e^{p / 2}, w = e^{p}, eps = c * eps_cli:
 *   mu = Enc(x)     s = mu + sd xi     y = Dec(s)     r = y - x
 *   f_K = sum c1 |mu|^2 / 2 + 1/2 sum_l (w_l - 1 - p_l) + 1/2 sum c0 |r|^2 + 1/2 D (eps + log 2 pi)
 * (z2 integrated out as above; with K = 1, xi = z1 and z2 = 0 this is the loss vaek_train_step differentiates).  Per Dense layer i of a
 * stack (W_i [n_in][n_out], b_i; relu after layers 0 .. 2) and a direction (dW_i, db_i):
 *   forward   a_i = h_{i-1} W_i + b_i                     h_i = M_i . a_i        M_i = [a_i > 0]   (no mask on layer 3)
 *   tangent   da_i = dh_{i-1} W_i + h_{i-1} dW_i + db_i   dh_i = M_i . da_i
 *   backward  g_a_i = M_i . g_h_i     g_h_{i-1} = g_a_i W_i^T     df/dW_i = sum h_{i-1}^T g_a_i     df/db_i = sum g_a_i
 *   tangent   dg_a_i = M_i . dg_h_i   dg_h_{i-1} = dg_a_i W_i^T + g_a_i dW_i^T
 *             (Hv)_W_i = sum (dh_{i-1}^T g_a_i + h_{i-1}^T dg_a_i)     (Hv)_b_i = sum dg_a_i
 * (relu has no second derivative away from the kink, so the tangent-backward pass needs the masks only).  The head is the block
 * above's with one decoder: ds = dmu + dp sd xi / 2, g_y = c0 r, dg_y = c0 (dy - deps r), g_mu = g_s + c1 mu, dg_mu = dg_s + c1 dmu with
 * g_s / dg_s what the decoder stack hands back at its input, and the p and c leaves of the gradient and of H v are the formulas above
 * unchanged.  Leaves, rows, samples and directions are widened to float64 once and everything below is float64 on
 * v_mfma_f64_16x16x4_f64: a unit is LIVE iff its FLOAT64 pre-activation is > 0 (the derivative at exactly 0 is 0) -- the float32
 * definition of "live" of vaek_mlp3_decoder_jacobian_replicas does not apply here.  Nothing is finite-differenced.
 * LAUNCHES.  A CHAIN launch, grid (ceil(rows K / 8), n): a workgroup carries 8 columns through both stacks, forward and backward, as a
 * [unit][8 primal | 8 tangent] float64 image and stores every layer's input and masked output gradient to the workspace; a CONTRACTION
 * launch: a workgroup owns 16 x 64 elements of one layer's [kernel | bias] and sums over ALL the replica's columns in column order; one
 * more workgroup a replica adds the per-tile partials of the p and c leaves and of f_K in tile order.  Nothing stored in a launch is read
 * back in it; no atomic, counter, wait or spin.  vaek_mlp3_sampled_elbo_hvp_replicas: the outputs and rules of
 * vaek_sampled_elbo_hvp_replicas; LAUNCHES: 3 + 2 nvec.  vaek_mlp3_sampled_elbo_hessian_lanczos_replicas: the Lanczos run and the
 * 142-double RECORD of vaek_sampled_elbo_hessian_lanczos_replicas slot for slot ([140] K, [141] 0.0), with every length-P vector
 * operation spread over chunks of 2048 elements (grid (ceil(P / 2048), n)) and every dot a per-chunk partial added in chunk order by
 * the next launch; LAUNCHES: 6 + 6 steps, whatever the replicas do (a replica that is done is skipped by the launches that follow).
 * Both calls: rows 1 .. 4096, samples 1 .. 1024, nvec 0 .. 64, steps 1 .. 32, rows * samples <= 2^13 per replica and n * rows * samples
 * <= vaek_mlp3_sampled_elbo_hessian_max_columns() = 2^14 (caps on the length of a launch and on the workspace -- a column costs
 * 2 sum_layers (n_in + n_out) doubles, 51 KB at the widest shape --, not tuned values).  The workspace of
 * vaek_mlp3_sampled_elbo_hessian_workspace_bytes(ctx, n, rows, samples) bytes is the call's own, 16-byte aligned.  The guarantees of the
 * block above hold: replica r BITWISE what n = 1 leaves, two runs bitwise equal, drawing mode bitwise explicit mode, sample 0 of row i
 * vaek_make_batch's z1, nothing depends on ctx.batch, doubles between two replicas' blocks untouched, asynchronous, allocates nothing,
 * capturable.  vaek_supports_mlp3_sampled_elbo_hessian: vaek_supports_mlp3_log_likelihood's predicate.  NOT covered: other depths, two
 * decoders, bf16, D or L > 32, Ritz vectors, more than 32 steps, data parallelism.  VAEK_ERR_INVALID: the list of the block above. */
int vaek_supports_mlp3_sampled_elbo_hessian(const vaek_ctx* ctx, int32_t kind, int32_t* yes);
int vaek_mlp3_sampled_elbo_hessian_max_columns(void);
int vaek_mlp3_sampled_elbo_hessian_workspace_bytes(const vaek_ctx* ctx, int32_t n, int32_t rows, int32_t samples, size_t* bytes);
int vaek_mlp3_sampled_elbo_hvp_replicas(vaek_ctx* ctx, const float* params, const vaek_sampled_elbo_hvp* hp, int32_t kind, const float* A,
                                        int32_t dd, int32_t did, int32_t pad, float var_added, uint32_t x_tag, uint32_t z_tag,
                                        void* workspace, void* stream);
int vaek_mlp3_sampled_elbo_hessian_lanczos_replicas(vaek_ctx* ctx, const float* params, const vaek_sampled_elbo_hessian* hs, int32_t kind,
                                                    const float* A, int32_t dd, int32_t did, int32_t pad, float var_added, uint32_t x_tag,
                                                    uint32_t z_tag, void* workspace, void* stream);
/* DECODER JACOBIAN SPECTRA of N THREE-HIDDEN-LAYER MLP VAEs of the context's shape in one call (csrc/mlp3_jacobian.hip): how many
 * directions of the latent space the decoder moves its output along, row by row.  For a latent row z of replica r
 *   J(z) = d Decoder(z) / dz  (D x L)  = K3^T M3 K2^T M2 K1^T M1 K0^T,   M_i = diag(pre_i(z) > 0),
 * the four decoder kernels with the three relu masks of the primal pass between them (a unit is live iff its float32 pre-activation is
 * > 0; the derivative at exactly 0 is 0, where jax.grad of `maximum` gives 0.5: a difference on a set of measure zero), and
 *   G(z) = J^T J  (L x L, float64 from the float32 J),  lambda_1 >= .. >= lambda_L its eigenvalues = the squared singular values of J.
 * ROW RECORD of vaek_decoder_jacobian_row_record_len = 2 L + 4 doubles (row i of replica r at row_out + r * row_out_stride + i * (2 L
 * + 4), where row_out is given):
 *   [0, L)     lambda, descending (ranked by counting, ties by index; nothing is clamped)
 *   [L, 2 L)   diag G: |d Decoder / d z_l|^2, the sensitivity of the output to latent l
 *   [2 L]      the numerical rank #{k : lambda_k > rank_tol * lambda_1}, 0 where lambda_1 = 0
 *   [2 L + 1]  sweeps of the Jacobi solve,  [2 L + 2] off_F where it stopped,  [2 L + 3] |G|_F.
 * MODEL RECORD of vaek_decoder_jacobian_record_len = 2 L + 8 doubles at out + r * out_stride, written with per-lane vector stores:
 *   [0] rows   [1] mean rank   [2] min rank   [3] max rank   [4] mean |J|_F^2   [5] max sweeps
 *   [6] max off_F / |G|_F (0 where |G|_F = 0)   [7] rank_tol as used
 *   [8, 8 + L)       mean over rows of the k-th largest eigenvalue of J^T J
 *   [8 + L, 8 + 2 L) mean over rows of diag J^T J.
 * Doubles between two records where a stride exceeds the length are not touched; nothing but the records and the workspace is written.
 * Replica r reads params + r * state_stride (vaek_param_count floats; never written; the decoder's leaves only) and its latents:
 *   - EXPLICIT ROWS (z != NULL): from z + r * z_stride as [rows][L] floats (z_stride == 0: one set shared by all replicas); z_seeds,
 *     z_steps and z_tag are not read;
 *   - DRAWING MODE (z == NULL): row i is the z1 that vaek_make_batch writes for row i under (z_seeds[r], step_host = z_steps[r], z_tag),
 *     row0 = 0: Philox blocks q < ceil(L / 4) of the row's latent stream, bit for bit -- sample 0 of the block rule of
 *     vaek_log_likelihood_replicas, the latents sample_batch decodes at a stats event.
 * THREE launches per call whatever n is (profile labels mlp3_jacobian_tangent, mlp3_jacobian_solve, mlp3_jacobian_finalize): a
 * workgroup per tile of 64 / (L + 1) rows carries each row's primal column and its L tangent columns through the four decoder products
 * together (v_mfma_f32_16x16x4_f32, exact f32; the bias on the primal column only, relu and its mask applied to the stored image) and
 * stores J (float32) in the workspace; a workgroup per row forms G in float64 (each entry a sum over d in d order of exact products)
 * and solves it with the cyclic Jacobi of the covariance spectra (stop at off_F <= 2^-43 |G|_F or vaek_cov_spectrum_max_sweeps); n
 * workgroups add the rows in a binary tree per 256 rows, then the tiles in order.  Nothing stored in a launch is read back in it; no
 * atomic, counter, wait or status word.
 * DEFINING PROPERTIES: a column's arithmetic does not depend on its place in a tile, so a row's record depends on its latent's and the
 * parameters' bits only: replica r's records are BITWISE what a call with n = 1 on its slices leaves, two runs are bitwise equal,
 * drawing mode equals explicit mode on the z1 vaek_make_batch writes, and the records do not depend on ctx.batch, state_stride or
 * whether row_out is given.  sum lambda = trace G to 1e-12 relative; G = 0 (a dead decoder, an exact kink) ends at 0 sweeps, rank 0.
 * Away from the kinks (every |pre| above the float32 forward's error) lambda and diag G agree with the float64 evaluation within the
 * float32 error of G plus 64 L 2^-53 |G|_F.  Float32 J does not resolve singular values below about 2^-12 sigma_max in J^T J: choose
 * rank_tol above 2^-24.
 * rows is 1 .. vaek_stats_event_max_rows() = 4096, n 1 .. vaek_train_loop_max_replicas(), and n * rows * L <=
 * vaek_mlp3_decoder_jacobian_max_columns() = 2^20 (a cap that bounds the workspace at 128 MB of J and the length of a call on a shared
 * machine, not a tuned value).  `workspace`: device memory of vaek_mlp3_decoder_jacobian_workspace_bytes(ctx, n, rows) bytes, 16-byte
 * aligned, the call's own, no need to clear; it holds J and the row records.  The weights are read one dword at a time: state_stride
 * has no alignment rule.  Asynchronous on `stream`, allocates nothing, does not synchronise, capturable into a hipGraph.
 * vaek_supports_mlp3_decoder_jacobian: vaek_supports_mlp3_log_likelihood's predicate without the kind (the call draws no data rows):
 * float32, one decoder, exactly three hidden layers of 64 .. 256 units in the encoder and in the decoder, D, L <= 32 -- whatever
 * ctx.batch, world and force_generic are.  NOT covered: other depths, bf16, D or L > 32, two-decoder models, right singular vectors.
 * VAEK_ERR_INVALID (message names vaek_mlp3_decoder_jacobian_replicas, nothing touched): a NULL or unsupported context, NULL params or
 * description, a wrong struct_size, n, rows or n * rows * L out of range, a NULL out, NULL z_seeds or z_steps in drawing mode,
 * state_stride < P, out_stride < 2 L + 8, row_out_stride < rows * (2 L + 4) where row_out is given, z_stride < 0 or 0 < z_stride <
 * rows * L, rank_tol outside [0, 1) or NaN, z_tag >= 2^30, out or row_out not 8-byte aligned, a NULL or misaligned workspace.
 * vaek_mlp3_decoder_jacobian_workspace_bytes refuses an unsupported context and sizes outside those ranges and leaves *bytes alone. */
typedef struct vaek_decoder_jacobian {
    int32_t struct_size;                  /* = sizeof(vaek_decoder_jacobian), ABI guard                 */
    int32_t n;                            /* replicas                                                   */
    int32_t rows;                         /* latent rows, 1 .. vaek_stats_event_max_rows()              */
    int32_t reserved;                     /* 0                                                          */
    int64_t state_stride;                 /* floats between two replicas' params, >= P                  */
    const uint64_t* z_seeds;              /* device [n]: seed of the latents (drawing mode)             */
    const uint32_t* z_steps;              /* device [n]: their RNG step (drawing mode)                  */
    const float* z;                       /* device [rows][L] per replica: explicit rows; NULL = draw   */
    int64_t z_stride;                     /* floats between two replicas' latents; 0 = shared           */
    double rank_tol;                      /* 0 <= rank_tol < 1                                          */
    double* out;                          /* device: model record r at out + r * out_stride             */
    int64_t out_stride;                   /* >= vaek_decoder_jacobian_record_len()                      */
    double* row_out;                      /* device [rows][2 L + 4] per replica, or NULL                */
    int64_t row_out_stride;               /* doubles between two replicas' row blocks                   */
} vaek_decoder_jacobian;
int vaek_supports_mlp3_decoder_jacobian(const vaek_ctx* ctx, int32_t* yes);
int vaek_decoder_jacobian_record_len(const vaek_ctx* ctx, int64_t* doubles);
int vaek_decoder_jacobian_row_record_len(const vaek_ctx* ctx, int64_t* doubles);
int vaek_mlp3_decoder_jacobian_max_columns(void);
int vaek_mlp3_decoder_jacobian_workspace_bytes(const vaek_ctx* ctx, int32_t n, int32_t rows, size_t* bytes);
int vaek_mlp3_decoder_jacobian_replicas(vaek_ctx* ctx, const float* params, const vaek_decoder_jacobian* dj, uint32_t z_tag,
                                        void* workspace, void* stream);
/* DECODER JACOBIAN SPECTRA of N LINEAR VAEs of the context's shape, ONE OR TWO DECODERS, in one call (csrc/linear_jacobian.hip):
 * vaek_mlp3_decoder_jacobian_replicas for the models without hidden layers -- the description struct, the ROW RECORD (2 L + 4 doubles),
 * the MODEL RECORD (2 L + 8 doubles), their two length queries and the two row modes (explicit z; z == NULL: the z1 vaek_make_batch
 * writes under (z_seeds[r], z_steps[r], z_tag), bit for bit) are those of the block above, unchanged.  For networks.py:73-83
 *   x_hat(z) = z K_d + b_d [+ sigmoid(z K_s + b_s)],      J(z) = K_d^T [+ diag(g(u(z))) K_s^T],   u = z K_s + b_s,
 *   g(u) = sigmoid'(u) = e / ((1 + e)(1 + e)),  e = exp(-|u|)
 * (symmetric in u, no 1 - s cancellation, never inf or NaN for a finite u, exactly 0 for a saturated head; the quotient is rounded
 * essentially once, 1 + e and its square carried as pairs of doubles: error well below 1 ulp of exp's e), and G(z) = J^T J with its
 * eigenvalues as above.  With one decoder J is K_d^T at every z: all row records of a replica are bitwise equal and their lambda are
 * the eigenvalues of K^T K in the record of vaek_exact_log_likelihood_replicas (two Jacobi solves apart); z, where given, is checked
 * and not read.  With two decoders J changes from row to row through the D slopes g(u_d).
 * ARITHMETIC: float64 from u onward (J costs one exp per output column, so nothing forces the float32 J of the MLP call):
 * u_d = b_s[d] + sum_l z_l K_s[l][d] in l order, J[l][d] = K_d[l][d] + g_d K_s[l][d], G_ij a sum over d in d order, then the cyclic
 * Jacobi of the covariance spectra (stop at off_F <= 2^-43 |G|_F or vaek_cov_spectrum_max_sweeps), the counting rank and the tails: the
 * text of the MLP call's solve launch (csrc/jacobian_dev.h), instantiated for a float64 J.
 * TWO launches per call whatever n is (profile labels linear_jacobian_rows, linear_jacobian_finalize): a workgroup per (row, replica)
 * does all of the above and stores the row record into the workspace and, where given, row_out; n workgroups add the rows in a binary
 * tree per 256 rows, then the tiles in order -- the MLP call's finalize launch, the same code.  Nothing stored in a launch is read back
 * in it; no atomic, counter, wait or status word.
 * DEFINING PROPERTIES: a row's record depends on its latent's and the parameters' bits only: replica r's records are BITWISE what a
 * call with n = 1 on its slices leaves, two runs are bitwise equal, drawing mode equals explicit mode on the z1 vaek_make_batch writes,
 * and the records do not depend on ctx.batch, state_stride, the number of rows in the call or whether row_out is given.  A two-decoder
 * context with K_s = 0, or with every head saturated (g = 0), leaves bitwise the row records of the one-decoder context holding the same
 * K_d.  Rows l >= k of K_d and K_s exactly zero give diag G[l] = 0.0 exactly and rank <= k; all kernels zero ends at 0 sweeps, rank 0.
 * lambda and diag G agree with the float64 NumPy evaluation (numpy.linalg.eigvalsh) within (2^-43 + 8 x the reference's own error
 * of G against long double + 64 L 2^-53) |G|_F -- measured per case in tests/test_gpu_linear_jacobian.py.
 * rows is 1 .. vaek_stats_event_max_rows() = 4096, n 1 .. vaek_train_loop_max_replicas(), and n * rows <=
 * vaek_linear_decoder_jacobian_max_rows() = 2^20, one workgroup each (a cap on the length of a launch on a shared machine, not a tuned
 * value).  `workspace`: device memory of vaek_linear_decoder_jacobian_workspace_bytes(ctx, n, rows) bytes -- the row records only --,
 * 16-byte aligned, the call's own, no need to clear.  The weights are read one dword at a time: state_stride has no alignment rule.
 * Asynchronous on `stream`, allocates nothing, does not synchronise, capturable into a hipGraph.
 * vaek_supports_linear_decoder_jacobian: vaek_supports_log_likelihood's predicate without the kind (the call draws no data rows):
 * float32, no hidden layers, one or two decoders, D, L <= 32, D <= 28 with two decoders -- whatever ctx.batch, world and force_generic
 * are.  NOT covered: models with hidden layers (vaek_mlp3_decoder_jacobian_replicas has the three-layer ones), bf16, D or L > 32, left
 * or right singular vectors, tangent-space alignment, data parallelism.
 * VAEK_ERR_INVALID (message names vaek_linear_decoder_jacobian_replicas, nothing touched): the list of the block above with n * rows in
 * the place of n * rows * L.  vaek_linear_decoder_jacobian_workspace_bytes refuses an unsupported context and sizes outside those
 * ranges and leaves *bytes alone. */
int vaek_supports_linear_decoder_jacobian(const vaek_ctx* ctx, int32_t* yes);
int vaek_linear_decoder_jacobian_max_rows(void);
int vaek_linear_decoder_jacobian_workspace_bytes(const vaek_ctx* ctx, int32_t n, int32_t rows, size_t* bytes);
int vaek_linear_decoder_jacobian_replicas(vaek_ctx* ctx, const float* params, const vaek_decoder_jacobian* dj, uint32_t z_tag,
                                          void* workspace, void* stream);
/* One train step of N INDEPENDENT three-hidden-layer MLP VAEs of the context's shape (csrc/fused_mlp3.hip, step path "mlp3"): the
 * two launches of that step with gridDim.y = N, blockIdx.y = r training replica r.  A solo step keeps 7 of the MI355X's 256 CUs
 * busy for most of its length (one chain workgroup per 16 batch rows at batch 100); neither launch has a counter, a wait or an
 * atomic, so the idle CUs take other models of a sweep with no new synchronisation.  It is vaek_train_step_gen for N models:
 * replica r trains on its batch x + r * B * D, z1 + r * B * L, z2 + r * B * D ([n][B][D], [n][B][L], [n][B][D] stacks) and draws
 * its next one into the same slices of x_next / z1_next / z2_next, its generator step read from counter[2 r + which] and
 * counter[2 r + (which ^ 1)] = step + 1 stored (int32 [n][2]).  `rep` is the vaek_replicas of vaek_train_loop_gen_replicas:
 * replica r owns params / m / v + r * state_stride, grads + r * grads_stride, step_dev[r], seeds[r], lrs[r] (lrs == NULL: `lr`),
 * A + r * a_stride (0: shared; A may be NULL for kind 2) and the ring loss_hist + r * loss_hist_cap.  kind, dd, did, pad,
 * var_added, row0, tag, which and the context (shape, batch, epsilon) belong to the launch.  Floats between two replicas where
 * a stride exceeds the length are not touched.
 * STRIDE RULE: state_stride must be a multiple of 4 floats.  The step reads a layer's weights 16 bytes at a time where the
 * parameter pointer is 16-byte aligned, and one float at a time where it is not, and the two forms sum in different orders: with
 * that stride every replica's pointer has the base's alignment, so every replica takes the form a solo call on its slice takes.
 * NO-DRAW FORM: x_next == z1_next == z2_next == NULL draws nothing -- N x vaek_train_step; seeds, A and counter may be NULL and
 * kind is ignored.
 * DEFINING PROPERTY: for every r, what the call leaves in replica r's params, m, v, grads, step_dev[r], ring, next batch and
 * counter[2 r .. 2 r + 1] is BITWISE what vaek_train_step_gen (no-draw form: vaek_train_step) leaves when called alone on those
 * slices with seed = seeds[r], lr = lrs[r], replica r's A and counter + 2 r, the ring of vaek_set_loss_history standing in for
 * replica r's: the same code on the same inputs.  The ring of vaek_set_loss_history is NOT written by this call.
 * Asynchronous on `stream`, allocates nothing, does not synchronise, capturable into a hipGraph; two launches per call whatever
 * n is (profile labels fused_mlp3_chain_replicas, fused_mlp3_grads_adam[_gen]_replicas).
 * vaek_supports_train_step_replicas: the step path is "mlp3" and world == 1.  vaek_train_step_max_replicas() = 256: a cap that
 * bounds the length of one launch on a shared machine, not a tuned value; 36 replicas at batch 100 fill the first round of the chain
 * launch (7 workgroups each, one per CU), n above that is legal and only queues workgroups.
 * WORKSPACE: the call's OWN buffer of vaek_train_step_replicas_workspace_bytes(ctx, n) bytes, 16-byte aligned: n times the step's
 * region of stored activations (its float count rounded up to a multiple of 4).  It is NOT the buffer of vaek_workspace_bytes,
 * which this entry point neither needs nor changes.
 * VAEK_ERR_INVALID (with a message, buffers untouched): n < 1 or n > the cap; state_stride < P or not a multiple of 4;
 * grads_stride < grad_len; a ring with loss_hist_cap < 1; a_stride < 0; NULL seeds or NULL counter in the drawing form; some but
 * not all of the _next pointers NULL; dd or did > 16; kind outside 0 .. 2 in the drawing form; a missing or misaligned workspace;
 * a wrong struct_size; a context whose path is not "mlp3", or world > 1.  Data parallelism, gradients-only and the bucketed
 * entry have no replica form. */
int vaek_supports_train_step_replicas(const vaek_ctx* ctx, int32_t* yes);
int vaek_train_step_max_replicas(void);
int vaek_train_step_replicas_workspace_bytes(const vaek_ctx* ctx, int32_t n, size_t* bytes);
int vaek_train_step_gen_replicas(vaek_ctx* ctx, float* params, float* grads, float* m, float* v, int32_t* step_dev,
                                 const vaek_replicas* rep, const float* x, const float* z1, const float* z2, float lr, void* workspace,
                                 int32_t kind, const float* A, int32_t dd, int32_t did, int32_t pad, float var_added, float* x_next,
                                 float* z1_next, float* z2_next, int64_t row0, int32_t* counter, int32_t which, uint32_t tag,
                                 void* stream);
/* Convolutional VAE of BASELINE config 5 -- NO reference counterpart (the reference has no convolutional model: its only image
 * code is utils.py:129-133); the layer is specified in DESIGN.md 3.4 and checked against oracle/conv_vae_oracle.py:conv_fwd.
 * 4 x 4 / stride 2 / pad 1 convolution, NHWC float32 tensors, HWIO kernel [4][4][c_in][c_out], bf16 matrix-core products with
 * float32 accumulation (the envelope of the bf16 Dense path, not the 1e-5 ELBO contract):
 *   y[n, i, j, o] = act(bias[o] + sum_{kh, kw, c} x[n, 2 i + kh - 1, 2 j + kw - 1, c] * w[kh, kw, c, o]),  y: [batch, height/2, width/2, c_out].
 * No context needed.  With the entry points below every product of both layer kinds' forward and backward passes exists
 * (vae_training_amd/conv_vae.py assembles the train step from them).
 * `workspace`: vaek_conv2d_forward_workspace bytes (transposed = 0 / 1 for the two entry points; 0 bytes = none needed), 16-byte
 * aligned, or NULL.  With a workspace, c_in a power of two (>= 8; >= 16 transposed), c_out a multiple of 32 and 16-byte aligned
 * tensors the layer runs on bf16 copies through the LDS-DMA GEMM (the same bf16 products, several times faster); otherwise, and
 * always for NULL, the register-staged kernel.  Layers with ONE channel on the thin side (c_in = 1 here, c_out = 1 transposed)
 * are streaming float32 kernels -- exact, no bf16 rounding.
 * bf16 copies (all optional, NULL = none; 16-byte aligned): `x_bf16` / `dy_bf16` / `y_bf16` INPUTS are bf16 images of the float32
 * tensor of the same name that the caller vouches for (an earlier call's output copy, or vaek_to_bf16) -- the LDS-DMA form then
 * skips its own conversion pass, the other forms ignore them; `y_bf16` / `out_bf16` OUTPUTS are written with the bf16 rounding of
 * the float32 result in every form (from the epilogue where the form can, by a conversion pass otherwise).
 * LEAN forms (round 3: a hidden tensor of the conv VAE lives in HBM as bf16 only; LDS-DMA shapes only, VAEK_ERR_INVALID elsewhere):
 *   - the float32 INPUT (x, y of the transposed call; x / dy of the kernel gradient) may be NULL when its bf16 copy is given;
 *   - the float32 RESULT (y, out) may be NULL when its bf16 copy is asked for -- also on the one-channel forward layer's matrix-core form;
 *   - relu bit 1 (relu = 2 or 3): `mask` points to the bf16 copy of the mask source instead of the float32 tensor
 *     ([mask > 0] is the same set either way: bf16 rounding keeps the sign and never reaches zero from a normal number). */
int vaek_conv2d_forward_workspace(int32_t batch, int32_t height, int32_t width, int32_t c_in, int32_t c_out, int32_t transposed, size_t* bytes);
int vaek_conv2d_forward(const float* x, const float* w, const float* bias, const float* mask, float* y, int32_t batch, int32_t height,
                        int32_t width, int32_t c_in, int32_t c_out, int32_t relu, void* workspace, const void* x_bf16, void* y_bf16,
                        void* stream);   /* mask: as below; NULL = none */
int vaek_to_bf16(const float* src, void* dst_bf16, int64_t n, void* stream);      /* n floats -> n bf16, round to nearest even */
/* The transposed convolution of the same specification = the adjoint of vaek_conv2d_forward with the SAME kernel array
 * (oracle: conv_t_fwd): y [batch, height, width, c_in], w [4][4][c_out][c_in] (the HWIO kernel of the convolution it is the adjoint
 * of), out [batch, 2 height, 2 width, c_out] = act(bias + ...).  It is also the convolution's input gradient (y := dL/d output, bias
 * NULL); `mask` (NULL or a tensor of out's shape) multiplies the result by [mask > 0] -- the relu of the layer below. */
int vaek_conv2d_transpose_forward(const float* y, const float* w, const float* bias, const float* mask, float* out, int32_t batch,
                                  int32_t height, int32_t width, int32_t c_in, int32_t c_out, int32_t relu, void* workspace,
                                  const void* y_bf16, void* out_bf16, void* stream);
/* Kernel gradient of vaek_conv2d_forward (oracle: conv_bwd): dw[kh, kw, c, o] = sum_{n, i, j} x[n, 2 i + kh - 1, 2 j + kw - 1, c] *
 * dy[n, i, j, o], dbias[o] = sum dy (NULL: not wanted); x [batch, height, width, c_in], dy [batch, height/2, width/2, c_out].
 * Batch-split slabs in `workspace` (vaek_conv2d_weight_grad_workspace bytes) + a fixed-order sum: bitwise repeatable.  With
 * (x := dL/d out, dy := the layer's input) it is the TRANSPOSED layer's kernel gradient in its [4][4][c_out][c_in] layout. */
int vaek_conv2d_weight_grad_workspace(int32_t batch, int32_t height, int32_t width, int32_t c_in, int32_t c_out, size_t* bytes);
int vaek_conv2d_weight_grad(const float* x, const float* dy, float* dw, float* dbias, void* workspace, int32_t batch, int32_t height,
                            int32_t width, int32_t c_in, int32_t c_out, const void* x_bf16, const void* dy_bf16, void* stream);
/* dbias[c] = sum over the pixels of dy[pixels][c] (the bias gradient of a transposed layer); workspace: 512 * c floats.
 * _bf16: the same sums (float32 accumulation, fixed order) of a bf16 tensor -- c a power of two in 8 .. 2048, 16-byte aligned. */
int vaek_conv2d_bias_grad(const float* dy, float* dbias, void* workspace, int64_t pixels, int32_t c, void* stream);
int vaek_conv2d_bias_grad_bf16(const void* dy_bf16, float* dbias, void* workspace, int64_t pixels, int32_t c, void* stream);
/* Dense + reparameterisation (networks.py:72-74) as one block: mu = x @ w + b, samples = mu + exp(logvar_e / 2) * z1. */
int vaek_dense_fwd_reparam(vaek_ctx* ctx, const float* x, const float* w, const float* b, float* mu, float* samples, const float* z1,
                           const float* logvar_e, int32_t rows, int32_t n_in, int32_t n_out, void* stream);
/* Backward of the reparameterisation + the KL term's mu and logvar_e parts (what jax.value_and_grad does with networks.py:73-74, 94):
 * in place d_samples -> d_mu = d_samples + mu / batch_total; d_logvar_e[l] = 0.5 exp(lv_l / 2) sum_rows d_samples z1
 * - 0.5 (1 - exp(lv_l)) rows / batch_total.  latent_dim <= 256. */
int vaek_reparam_bwd(vaek_ctx* ctx, float* d_samples, const float* mu, const float* z1, const float* logvar_e, float* d_logvar_e,
                     int32_t rows, int32_t latent_dim, int64_t batch_total, void* workspace, void* stream);
/* n standard normals and/or the raw Philox words they came from (block b = counter (b_lo, b_hi, step, tag)). */
int vaek_rng_fill(vaek_ctx* ctx, float* normals, uint32_t* bits, int64_t n, uint64_t seed, uint32_t step, uint32_t tag,
                  void* stream);
/* Optional device ring buffer: every vaek_train_step also stores its loss at buf[(t - 1) % cap],
 * t = Adam step (what the reference appends to vae_losses, vae.py:130, without a per-step copy). */
int vaek_set_loss_history(vaek_ctx* ctx, float* buf, int64_t cap);

/* ---- roofline denominators measured on the box (bench.py; not on the train-step path) -------------- */
/* float4 stream copy of `bytes` (multiple of 16) src -> dst; time it with vaek_profile_*. */
int vaek_microbench_copy(vaek_ctx* ctx, const void* src, void* dst, int64_t bytes, void* stream);
/* Back-to-back MFMA loop, independent accumulators: kind 0 = v_mfma_f32_16x16x4_f32, 1 =
 * v_mfma_f32_32x32x16_bf16; `waves_per_simd` workgroups of 4 waves per CU.  *flops_out = flops of the launch. */
int vaek_microbench_mfma(vaek_ctx* ctx, int32_t kind, int32_t iters, int32_t waves_per_simd, float* scratch,
                         double* flops_out, void* stream);

/* Launch floor of this platform: n back-to-back launches of a kernel of `blocks` workgroups that does nothing (kind 0)
 * or one dependent pair of loads per thread (kind 1; p = >= 65 small ints, out = >= blocks ints).  Time them with
 * vaek_profile_* (kernel timestamps) or around a hipGraph replay (launch-to-launch interval). */
int vaek_microbench_launch(vaek_ctx* ctx, int32_t kind, int32_t blocks, int32_t n, const int32_t* p, int32_t* out, void* stream);

/* ---- in-process kernel timing (bench.py's roofline leg) --------------------------------------- */
/* Between begin and report every kernel the library launches for this context is bracketed by a
 * pair of hipEvents recorded on the launch stream (pool of max_records pairs, allocated here, so
 * the launch path still allocates nothing).  vaek_profile_report synchronises the events, stops
 * profiling and writes a JSON object {"label": {"count": n, "total_ms": t}, ...} into buf. */
int vaek_profile_begin(vaek_ctx* ctx, int32_t max_records);
int vaek_profile_report(vaek_ctx* ctx, char* buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* VAEK_H */
