// N consecutive train steps of a LINEAR VAE (encoder = one Dense D -> L, decoder = one Dense L -> D: every "" layer-size
// experiment of seed_linpadding_expts.sh, the configuration the headline metric is quoted on), software-pipelined over
// launches: vaek_train_steps (include/vaek.h).  Same function as N calls of VAE.train_step (networks.py:87-101: forward,
// ELBO, value_and_grad, Adam), evaluated through its sufficient statistic.
//
// Why this is exact.  With no non-linearity between input and loss, every per-sample quantity is LINEAR in
//     u_b = [z1_b (L) | x_b (D) | z2_b (D) | 1]                                   (NF = L + 2 D + 1 features):
//     mu_b = E u_b,        E = [0 | We^T | 0 | be]                                  (networks.py:67-68)
//     samples_b = S u_b,   S = E + [diag(e^{lv/2}) | 0 | 0 | 0]                     (networks.py:73-74)
//     r_b = x_hat_b - x_b = R u_b,   R = [Wd^T diag(e^{lv/2}) | Wd^T We^T - I | e^{eps/2} I | Wd^T be + bd]   (:80-83)
// and the loss and every gradient of SURVEY.md 8(a) row a5 are quadratic in u_b summed over the batch, i.e. functions of
//     M = sum_b u_b u_b^T                                                           (NF x NF, parameter-INDEPENDENT)
// and of the parameters alone:  sum_b |r_b|^2 = tr(R M R^T),  sum_b |mu_b|^2 = tr(E M E^T),  dWd = c0 S M R^T,
// [dWe | dbe] = columns of c0 Wd R M + E M / B,  d lv_l = 1/2 e^{lv_l/2} c0 (Wd R M)[l, z1_l] - 1/2 (1 - e^{lv_l}),
// d eps = (-1/2 tr(RMR^T) e^{-eps} + 1/2 B D + 1/2 e^{-eps/2} sum_d (R M)[d, z2_d]) / B,  c0 = e^{-eps} / B.
//
// What it buys.  The streaming pass over the batch (11.5 MB at the metric's size, the whole algorithmic traffic) no longer
// depends on the parameters, so nothing couples the 256 workgroups of a step to the previous step's all-reduce -> Adam ->
// broadcast: the two-kernel step (fused_mfma.hip + fused_finalize) spends most of its 13 us waiting on exactly that chain.
// Here launch n carries three roles at once (the persistent form below: wave-specialised streamers, the updater on the float64
// matrix cores -- DESIGN.md 3.0):
//     streamers   (one per 256-sample tile)  batch n:   x, z1, z2 tiles land in LDS by global_load_lds, then
//                 M_tile = U^T U on v_mfma_f32_16x16x4_f32 (exact f32 fmaf chains; upper block triangle only) -> one
//                 partial image per workgroup.  No weights, no elementwise pass, no transposition (the k axis of the MFMA
//                 is the sample axis and any sample order will do: operands are read straight from the row-major images).
//     reducers    batch n-1: fixed-order float64 sum of the partial images -> M.
//     updater     (one workgroup) batch n-2: the small dense algebra above in float64, the closed-form KL terms, the three
//                 loss means, Adam (flax.optim.Adam.apply_gradient, networks.py:100), the step counter, the loss ring.
// In that launch-per-step form stream order is the only synchronisation.  The PERSISTENT form (default where it applies) runs
// up to 64 steps in ONE launch with the same three roles as resident workgroups: streamers walk the batches with the tile of
// batch n + 1 / n + 2 in flight while batch n is multiplied, reducers and the updater follow behind through per-batch arrival
// counters (write-through partial images, one counter add per workgroup, relaxed polls: cdna guide G16 R1).  Every batch of
// the launch has its OWN partial / M slot, so a streamer never waits for anybody: nothing can dead-lock, whatever the
// dispatcher does with residency, and every poll is bounded (status word, vaek_train_steps_status).  What it buys on top:
// no launch boundary and no cold start per step (the updater's instruction stream and parameters stay on one CU).
// A call of more than 64 steps is several such launches, CHAINED: launch j streams batches [64 j, 64 j + 64), but reduces
// [64 j - 1, 64 j + 63) and updates [64 j - 4, 64 j + 60) -- the launch-per-step form's shift, widened to kLinCarry = 4 for the
// updater, across the launch boundary -- and the call's last launch runs every role to the end (lin_windows).  A later launch's
// reducers and updater so start on batches that are complete (ordered by the stream) while its streamers fill their pipeline,
// and the three roles end together instead of the streamers idling through the drain.  Batch n of a call lives in slot n % 68 of
// the workspace (64 + the four carried: partial images, M, arrival counters -- 68 x ntiles x 6 KB of images, 95.3 MB at the
// metric's 228 tiles); a slot comes round again 68 batches later, when its batch was updated at least a whole launch ago, so
// still nobody waits for a slot.
//
// Numerics: M accumulates exact-f32 products in chains of 72 samples (one multiplying wave's 18 MFMA k-steps at the metric's
// 288-row tile; 36 in the launch-per-step form), summed further in
// float64; everything downstream is float64 until the final rounding of each gradient to float32.  Against the float64
// oracle the loss sits at ~1e-7 relative (tests/test_gpu_steps.py), like the sample-by-sample kernels -- but it is a
// different summation order, so this path is NOT bitwise comparable with vaek_train_step.
#include <stdlib.h>

#include "linear_moments_dev.h"

namespace vaek {

// zeroes the arrival counters of a workspace (once per workspace: afterwards every launch leaves them zero) and, unless the
// workspace carries the mark of an earlier initialisation, the sticky status word
constexpr unsigned kLinMagic = 0x4c494e33u;
__global__ void lin_init_kernel(unsigned* cnt, int n_words, unsigned* status) {
    for (int k = threadIdx.x; k < n_words; k += blockDim.x) cnt[k] = 0u;
    if (threadIdx.x == 0 && status[1] != kLinMagic) { status[0] = 0u; status[1] = kLinMagic; }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
constexpr size_t kLinMaxLds = 160 * 1024;
// workspace: [cnt_stream: kLinSlots (68) batches x 8 shards x 128 B][cnt_reduce: 68 words][status word, init mark][68 M slots][68 partial
// image slots] -- the metric's shape: 68 x 228 images of 6 KB = 95.3 MB
constexpr size_t kLinCntStreamBytes = (size_t)kLinSlots * kLinShards * kLinShardStride * 4, kLinCntBytes = kLinCntStreamBytes + 1024, kLinHeadBytes = kLinCntBytes + 256;
static_assert(kLinSlots * sizeof(unsigned) <= 1024, "cnt_reduce");

LinPlan lin_plan(const vaek_ctx* c) {
    LinPlan p{};
    const int D = c->D, L = c->L;
    p.ok = c->cfg.n_enc_hidden == 0 && c->cfg.n_dec_hidden == 0 && !c->cfg.sigmoid_decoder && c->cfg.dtype == VAEK_F32 &&
           L + 2 * D + 1 <= 64 && (long long)c->B * std::min(D, L) >= 8;
    if (!p.ok) return p;
    // 16-feature blocks of the kernel instantiation that serves this model: 3 (up to 48 features: the metric's 45) or 4
    p.NB = (L + 2 * D + 1 + 15) / 16 <= 3 ? 3 : 4;
    p.NO = p.NB * (p.NB + 1) / 2 * 256;
    // a tile slot doubles as the combine's cross-wave scratch; a persistent streamer's LDS: three slots, the two validity columns,
    // the zero word, the batch pointer tables
    const auto slot_bytes = [&](int T) { return std::max((size_t)LinTile(D, L, T).bytes, (size_t)lin_scratch_bytes(p.NB)); };
    const auto ring_slot_bytes = [&](int T) { return std::max((size_t)LinTile(D, L, T).bytes, (size_t)lin_ring_scratch_bytes(p.NB)); };
    const auto ring_bytes = [&](int T) { return 3 * ring_slot_bytes(T) + 8 * (size_t)T + 16 + 3 * kLinMaxPersist * sizeof(void*) + 64; };
    const auto ksteps_ok = [&](int T) { return (LinTile(D, L, T).np + LNW - kLinCW - 1) / (LNW - kLinCW) <= 18; };
    // Samples per tile.  256, unless a slightly taller tile lets every streamer of the persistent launch take exactly ONE tile per
    // batch (the metric: 65 536 samples = 228 tiles of 288 on the 231 CUs the updater and the reducers leave).
    const int smax = c->n_cu - 1 - kLinReduceSets * kLinReduceWgs;
    const bool upd_ok = p.NB == 3 ? LinUpdM<3, 0, 0>::shape_ok(D, L) : LinUpdM<4, 0, 0>::shape_ok(D, L);
    p.T = 256;
    if (p.NB == 3) {
        if (smax >= 16 && c->B > 256 * smax) {
            const int T = 32 * (int)(((long long)c->B + 32ll * smax - 1) / (32ll * smax));
            if (T <= 512 && ksteps_ok(T) && ring_bytes(T) <= kLinMaxLds) p.T = T;
        }
    } else if (upd_ok && smax >= 16) {
        // Four blocks: rows of up to 252 bytes, and three slots of 256 of them are over the LDS.  The tallest tile whose ring fits
        // (D = 20, L = 20: 192 rows) -- the fewest partial images, and a batch of up to T rows (run.py's 100) is one tile; the
        // streamers then take ceil(tiles / streamers) tiles each (the metric's size: 342 tiles of 192, two on each of 171 CUs).
        int T = 256;
        while (T > 32 && !(ksteps_ok(T) && ring_bytes(T) <= kLinMaxLds)) T -= 32;
        p.T = T;
    }
    p.ntiles = (c->B + p.T - 1) / p.T;
    // launch-per-step form: one slot + validity column + zero word | updater | reducer sums
    const size_t upd = std::max(p.NB == 3 ? LinUpd<3, 0, 0>::lds_bytes(D, L) : LinUpd<4, 0, 0>::lds_bytes(D, L),
                                p.NB == 3 ? LinUpdM<3, 0, 0>::lds_bytes(D, L, (int)c->P) : LinUpdM<4, 0, 0>::lds_bytes(D, L, (int)c->P));
    p.lds_step = std::max(slot_bytes(p.T) + 4 * (size_t)p.T + 16, std::max(upd, (size_t)2 * 16 * 32 * sizeof(double))) + 64;
    // The persistent form gives every workgroup a CU of its own (the updater's float64 chains and the streamers' MFMA loops both
    // lose a factor ~2 when they share one): each workgroup asks for more than half a CU's LDS -- the streamers need it anyway for
    // their ring of tile slots -- and the grid stays within the CU count.
    p.lds_persist = std::max(std::max(p.lds_step, ring_bytes(p.T)), (size_t)82 * 1024);
    p.persist = upd_ok && p.lds_persist <= kLinMaxLds && ksteps_ok(p.T) && smax >= 16;
    if (p.persist) {      // streamers: the CUs the updater and the reducers leave, tiles dealt evenly
        const int per = (p.ntiles + smax - 1) / smax;
        p.n_stream = (p.ntiles + per - 1) / per;
        p.n_reduce = kLinReduceSets * std::min(kLinReduceWgs, p.NO / 32);
    }
    // the metric's shape with its dimensions (and the k-steps per wave of its 288-row tile) at compile time, and M20's (D = 20,
    // L = 20, 192-row tile); every other linear model on the run-time instantiations of its block count
    p.which_persist = p.NB == 3 ? (D == 12 && L == 20 && p.T == 288 ? 0 : 1) : (D == 20 && L == 20 && p.T == 192 ? 3 : 2);
    p.which_step = D == 12 && L == 20 ? 2 : p.NB - 3;
    const int slots = p.persist ? kLinSlots : 2;
    p.M_off = kLinHeadBytes;
    p.partial_off = p.M_off + (size_t)slots * p.NO * sizeof(double) + 256;
    p.ws_bytes = (p.partial_off + (size_t)slots * p.ntiles * p.NO * sizeof(float) + 256 + 255) / 256 * 256;
    if (c->cfg.world > 1 && p.persist) p.comm_bytes = (size_t)kLinCommBanks * c->cfg.world * 2 * p.NO * sizeof(unsigned long long);
    return p;
}

// data parallel: the persistent form only, and only once the P2P communicator (vaek_comm_create / _init) carries the moment region
bool lin_steps_supported(const vaek_ctx* c) {
    return c->lin.ok && (c->cfg.world == 1 || (c->lin.persist && c->comm.ready && c->comm.lin_bytes > 0));
}
// the in-launch batch generator serves the datasets a linear VAE can be trained on (the sigmoid dataset brings a second decoder)
bool lin_steps_gen_supported(const vaek_ctx* c, int kind) { return lin_steps_supported(c) && c->lin.persist && (kind == 0 || kind == 2); }

struct LinWs { float* partial; double* M; unsigned* cnt; unsigned* cnt_reduce; unsigned* status; };
static LinWs lin_ws(const vaek_ctx* c, void* ws) {
    char* base = static_cast<char*>(ws) + c->ws_lin;
    LinWs w;
    w.cnt = reinterpret_cast<unsigned*>(base); w.cnt_reduce = reinterpret_cast<unsigned*>(base + kLinCntStreamBytes);
    w.status = reinterpret_cast<unsigned*>(base + kLinCntBytes);
    w.M = reinterpret_cast<double*>(base + c->lin.M_off); w.partial = reinterpret_cast<float*>(base + c->lin.partial_off);
    return w;
}

// The kernels by LinPlan::which_persist / which_step, each given the LDS cap (not a request) the first time it is launched on a
// device.  The device code lists the instantiations in the order these tables name them.
typedef void (*LinStepKernel)(const LinArgs);
static const LinPersistKernel kLinPersist[] = {lin_persist_kernel<3, 12, 20, 18, false>, lin_persist_kernel<3, 0, 0, 0, false>,
                                                lin_persist_four(0), lin_persist_four(1)};
static const LinPersistGenKernel kLinPersistGen[] = {lin_persist_kernel<3, 12, 20, 18, true>, lin_persist_kernel<3, 0, 0, 0, true>,
                                                     lin_persist_four_gen(0), lin_persist_four_gen(1)};
static const LinStepKernel kLinStep[] = {lin_step_kernel<3, 0, 0>, lin_step_kernel<4, 0, 0>, lin_step_kernel<3, 12, 20>};
template <typename K, size_t N> static int lin_kernel(const K (&table)[N], int which, K* fn) {
    static thread_local PerDeviceOnce attr_set[N];
    VAEK_HIP_CHECK(set_max_dynamic_lds(attr_set[which], table[which], kLinMaxLds));
    *fn = table[which];
    return VAEK_OK;
}

static void lin_fill_common(const vaek_ctx* c, LinArgs& a, float* params, float* grads, float* m, float* v, int32_t* step_dev, float lr) {
    a.B = c->B; a.D = c->D; a.L = c->L; a.T = c->lin.T; a.ntiles = c->lin.ntiles;
    a.params = params; a.grads = grads; a.m = m; a.v = v; a.step_dev = step_dev; a.lr = lr;
    // data parallel: M is summed over the ranks before the updater sees it, so its "rows" are the GLOBAL batch
    const double rows = c->cfg.world > 1 ? (double)c->Bt : (double)c->B;
    a.inv_bt = (float)(1.0 / (double)c->Bt); a.eps_cli = c->cfg.eps_cli; a.rows = (float)rows;
    a.rows_over_bt = (float)(rows / (double)c->Bt); a.off_eps = (int)c->off_eps; a.P = (int)c->P;
    a.comm = LinComm{};
    a.comm.world = 1;
    if (c->cfg.world > 1 && c->comm.ready && c->comm.lin_bytes > 0) {
        a.comm.world = c->cfg.world; a.comm.rank = c->cfg.rank; a.comm.ng2 = 2 * c->lin.NO;
        for (int r = 0; r < c->cfg.world; ++r)
            a.comm.peer[r] = reinterpret_cast<unsigned long long*>(static_cast<char*>(c->comm.peers[r]) + c->comm.lin_off);
    }
    a.loss_hist = c->loss_hist; a.loss_hist_cap = c->loss_hist_cap;
    static const int stagger = getenv("VAEK_LIN_STAGGER") ? atoi(getenv("VAEK_LIN_STAGGER")) : 3;      // diagnostic override
    a.stagger = stagger;
}

// The arrival counters start from zero (every persistent launch leaves them zero again): zeroed once per (context, workspace) by a
// launch that has run in stream order.  A launch recorded into a graph being captured has not, and may never run.
static int lin_ensure_init(vaek_ctx* c, const LinWs& w, void* ws, hipStream_t st) {
    if (c->lin_ws_ready == ws) return VAEK_OK;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    VAEK_HIP_CHECK(hipStreamIsCapturing(st, &cap));
    hipLaunchKernelGGL(lin_init_kernel, dim3(1), dim3(1024), 0, st, w.cnt, (int)(kLinCntBytes / 4), w.status);
    VAEK_HIP_CHECK(hipGetLastError());
    c->lin_ws_issued = ws;
    c->lin_ws_ready = cap == hipStreamCaptureStatusNone ? ws : nullptr;
    return VAEK_OK;
}

// gen != nullptr: the batches are drawn inside the launch (xs / z1s / z2s unused)
static int lin_train_steps_impl(vaek_ctx* c, float* params, float* grads, float* m, float* v, int32_t* step_dev, const float* const* xs,
                                const float* const* z1s, const float* const* z2s, const BatchArgs* gen, int n_steps, float lr, void* ws, hipStream_t st) {
    const LinPlan& p = c->lin;
    const LinWs w = lin_ws(c, ws);
    static const char* env = getenv("VAEK_LIN_PERSIST");              // diagnostic: 0 forces the launch-per-step form
    static const int roles = getenv("VAEK_LIN_ROLES") ? atoi(getenv("VAEK_LIN_ROLES")) : 7;   // diagnostic: 1 stream, 2 reduce, 4 update
    const bool persistent = p.persist && (gen || c->cfg.world > 1 || !(env && atoi(env) == 0));   // data parallel, in-launch draw: persistent form only
    if (gen && !persistent) { set_error("vaek_train_steps_gen: this context has no persistent form"); return VAEK_ERR_INVALID; }
    if (persistent) {
        LinPersistKernel fn = nullptr;
        LinPersistGenKernel fng = nullptr;
        if (int rc = gen ? lin_kernel(kLinPersistGen, p.which_persist, &fng) : lin_kernel(kLinPersist, p.which_persist, &fn)) return rc;
        if (int rc = lin_ensure_init(c, w, ws, st)) return rc;
        for (int j = 0; j < lin_launches(n_steps); ++j) {
            // launch j streams its 64 batches, reduces from the batch the launch before left it, updates from the two it was left
            const LinWindows win = lin_windows(n_steps, j);
            const int s0 = win.stream.first, n = win.stream.count;
            LinArgs a{};
            lin_fill_common(c, a, params, grads, m, v, step_dev, lr);
            a.persistent = 1; a.n_steps = win.update.count; a.n_red = win.reduce.count; a.n_str = n;
            a.slot_upd = win.update.first % kLinSlots; a.slot_red = win.reduce.first % kLinSlots; a.slot_str = s0 % kLinSlots;
            a.d_red = win.reduce.first - win.update.first; a.d_str = s0 - win.update.first;
            a.sets = kLinReduceSets;
            a.has_update = 1; a.n_reduce = p.n_reduce; a.n_stream = p.n_stream;
            if (!(roles & 4)) a.has_update = 0;
            if (!(roles & 2)) { a.has_update = 0; a.n_reduce = 0; }
            if (!(roles & 1)) a.n_stream = 0;
            if (roles != 7) c->lin_ws_ready = nullptr;        // nobody re-zeroes the counters without the updater: start over next call
            a.partial_base = w.partial; a.M_base = w.M;
            a.cnt_stream = w.cnt; a.cnt_reduce = w.cnt_reduce; a.status = w.status;
            const dim3 grid((unsigned)(a.has_update + a.n_reduce + a.n_stream));
            if (gen) {
                ProfScope ps("lin_moments_persistent_gen", st);
                launch_k(ps, fng, grid, dim3(LNT), p.lds_persist, st, a, *gen);
            } else {
                LinPtrs ptrs{};
                for (int i = 0; i < n; ++i) { ptrs.x[i] = xs[s0 + i]; ptrs.z1[i] = z1s[s0 + i]; ptrs.z2[i] = z2s[s0 + i]; }
                ProfScope ps("lin_moments_persistent", st);
                launch_k(ps, fn, grid, dim3(LNT), p.lds_persist, st, a, ptrs);
            }
        }
        VAEK_HIP_CHECK(hipGetLastError());
        return VAEK_OK;
    }
    LinStepKernel fn = nullptr;
    if (int rc = lin_kernel(kLinStep, p.which_step, &fn)) return rc;
    const size_t pstride = (size_t)p.ntiles * p.NO;
    for (int n = 0; n < n_steps + 2; ++n) {       // launch n: stream batch n, reduce batch n - 1, update batch n - 2
        LinArgs a{};
        lin_fill_common(c, a, params, grads, m, v, step_dev, lr);
        a.has_update = (n >= 2 && (roles & 4)) ? 1 : 0;
        a.n_reduce = (n >= 1 && n <= n_steps && (roles & 2)) ? p.NO / 32 : 0;
        a.n_stream = (n < n_steps && (roles & 1)) ? p.ntiles : 0;
        if (a.has_update + a.n_reduce + a.n_stream == 0) continue;
        if (a.n_stream) { a.x = xs[n]; a.z1 = z1s[n]; a.z2 = z2s[n]; a.partial_out = w.partial + (n & 1) * pstride; }
        if (a.n_reduce) { a.partial_in = w.partial + ((n - 1) & 1) * pstride; a.M_out = w.M + ((n - 1) & 1) * p.NO; }
        a.M_in = w.M + (n & 1) * p.NO;             // (n - 2) & 1
        ProfScope ps(a.n_stream ? "lin_moments_step" : "lin_moments_drain", st);
        launch_k(ps, fn, dim3((unsigned)(a.has_update + a.n_reduce + a.n_stream)), dim3(LNT), p.lds_step, st, a);
    }
    VAEK_HIP_CHECK(hipGetLastError());
    return VAEK_OK;
}

int lin_train_steps(vaek_ctx* c, float* params, float* grads, float* m, float* v, int32_t* step_dev, const float* const* xs,
                    const float* const* z1s, const float* const* z2s, int n_steps, float lr, void* ws, hipStream_t st) {
    return lin_train_steps_impl(c, params, grads, m, v, step_dev, xs, z1s, z2s, nullptr, n_steps, lr, ws, st);
}
int lin_train_steps_gen(vaek_ctx* c, float* params, float* grads, float* m, float* v, int32_t* step_dev, const BatchArgs& gen, int n_steps,
                        float lr, void* ws, hipStream_t st) {
    return lin_train_steps_impl(c, params, grads, m, v, step_dev, nullptr, nullptr, nullptr, &gen, n_steps, lr, ws, st);
}

// ---- the two halves of ONE step of the launch-per-step form, for a host-side collective between them ------------------------------
// Data parallel without the P2P communicator (GradExchange mode "rccl"): the moment matrix is additive over the ranks' shards
// (the loss is a batch mean, networks.py:97-98), so a rank forms the M of its shard (lin_moments: streamers, then reducers, two
// launches ordered by the stream), torch.distributed sums the 12 KB float64 image over the ranks (RCCL; gloo in rehearsal -- every
// rank receives the same bits), and every rank applies the identical update (lin_update: rows = the GLOBAL batch).
int lin_moments(vaek_ctx* c, const float* x, const float* z1, const float* z2, double* M_out, void* ws, hipStream_t st) {
    const LinPlan& p = c->lin;
    LinStepKernel fn = nullptr;
    if (int rc = lin_kernel(kLinStep, p.which_step, &fn)) return rc;
    LinArgs a{};
    lin_fill_common(c, a, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f);
    a.n_stream = p.ntiles; a.x = x; a.z1 = z1; a.z2 = z2; a.partial_out = lin_ws(c, ws).partial;
    { ProfScope ps("lin_moments_stream", st); launch_k(ps, fn, dim3((unsigned)p.ntiles), dim3(LNT), p.lds_step, st, a); }
    a.n_stream = 0; a.n_reduce = p.NO / 32; a.partial_in = a.partial_out; a.M_out = M_out;
    a.comm = LinComm{}; a.comm.world = 1;                      // the ranks meet on the host, not in the reducers
    { ProfScope ps("lin_moments_reduce", st); launch_k(ps, fn, dim3((unsigned)a.n_reduce), dim3(LNT), p.lds_step, st, a); }
    VAEK_HIP_CHECK(hipGetLastError());
    return VAEK_OK;
}
int lin_update(vaek_ctx* c, float* params, float* grads, float* m, float* v, int32_t* step_dev, const double* M_in, float lr, hipStream_t st) {
    LinStepKernel fn = nullptr;
    if (int rc = lin_kernel(kLinStep, c->lin.which_step, &fn)) return rc;
    LinArgs a{};
    lin_fill_common(c, a, params, grads, m, v, step_dev, lr);
    a.has_update = 1; a.M_in = M_in;
    ProfScope ps("lin_moments_update", st);
    launch_k(ps, fn, dim3(1), dim3(LNT), c->lin.lds_step, st, a);
    VAEK_HIP_CHECK(hipGetLastError());
    return VAEK_OK;
}

// synchronous: did a bounded wait of the persistent form ever give up (a workgroup that never became resident, a lost store)?
// The word is STICKY -- no launch clears it, and while it is set every wait of every later launch returns at once (the grid
// drains, its results are garbage) -- until this call reads it: read-and-clear.
int lin_steps_status(vaek_ctx* c, void* ws, int* gave_up) {
    *gave_up = 0;
    if (c->lin_ws_issued != ws) return VAEK_OK;            // no persistent launch has been issued on this workspace yet
    const LinWs w = lin_ws(c, ws);
    unsigned s = 0;
    VAEK_HIP_CHECK(hipMemcpy(&s, w.status, sizeof(s), hipMemcpyDeviceToHost));
    *gave_up = (int)s;
    if (s) {
        VAEK_HIP_CHECK(hipMemset(w.status, 0, sizeof(unsigned)));
        c->lin_ws_ready = nullptr;                         // the counters of the launch that gave up are in an unknown state
    }
    return VAEK_OK;
}

// ---- diagnostic: the streamer and reducer roles of ONE persistent launch, every batch's M copied out ------------------------------
// What VAEK_LIN_ROLES=3 runs (has_update = 0, the windows of a single-launch call), with the batches' M slots copied to the caller
// in stream order.  Nobody re-zeroes the arrival counters without the updater: lin_ws_ready is dropped, the next call starts over.
static int lin_debug_moments(vaek_ctx* c, const float* const* xs, const float* const* z1s, const float* const* z2s, int n, int32_t* step_dev,
                             double* M_out, void* ws, hipStream_t st) {
    const LinPlan& p = c->lin;
    const LinWs w = lin_ws(c, ws);
    LinPersistKernel fn = nullptr;
    if (int rc = lin_kernel(kLinPersist, p.which_persist, &fn)) return rc;
    if (int rc = lin_ensure_init(c, w, ws, st)) return rc;
    const LinWindows win = lin_windows(n, 0);
    LinArgs a{};
    lin_fill_common(c, a, nullptr, nullptr, nullptr, nullptr, step_dev, 0.f);
    a.persistent = 1; a.n_steps = 0; a.n_red = win.reduce.count; a.n_str = win.stream.count;
    a.slot_upd = 0; a.slot_red = 0; a.slot_str = 0; a.d_red = 0; a.d_str = 0;
    a.sets = kLinReduceSets;
    a.has_update = 0; a.n_reduce = p.n_reduce; a.n_stream = p.n_stream;
    a.comm = LinComm{}; a.comm.world = 1;                      // one rank's own batches
    c->lin_ws_ready = nullptr;
    a.partial_base = w.partial; a.M_base = w.M;
    a.cnt_stream = w.cnt; a.cnt_reduce = w.cnt_reduce; a.status = w.status;
    LinPtrs ptrs{};
    for (int i = 0; i < n; ++i) { ptrs.x[i] = xs[i]; ptrs.z1[i] = z1s[i]; ptrs.z2[i] = z2s[i]; }
    {
        ProfScope ps("lin_moments_persistent", st);
        launch_k(ps, fn, dim3((unsigned)(a.n_reduce + a.n_stream)), dim3(LNT), p.lds_persist, st, a, ptrs);
    }
    VAEK_HIP_CHECK(hipGetLastError());
    VAEK_HIP_CHECK(hipMemcpyAsync(M_out, w.M, (size_t)n * p.NO * sizeof(double), hipMemcpyDeviceToDevice, st));      // batch i lives in slot i
    return VAEK_OK;
}

}  // namespace vaek

// Diagnostic entry (not part of include/vaek.h; tests/test_gpu_lin_moments.py).  op 0: the context's LinPlan into args->plan -- ok,
// NB, NO, T, ntiles, persist, which_step, which_persist, n_stream, n_reduce.  op 1: n <= 64 batches (host arrays of device pointers,
// as vaek_train_steps takes them) through the streamers and reducers of one persistent launch; M_out [n][NO] receives every batch's
// moment image.  step_dev: a device int32 the reducers read (the tag of the data-parallel exchange, unused here), left as it is.
// VAEK_ERR_INVALID where the context has no persistent form; the give-up word is vaek_train_steps_status's.
struct vaek_lin_debug_args {
    int32_t plan[10];
    int32_t n, reserved;
    const float* const* xs; const float* const* z1s; const float* const* z2s;
    int32_t* step_dev;
    double* M_out;
};
extern "C" int vaek_debug_lin(vaek_ctx* ctx, int32_t op, vaek_lin_debug_args* args, void* workspace, void* stream) {
    using namespace vaek;
    if (!ctx || !args) { set_error("vaek_debug_lin: null argument"); return VAEK_ERR_INVALID; }
    const LinPlan& p = ctx->lin;
    if (op == 0) {
        const int v[10] = {p.ok ? 1 : 0, p.NB, p.NO, p.T, p.ntiles, p.persist ? 1 : 0, p.which_step, p.which_persist, p.n_stream, p.n_reduce};
        for (int k = 0; k < 10; ++k) args->plan[k] = v[k];
        return VAEK_OK;
    }
    if (op != 1) { set_error("vaek_debug_lin: unknown op"); return VAEK_ERR_INVALID; }
    if (!p.ok || !p.persist || ctx->cfg.world != 1) { set_error("vaek_debug_lin: this context has no single-GPU persistent form"); return VAEK_ERR_INVALID; }
    if (args->n < 1 || args->n > kLinMaxPersist) { set_error("vaek_debug_lin: 1 <= n <= %d", kLinMaxPersist); return VAEK_ERR_INVALID; }
    if (!args->xs || !args->z1s || !args->z2s || !args->step_dev || !args->M_out) { set_error("vaek_debug_lin: null argument"); return VAEK_ERR_INVALID; }
    if (reinterpret_cast<uintptr_t>(args->M_out) & 7) { set_error("vaek_debug_lin: M_out must be 8-byte aligned"); return VAEK_ERR_INVALID; }
    for (int i = 0; i < args->n; ++i) {
        const float *x = args->xs[i], *z1 = args->z1s[i], *z2 = args->z2s[i];
        if (!x || !z1 || !z2 || ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(z1) | reinterpret_cast<uintptr_t>(z2)) & 15)) {
            set_error("vaek_debug_lin: batch %d has a null or not 16-byte aligned pointer", i);
            return VAEK_ERR_INVALID;
        }
    }
    if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 255)) {
        set_error("vaek_debug_lin: workspace must be a non-null, 256-byte aligned device pointer of vaek_workspace_bytes() bytes");
        return VAEK_ERR_WORKSPACE;
    }
    ProfBind pb(ctx);
    return lin_debug_moments(ctx, args->xs, args->z1s, args->z2s, args->n, args->step_dev, args->M_out, workspace, (hipStream_t)stream);
}

#ifdef VAEK_LIN_STAMPS
extern "C" int vaek_debug_lin_stamps(unsigned long long* buf) {
    return hipMemcpyToSymbol(HIP_SYMBOL(vaek::g_lin_stamp_buf), &buf, sizeof(buf)) == hipSuccess ? vaek::lin_stamps_four(buf) : -2;
}
#endif
