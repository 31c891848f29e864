// Resident train loop of a small-batch linear VAE (vaek_train_loop_gen): N train steps as a plain loop inside ONE workgroup.
//
// At the reference's batch size (run.py:14, 100 rows) the whole batch is one workgroup's tile -- the SINGLE form of
// fused_mfma.hip, one launch per step.  What that launch pays every step besides its chain is the launch-to-launch interval
// and a cold read of parameters, m and v from HBM plus their write back.  Here the step is the body of a loop:
//
//   - parameters, m and v are read from HBM ONCE per launch and written once, at its end; in between every thread keeps its
//     idx = t + 256 k slice in registers (the pk / mk / vk of the SINGLE tail), and the weights the chain needs are read from
//     an LDS image of the parameter vector that the Adam update refreshes;
//   - the batch of every step is drawn in the kernel by the work items of rng_dev.h (the very function vaek_make_batch's
//     kernel runs, so the values are the same bits), into an LDS image where the variant's T image leaves room for it and
//     into the caller's workspace where it does not;
//   - there is one workgroup: no arrival counter, no spin, no grid barrier, no atomic.  Nothing here can wait for ever.
//
// The chain (transposed operand layout, T image, ones rows, masking of rows past the batch) and the tail (closed-form KL /
// log-variance terms, the three means, Adam, the loss ring) are those of fused_linear_mfma_kernel<.., SINGLE>: the same text,
// included into both (mfma_chain_dev.h lists the pieces, and the pieces carry the comments).
//
// WHAT A LOOP AROUND THAT KERNEL'S BODY MUST NOT DO.  The single-step kernel reads `params` through a const __restrict__
// pointer and, in the loss slots, through uniform addresses: loads the compiler may serve from the scalar cache, which never
// sees this kernel's own vector stores.  The rule of this file: nothing stored inside the launch is read back inside it
// through a const __restrict__ pointer or a uniform-address global load.  Everything carried from step to step lives in
// registers (pk / mk / vk) or LDS (the parameter image); params / m / v / *step_dev are loaded before the loop and stored
// after it; grads and the ring are stored only.  The one thing read back from global memory is a batch staged in the
// workspace: per-lane addresses (vector loads) through plain pointers, behind __threadfence_block() + __syncthreads().
//
// THE REPLICA FORM (vaek_train_loop_gen_replicas).  Because the loop has no cross-workgroup state, N independent models of one
// shape are N workgroups of one launch: workgroup r runs this very loop on replica r's slices of the caller's buffers, with its
// own seed, learning rate, dataset matrix, loss ring and (where the batch is staged in memory) stage region.  The rule above is
// kept: the per-replica tables are never written by the launch, and step_dev[r] is read before the loop and stored after it.
#include "mfma_chain_dev.h"
#include "rng_dev.h"
#include "vaek_internal.h"

namespace vaek {

constexpr int kResidentMaxSteps = 1024;      // steps per launch: bounds a launch to milliseconds on a shared machine while the
                                             // launch boundary stays under 1 % of it -- a cap, not a tuned value

struct ResidentArgs {
    float* params; float* grads; float* m; float* v; int32_t* step_dev;
    float* stage;                  // the batch image in the workspace; nullptr: it fits LDS behind the parameter image
    int B, D, L, P, off_epsp, off_eps, n_steps;
    float inv_bt, eps_cli, lr, rows_over_bt, rows;
    float* loss_hist; long long loss_hist_cap;
    BatchArgs gen;                 // x / z1 / z2 are set by the kernel
};

// floats of a staged batch: [x | z2 | z1], every section padded to whole float4s so that the generator's and the chain's
// 16-byte accesses stay aligned for any B, D, L
__host__ __device__ inline int stage_sec(int n) { return (n + 3) & ~3; }
__host__ __device__ inline int stage_floats(int B, int D, int L) { return 2 * stage_sec(B * D) + stage_sec(B * L); }

template <int DP, int LP, bool SIG>
struct RGeom {
    using G = MGeom<DP, LP, SIG>;
    static constexpr int T_ALLOC = (G::LDS_FLOATS + 3) & ~3;      // the T / R image of the chain
    static constexpr int P_ALLOC = (G::PMAX + 3) & ~3;              // the parameter image behind it
    static constexpr int BASE_FLOATS = T_ALLOC + P_ALLOC;         // ... and behind that the batch image, where it fits
};

// What the replica form adds to ResidentArgs (vaek_train_loop_gen_replicas): workgroup r trains replica r.  The tables are never
// written by the launch, so the uniform-address (scalar) loads of seeds[r] / lrs[r] below keep the rule of this file.
struct ReplicaArgs {
    long long state_stride, grads_stride, a_stride, stage_stride;      // floats between two replicas' params / m / v, grads, A, stage
    const unsigned long long* seeds;                                   // [n]
    const float* lrs;                                                  // [n], or nullptr: ResidentArgs::lr for every replica
};

// Replica r's launch arguments: its slices of the caller's buffers, its seed, its learning rate.  Every replica's slice is disjoint
// from every other's (the host checks the strides against the lengths), and a workgroup reads and writes only its own.
__device__ __forceinline__ const ResidentArgs& replica_slice(const ResidentArgs& a) { return a; }       // the grid-1 form: as given
__device__ __forceinline__ ResidentArgs replica_slice(const ResidentArgs& a0, const ReplicaArgs& rp) {
    const long long r = blockIdx.x;
    ResidentArgs a = a0;
    a.params += r * rp.state_stride; a.m += r * rp.state_stride; a.v += r * rp.state_stride;
    a.grads += r * rp.grads_stride;
    a.step_dev += r;
    if (a.stage) a.stage += r * rp.stage_stride;
    if (a.loss_hist) a.loss_hist += r * a.loss_hist_cap;
    if (a.gen.A) a.gen.A += r * rp.a_stride;
    a.gen.seed = rp.seeds[r];
    if (rp.lrs) a.lr = rp.lrs[r];
    return a;
}

// THE TRAJECTORY RING (vaek_train_loop_gen_traj / vaek_train_loop_gen_replicas_traj).  A TrajArgs at the end of the pack makes the
// traced form: at every Adam step t with t % every == 0 the workgroup stores one record of 2 P + 4 floats -- [0, P) the parameters
// step t's gradient was evaluated at (pk before adam_apply_f), [P, 2 P + 4) the step's gradient buffer exactly as `grads` would
// hold it (gk, loss slots included) -- to slot (t / every - 1) % cap of its ring.  Both are in this thread's registers at that
// point: the record is per-lane vector stores and nothing else.  The rule above is kept: the ring is stored only, never read.
// Without a TrajArgs in the pack TrajOff is what the body sees and `if constexpr` removes every line of it: the untraced kernels
// are the text they were.
struct TrajOff { static constexpr bool on = false; };
struct TrajRing {
    static constexpr bool on = true;
    float* buf; int every; long long cap, record_stride;
    // where step `tstep`'s record goes, or nullptr where the step is not recorded (tstep > 0: a slot is never negative)
    __device__ __forceinline__ float* record(int tstep) const {
        if (tstep <= 0 || tstep % every != 0) return nullptr;
        return buf + (long long)(tstep / every - 1) % cap * record_stride;
    }
};
__device__ __forceinline__ TrajOff traj_ring() { return {}; }
__device__ __forceinline__ TrajOff traj_ring(const ReplicaArgs&) { return {}; }
__device__ __forceinline__ TrajRing traj_ring(const TrajArgs& tj) { return {tj.buf, tj.every, tj.cap, tj.record_stride}; }
__device__ __forceinline__ TrajRing traj_ring(const ReplicaArgs&, const TrajArgs& tj) {
    return {tj.buf + (long long)blockIdx.x * tj.replica_stride, tj.every, tj.cap, tj.record_stride};
}
__device__ __forceinline__ const ResidentArgs& replica_slice(const ResidentArgs& a, const TrajArgs&) { return a; }
__device__ __forceinline__ ResidentArgs replica_slice(const ResidentArgs& a0, const ReplicaArgs& rp, const TrajArgs&) { return replica_slice(a0, rp); }

// RP is empty (vaek_train_loop_gen: one model, grid 1) or ReplicaArgs (vaek_train_loop_gen_replicas: N independent models of one
// shape, workgroup r training replica r), each with or without a trailing TrajArgs.  The body has no cross-workgroup state -- no
// counter, no wait, no atomic -- so the replicas share nothing but the code and the launch-wide arguments.
template <int DP, int LP, bool SIG, bool EXACT, typename... RP>
__global__ __launch_bounds__(256) void linear_resident_kernel(const ResidentArgs a0, const RP... rp) {
    const ResidentArgs& a = replica_slice(a0, rp...);
    [[maybe_unused]] const auto traj = traj_ring(rp...);
    using TR = decltype(traj_ring(rp...));
    using G = MGeom<DP, LP, SIG>;
    using RG = RGeom<DP, LP, SIG>;
    using AD = typename G::AD;
    using AL = typename G::AL;
    constexpr int NDB = AD::NB, NLB = AL::NB, NSUB = G::NSUB, NOUT = G::NOUT;
    extern __shared__ __attribute__((aligned(16))) float T[];
    float* const Pimg = T + RG::T_ALLOC;
    float* const pother = Pimg;      // mfma_chain_grad.inc
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int j = lane & 15, g = lane >> 4;           // B/C layout: sample column j, row group g
    const int ai = lane & 15, akg = lane >> 4;        // A layout: output row ai, k group akg
    const int D = EXACT ? DP : a.D, L = EXACT ? LP : a.L;
    const int off_be = D * L, off_wd = off_be + L, off_bd = off_wd + L * D, off_ws = off_bd + D, off_bs = off_ws + L * D;
    const int off_epsp = SIG ? off_bs + D : off_ws;
    const bool vecD = D % 4 == 0, vecL = L % 4 == 0;

    // ---- the batch image and the generator that fills it ---------------------------------------------
    float* const stage = a.stage ? a.stage : Pimg + RG::P_ALLOC;
    BatchArgs gen = a.gen;
    gen.x = stage; gen.z2 = stage + stage_sec(a.B * D); gen.z1 = stage + 2 * stage_sec(a.B * D);
    const int nitems = (int)make_batch_item_count(gen);      // <= 256 rows x 24 pieces: int, so that the items' divisions are 32-bit

#include "mfma_chain_srcoff.inc"

    // ---- the launch's ONE read of parameters, moments and step counter ----------------------------------
    float pk[NOUT], mk[NOUT], vk[NOUT];
#pragma unroll
    for (int k = 0; k < NOUT; ++k) {
        const int idx = t + 256 * k;
        pk[k] = 0.f; mk[k] = 0.f; vk[k] = 0.f;
        if (idx < a.P) { pk[k] = a.params[idx]; mk[k] = a.m[idx]; vk[k] = a.v[idx]; Pimg[idx] = pk[k]; }
    }
    const int t0 = a.step_dev[0];
    __syncthreads();

#define VAEK_MSTAMP(i) do {} while (0)      // mfma_chain_tile.inc's phase stamps: the fused kernel's diagnostic build only
    for (int it = 0; it < a.n_steps; ++it) {
        // ---- draw this step's batch: the RNG step is the Adam counter BEFORE the update, as vaek_make_batch(step_dev) -------
        const unsigned gstep = (unsigned)(t0 + it);
        for (int item = t; item < nitems; item += 256) make_batch_items(gen, gstep, item);
        __threadfence_block();
        __syncthreads();

        // ---- inputs of this wave's 64 samples in accumulator layout (clamped rows / columns, masked downstream) ------------
        float xv[NSUB][NDB][4], z2v[NSUB][NDB][4], z1v[NSUB][NLB][4];
        bool valid[NSUB];
        {
            const float* px[NSUB]; const float* pz2[NSUB]; const float* pz1[NSUB];
#pragma unroll
            for (int s = 0; s < NSUB; ++s) {
                const int b = wave * 64 + s * 16 + j;
                valid[s] = b < a.B;
                const int bc = valid[s] ? b : a.B - 1;
                px[s] = gen.x + bc * D; pz2[s] = gen.z2 + bc * D; pz1[s] = gen.z1 + bc * L;
            }
#pragma unroll
            for (int s = 0; s < NSUB; ++s)
#pragma unroll
                for (int db = 0; db < NDB; ++db) {
                    if (AD::full(db) && vecD) {
                        VAEK_LOAD_BLOCK_VEC(AD, xv[s][db], px[s], db, D);
                        VAEK_LOAD_BLOCK_VEC(AD, z2v[s][db], pz2[s], db, D);
                    } else {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            VAEK_LOAD_BLOCK_ELT(AD, xv[s][db], px[s], db, D, r);
                            VAEK_LOAD_BLOCK_ELT(AD, z2v[s][db], pz2[s], db, D, r);
                        }
                    }
                }
#pragma unroll
            for (int s = 0; s < NSUB; ++s)
#pragma unroll
                for (int lb = 0; lb < NLB; ++lb) VAEK_LOAD_BLOCK(AL, z1v[s][lb], pz1[s], lb, L, vecL);
        }

        // ---- weights as MFMA A operands and per-lane constants, from the parameter image -----------------------
#define VAEK_W(dst, idx, ok) dst = (ok) ? Pimg[idx] : 0.f
#define VAEK_WSD(dst, idx, ok) dst = (ok) ? expf(0.5f * Pimg[idx]) : 0.f                /* e^{lv/2}, networks.py:73 */
#include "mfma_chain_operands.inc"
#undef VAEK_W
#undef VAEK_WSD
        const float eps = a.off_eps >= 0 ? Pimg[a.off_eps] * a.eps_cli : a.eps_cli;
        const float inv_var = expf(-eps), sigma = expf(0.5f * eps);
        const float dscale = inv_var * a.inv_bt;
        // the ones rows: T doubles as the reduction image R at the end of every step, so they are written again
        if (G::ONE1) T[(G::FS + LP) * G::TS + t] = 1.f;          // each wave reads back only its own 64 columns
        if (G::ONE2) T[(G::FX + DP) * G::TS + t] = 1.f;

#include "mfma_chain_zero.inc"

#include "mfma_chain_tile.inc"

        // ---- column sums over the 16 lanes of a row, cross-wave sum through LDS ------------------------------------------
#include "mfma_chain_reduce.inc"

        // ---- the SINGLE tail: closed-form KL / log-variance terms, the three means, Adam, the loss ring -----------------------
        // Parameters come from pk (this thread's own) and the LDS image (the others'); all reads of the image come before the
        // barrier, the Adam update's writes to it after.
        const int tstep = t0 + it + 1;
        const float s_mse_t = fetch_cs(G::NCS + 0), s_musq_t = fetch_cs(G::NCS + 1), s_deps_t = fetch_cs(G::NCS + 2);
        float gk[NOUT];
#pragma unroll
        for (int k = 0; k < NOUT; ++k) {
            const int idx = t + 256 * k;
            gk[k] = 0.f;
            if (idx >= a.P + kExtra) continue;
            float gq_ = batch_sum_k(k);
#include "mfma_chain_grad.inc"
            gk[k] = gq_;
        }
        __syncthreads();
        const float bc1 = -expm1f((float)tstep * -0.10536051565782628f);
        const float bc2 = -expm1f((float)tstep * -0.0010005003335835335f);
        const bool last = it + 1 == a.n_steps;      // only the launch's last gradient is anybody's to read
        if constexpr (TR::on) {
            // the trajectory record of this step: theta BEFORE the update and the gradient evaluated at it, from registers
            if (float* const rec = traj.record(tstep)) {
#pragma unroll
                for (int k = 0; k < NOUT; ++k) {
                    const int idx = t + 256 * k;
                    if (idx < a.P) rec[idx] = pk[k];
                    if (idx < a.P + kExtra) rec[a.P + idx] = gk[k];
                }
            }
        }
#pragma unroll
        for (int k = 0; k < NOUT; ++k) {
            const int idx = t + 256 * k;
            if (idx >= a.P + kExtra) continue;
            if (last) a.grads[idx] = gk[k];
            if (idx == a.P && a.loss_hist) a.loss_hist[(long long)(tstep - 1) % a.loss_hist_cap] = gk[k];
            if (idx < a.P) {
                adam_apply_f(pk[k], gk[k], mk[k], vk[k], a.lr, bc1, bc2);
                Pimg[idx] = pk[k];
            }
        }
        __syncthreads();       // the next step reads the refreshed image, and rewrites T, only after every thread is here
    }

    // ---- the launch's ONE write of parameters, moments and step counter -----------------------------------
#pragma unroll
    for (int k = 0; k < NOUT; ++k) {
        const int idx = t + 256 * k;
        if (idx < a.P) { a.params[idx] = pk[k]; a.m[idx] = mk[k]; a.v[idx] = vk[k]; }
    }
    if (t == 0) a.step_dev[0] = t0 + a.n_steps;
}

// ---- variant table: the shapes of fused_mfma.hip -----------------------------------------------------
typedef void (*ResidentKernel)(const ResidentArgs);
typedef void (*ResidentReplicasKernel)(const ResidentArgs, const ReplicaArgs);
typedef void (*ResidentTrajKernel)(const ResidentArgs, const TrajArgs);
typedef void (*ResidentReplicasTrajKernel)(const ResidentArgs, const ReplicaArgs, const TrajArgs);
struct ResidentVariant {
    int dp, lp, sig, exact; ResidentKernel fn; size_t base_bytes; ResidentReplicasKernel fn_replicas;
    ResidentTrajKernel fn_traj; ResidentReplicasTrajKernel fn_replicas_traj;
};
#define VAEK_RESIDENT_ROW(DP, LP, SIG, EXACT) \
    {DP, LP, SIG, EXACT, linear_resident_kernel<DP, LP, (SIG) != 0, (EXACT) != 0>, sizeof(float) * RGeom<DP, LP, (SIG) != 0>::BASE_FLOATS, \
     linear_resident_kernel<DP, LP, (SIG) != 0, (EXACT) != 0, ReplicaArgs>, linear_resident_kernel<DP, LP, (SIG) != 0, (EXACT) != 0, TrajArgs>, \
     linear_resident_kernel<DP, LP, (SIG) != 0, (EXACT) != 0, ReplicaArgs, TrajArgs>},
static const ResidentVariant kResidentVariants[] = {VAEK_MFMA_SHAPES(VAEK_RESIDENT_ROW)};
#undef VAEK_RESIDENT_ROW
// every row can be picked: its operand and parameter images fit the LDS of a CU (pick_shape skips a row that does not)
#define VAEK_RESIDENT_FITS(DP, LP, SIG, EXACT) \
    static_assert(sizeof(float) * RGeom<DP, LP, (SIG) != 0>::BASE_FLOATS <= kLdsLimit, "a resident variant no context can take");
VAEK_MFMA_SHAPES(VAEK_RESIDENT_FITS)
#undef VAEK_RESIDENT_FITS

static const ResidentVariant* pick_resident(const vaek_ctx* c) { return pick_shape(kResidentVariants, c, &ResidentVariant::base_bytes); }

// THE predicate of vaek_train_loop_gen (vaek_ctx_create evaluates it once, into ctx->resident)
bool resident_supported(const vaek_ctx* c) {
    const vaek_config& cfg = c->cfg;
    return cfg.dtype == VAEK_F32 && cfg.n_enc_hidden == 0 && cfg.n_dec_hidden == 0 && cfg.world == 1 && !cfg.force_generic &&
           c->B >= 1 && c->B <= 256 && fused_mfma_supported(c) && pick_resident(c) != nullptr;
}

static size_t stage_bytes(const vaek_ctx* c) { return sizeof(float) * (size_t)stage_floats(c->B, c->D, c->L); }
static bool stage_in_lds(const vaek_ctx* c, const ResidentVariant* v) { return v->base_bytes + stage_bytes(c) <= kLdsLimit; }

// the region at ws_resident: a batch image, where the variant's LDS has no room for one
size_t resident_workspace_bytes(const vaek_ctx* c) {
    if (!resident_supported(c)) return 0;
    return stage_in_lds(c, pick_resident(c)) ? 0 : stage_bytes(c);
}

int resident_steps_per_launch() { return kResidentMaxSteps; }

// What every form does before its launches: pick the variant, size its LDS (raising the kernel's limit the first time a device sees
// it), and fill the launch arguments.  ws + ws_offset: where the batch image goes if LDS has no room for it.
struct ResidentLaunch { const ResidentVariant* var; size_t lds; ResidentArgs a; };
static int resident_setup(vaek_ctx* c, bool replicas, const TrajArgs* traj, float* params, float* grads, float* m, float* v, int32_t* step_dev,
                          float* loss_hist, long long loss_hist_cap, void* ws, size_t ws_offset, const BatchArgs& gen, float lr, ResidentLaunch& rl) {
    const ResidentVariant* var = rl.var = c->resident ? pick_resident(c) : nullptr;
    if (!var) { set_error("resident train loop not available for this configuration"); return VAEK_ERR_INVALID; }
    const bool in_lds = stage_in_lds(c, var);
    rl.lds = var->base_bytes + (in_lds ? stage_bytes(c) : 0);
    const int form = (replicas ? 2 : 0) + (traj ? 1 : 0);
    const void* const fns[4] = {(const void*)var->fn, (const void*)var->fn_traj, (const void*)var->fn_replicas, (const void*)var->fn_replicas_traj};
    static thread_local PerDeviceOnce attr_set[4][sizeof(kResidentVariants) / sizeof(kResidentVariants[0])];      // [form]: four kernels
    if (rl.lds > 64 * 1024)      // the most this variant ever asks for (the batch image grows with the batch, which another context may have larger)
        VAEK_HIP_CHECK(set_max_dynamic_lds(attr_set[form][var - kResidentVariants], fns[form], kLdsLimit));
    ResidentArgs& a = rl.a = ResidentArgs{};
    a.params = params; a.grads = grads; a.m = m; a.v = v; a.step_dev = step_dev;
    a.loss_hist = loss_hist; a.loss_hist_cap = loss_hist_cap;
    a.stage = in_lds ? nullptr : reinterpret_cast<float*>(static_cast<char*>(ws) + ws_offset);
    a.B = c->B; a.D = c->D; a.L = c->L; a.P = (int)c->P; a.off_epsp = (int)c->off_epsp; a.off_eps = (int)c->off_eps;
    a.inv_bt = (float)(1.0 / (double)c->Bt); a.eps_cli = c->cfg.eps_cli; a.lr = lr;
    a.rows_over_bt = (float)((double)c->B / (double)c->Bt); a.rows = (float)c->B;
    a.gen = gen;
    return VAEK_OK;
}

// ---- the replica form: vaek_train_loop_gen_replicas -------------------------------------------------------------------------
// 1024 replicas = 4 rounds of 256 workgroups on the MI355X's 256 CUs: a cap that bounds the length of one launch on a shared
// machine, not a tuned value.  More replicas than CUs is legal: the workgroups are independent, the extra ones queue.
constexpr int kResidentMaxReplicas = 1024;
int resident_max_replicas() { return kResidentMaxReplicas; }

// bytes of the replica call's OWN workspace (not a region of vaek_workspace_bytes): one batch image per replica where the variant
// stages the batch in memory, nothing where it fits LDS.  stage_floats is a multiple of 4, so every replica's image keeps the
// 16-byte alignment of the base.
size_t resident_replicas_workspace_bytes(const vaek_ctx* c, int n) { return (size_t)n * resident_workspace_bytes(c); }

// All four forms.  rep == nullptr: one model on the context's workspace region and ring; else rep->n of them, one workgroup each, on
// the caller's rings and the call's own workspace, never the context's.
int resident_train_loop(vaek_ctx* c, float* params, float* grads, float* m, float* v, int32_t* step_dev, const BatchArgs& gen,
                        int n_steps, float lr, void* ws, hipStream_t st, const vaek_replicas* rep, const TrajArgs* traj) {
    ResidentLaunch rl;
    if (int rc = resident_setup(c, rep != nullptr, traj, params, grads, m, v, step_dev, rep ? rep->loss_hist : c->loss_hist,
                                !rep ? c->loss_hist_cap : rep->loss_hist ? rep->loss_hist_cap : 0, ws, rep ? 0 : c->ws_resident, gen, lr, rl)) return rc;
    ResidentArgs& a = rl.a;
    ReplicaArgs rp{};
    if (rep) {
        rp.state_stride = rep->state_stride; rp.grads_stride = rep->grads_stride; rp.a_stride = rep->a_stride;
        rp.stage_stride = stage_floats(c->B, c->D, c->L);
        rp.seeds = reinterpret_cast<const unsigned long long*>(rep->seeds); rp.lrs = rep->lrs;
    }
    const dim3 grid(rep ? (unsigned)rep->n : 1u), block(256);
    // every launch leaves params / m / v / grads / *step_dev / the ring in HBM: the next one starts from memory alone
    for (int left = n_steps; left > 0; left -= kResidentMaxSteps) {
        a.n_steps = left < kResidentMaxSteps ? left : kResidentMaxSteps;
        // the traced launch finds the slot of every record from the step counter it reads itself: nothing to carry between launches
        ProfScope ps(rep ? (traj ? "linear_resident_replicas_traj" : "linear_resident_replicas") : traj ? "linear_resident_traj" : "linear_resident", st);
        if (rep && traj) launch_k(ps, rl.var->fn_replicas_traj, grid, block, rl.lds, st, a, rp, *traj);
        else if (rep) launch_k(ps, rl.var->fn_replicas, grid, block, rl.lds, st, a, rp);
        else if (traj) launch_k(ps, rl.var->fn_traj, grid, block, rl.lds, st, a, *traj);
        else launch_k(ps, rl.var->fn, grid, block, rl.lds, st, a);
        VAEK_HIP_CHECK(hipGetLastError());
    }
    return VAEK_OK;
}

}  // namespace vaek
