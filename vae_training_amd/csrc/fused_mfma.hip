// Fused linear-VAE train step, matrix-core formulation (the metric's kernel).
//
// Same contract as fused_linear_kernel (fused_small.hip): x, z1, z2 read from HBM exactly once, one
// partial gradient row per workgroup, no atomics.  What changes is WHERE the 1 200 FMAs per sample run.
// The VALU formulation needs every weight as a per-lane register operand: 532 dwords LDS->VGPR per lane
// and step, which at one wave per SIMD (B = 65 536 -> 256 samples per CU) makes the kernel LDS-bound.
// Here the whole forward/backward chain runs on v_mfma_f32_16x16x4_f32 (exact f32 fmaf chains) in the
// TRANSPOSED orientation -- features on the MFMA rows, 16 samples on the columns:
//
//     muT [L x16] = We^T [L xD] . xT [D x16]        A = weights (a few VGPRs per lane, loaded once),
//     yT  [D x16] = Wd^T [D xL] . samplesT [L x16]   B = the previous product's ACCUMULATOR registers:
//     gT  [L x16] = Wd   [L xD] . dyT [D x16]        lane (sample j, group g) register r of a 16-row block
//                                                     is exactly the B operand of k-step r, so products
//                                                     chain with no LDS, no shuffles, no re-layout.
//
// Row numbering inside a 16-row block is chosen per block: a FULL block uses feature = 16b + 4g + r (each
// lane's 4 registers are 4 consecutive features -> float4 loads of z1); a PARTIAL block uses
// 16b + 4r + g, which packs `rem` features into ceil(rem/4) registers = ceil(rem/4) k-steps (L = 20:
// block 1 costs 1 step, not 4; D = 12: 3 steps).  Elementwise work (reparameterisation, residual, dy,
// dmu, loss terms) happens in that accumulator layout, one sample per lane-column.
//
// The batch-reduction GEMMs samples^T dy and x^T dmu need the sample index on the K axis instead, i.e. a
// transpose: each lane drops its 16 values per 16-sample sub-tile into the feature-major LDS image
// T[feature][sample] (row stride = 2 mod 32 banks) and the wave reads its own 64 columns back as MFMA
// operands.  Bias / epsilon_p gradients are column sums: accumulated per lane, reduced over the 16
// lanes of a row with DPP-class shuffles once per kernel.
#include "comm_dev.h"
#include "mfma_chain_dev.h"
#include "rng_dev.h"
#include "vaek_internal.h"

namespace vaek {

#ifdef VAEK_STAMPS
#define VAEK_MSTAMP(i)                                                                       \
    do {                                                                                     \
        __builtin_amdgcn_sched_barrier(0);                                                   \
        unsigned long long _t;                                                               \
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(_t)::"memory"); \
        if (a.stamps && (threadIdx.x & 63) == 0) a.stamps[((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 8 + (i)] = _t; \
        __builtin_amdgcn_sched_barrier(0);                                                   \
    } while (0)
#else
#define VAEK_MSTAMP(i) do {} while (0)
#endif

// SINGLE: the one-workgroup (batch <= 256 rows) form that finalizes itself -- a separate instantiation, so that the
// metric's multi-workgroup kernel is compiled exactly as if this form did not exist (folded into one kernel behind a
// runtime flag it cost that kernel 0.35 us per launch).
template <int DP, int LP, bool SIG, bool EXACT, bool SINGLE>
__global__ __launch_bounds__(256) void fused_linear_mfma_kernel(const float* __restrict__ params, const FusedArgs a) {
    if (SINGLE && blockIdx.x > 0) {      // single-launch step with a batch to draw: workgroups 1.. are K7's work items
        const unsigned gstep = make_batch_step(a.gen);
        make_batch_items(a.gen, gstep, (long long)(blockIdx.x - 1) * 256 + threadIdx.x);
        make_batch_advance(a.gen, gstep, blockIdx.x == 1 && threadIdx.x == 0);
        return;
    }
    using G = MGeom<DP, LP, SIG>;
    using AD = typename G::AD;
    using AL = typename G::AL;
    constexpr int NDB = AD::NB, NLB = AL::NB, NSUB = G::NSUB, NOUT = G::NOUT;
    extern __shared__ __attribute__((aligned(16))) float T[];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int j = lane & 15, g = lane >> 4;           // B/C layout: sample column j, row group g
    const int ai = lane & 15, akg = lane >> 4;        // A layout: output row ai, k group akg
    const int D = EXACT ? DP : a.D, L = EXACT ? LP : a.L;      // EXACT: every bound below folds at compile time
    const int off_be = D * L, off_wd = off_be + L, off_bd = off_wd + L * D, off_ws = off_bd + D, off_bs = off_ws + L * D;
    const int off_epsp = SIG ? off_bs + D : off_ws;
    const bool vecD = D % 4 == 0, vecL = L % 4 == 0;

    // ---- inputs of this wave's 64 samples, in accumulator layout, straight from HBM ----------------
    float xv[NSUB][NDB][4], z2v[NSUB][NDB][4], z1v[NSUB][NLB][4];
    bool valid[NSUB];
    // Every load is UNCONDITIONAL, from a clamped row and column, and nothing is zeroed afterwards (VAEK_LOAD_BLOCK).
    auto load_inputs = [&](int tile, int what = 3) {
        const float* px[NSUB]; const float* pz2[NSUB]; const float* pz1[NSUB];
#pragma unroll
        for (int s = 0; s < NSUB; ++s) {
            const long long b = (long long)tile * G::TILE + wave * 64 + s * 16 + j;
            valid[s] = b < a.B;
            const long long bc = valid[s] ? b : (long long)a.B - 1;
            px[s] = a.x + bc * D; pz2[s] = a.z2 + bc * D; pz1[s] = a.z1 + bc * L;
        }
        // Issue order = order of first use: x of all four sub-tiles (the mu products can start when a quarter of the
        // tile's bytes have landed), then z1 (reparameterisation), then z2 (residual) -- loads return in order.
        if (what & 1)
#pragma unroll
        for (int s = 0; s < NSUB; ++s)
#pragma unroll
            for (int db = 0; db < NDB; ++db) VAEK_LOAD_BLOCK(AD, xv[s][db], px[s], db, D, vecD);
        if (what & 2)
#pragma unroll
        for (int s = 0; s < NSUB; ++s)
#pragma unroll
            for (int lb = 0; lb < NLB; ++lb) VAEK_LOAD_BLOCK(AL, z1v[s][lb], pz1[s], lb, L, vecL);
        if (what & 2)
#pragma unroll
        for (int s = 0; s < NSUB; ++s)
#pragma unroll
            for (int db = 0; db < NDB; ++db) VAEK_LOAD_BLOCK(AD, z2v[s][db], pz2[s], db, D, vecD);
    };
#if defined(VAEK_ABLATE) && VAEK_ABLATE == 2   // diagnostic (tools/ablate.sh): the same bytes as wide, fully coalesced 16-byte loads
    {
        const long long s0 = (long long)blockIdx.x * G::TILE + wave * 64;      // this wave's first sample
        const float4* px = reinterpret_cast<const float4*>(a.x + s0 * D);
        const float4* pz2 = reinterpret_cast<const float4*>(a.z2 + s0 * D);
        const float4* pz1 = reinterpret_cast<const float4*>(a.z1 + s0 * L);
        float sink = 0.f;
        for (int i = lane; i < 64 * D / 4; i += 64) { const float4 u = px[i], w2 = pz2[i]; sink += u.x + u.y + u.z + u.w + w2.x + w2.y + w2.z + w2.w; }
        for (int i = lane; i < 64 * L / 4; i += 64) { const float4 u = pz1[i]; sink += u.x + u.y + u.z + u.w; }
        sink += params[t % a.P];
        float* outp = a.partials + (long long)blockIdx.x * a.pstride;
        for (int idx = t; idx < a.P + kExtra; idx += 256) outp[idx] = sink;
        if (blockIdx.x == 0 && t == 0 && a.step_dev) a.step_dev[0] += 1;
        return;
    }
#endif
    load_inputs(blockIdx.x, 1);
    __builtin_amdgcn_sched_barrier(0);

    // ---- weights as MFMA A operands and per-lane constants ------------------------------------------
    // Like the inputs, every parameter load is unconditional (index 0 where the operand is padding) and the zeroing
    // selects come AFTER the input loads have been issued: a select inside the load sequence is an s_waitcnt there.
#define VAEK_W(dst, idx, ok) dst = params[(ok) ? (idx) : 0]
#define VAEK_WSD(dst, idx, ok) VAEK_W(dst, idx, ok)      /* logvar_e now, e^{lv/2} below */
#include "mfma_chain_operands.inc"
#undef VAEK_W
#undef VAEK_WSD
    const float eps_raw = a.off_eps >= 0 ? params[a.off_eps] : 0.f;

    // z1 / z2 AFTER the weights (loads return in order, and the first product needs the weights and x only); x went out
    // before the ~150 VALU of parameter indexing
    load_inputs(blockIdx.x, 2);
    if (G::ONE1) T[(G::FS + LP) * G::TS + t] = 1.f;          // each wave reads back only its own 64 columns: no barrier needed
    if (G::ONE2) T[(G::FX + DP) * G::TS + t] = 1.f;
#include "mfma_chain_srcoff.inc"
    __builtin_amdgcn_sched_barrier(0);        // nothing that WAITS for a parameter may be scheduled above the input loads

#pragma unroll
    for (int lb = 0; lb < NLB; ++lb)
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const bool ok = w_ok1(lb, db, s), ok2 = w_ok2(db, lb, s);
                wmu[lb][db][s] = ok ? wmu[lb][db][s] : 0.f; wg[lb][db][s] = ok ? wg[lb][db][s] : 0.f;
                wy[db][lb][s] = ok2 ? wy[db][lb][s] : 0.f;
                if (SIG) { wgs[lb][db][s] = ok ? wgs[lb][db][s] : 0.f; wys[db][lb][s] = ok2 ? wys[db][lb][s] : 0.f; }
            }
#pragma unroll
    for (int lb = 0; lb < NLB; ++lb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool ok = r < AL::nreg(lb) && AL::feat(lb, g, r) < L;
            c_be[lb][r] = ok ? c_be[lb][r] : 0.f;
            c_sd[lb][r] = ok ? expf(0.5f * c_sd[lb][r]) : 0.f;                // e^{lv/2}, networks.py:73
        }
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool ok = r < AD::nreg(db) && AD::feat(db, g, r) < D;
            c_bd[db][r] = ok ? c_bd[db][r] : 0.f;
            if (SIG) c_bs[db][r] = ok ? c_bs[db][r] : 0.f;
        }
    const float eps = a.off_eps >= 0 ? eps_raw * a.eps_cli : a.eps_cli;
    const float inv_var = expf(-eps), sigma = expf(0.5f * eps);
    const float dscale = inv_var * a.inv_bt;

#include "mfma_chain_zero.inc"
    VAEK_MSTAMP(0);

#ifdef VAEK_ABLATE   // diagnostic (tools/ablate.sh): what do dispatch + the input/weight loads + the partial-row store cost?
    {
        float sink = wmu[0][0][0] + wy[0][0][0] + wg[0][0][0] + c_be[0][0] + c_sd[0][0] + c_bd[0][0] + eps;
#pragma unroll
        for (int s = 0; s < NSUB; ++s) {
#pragma unroll
            for (int r = 0; r < 4; ++r) sink += xv[s][0][r] + z2v[s][0][r] + z1v[s][0][r] + z1v[s][NLB - 1][r];
        }
        float* outp = a.partials + (long long)blockIdx.x * a.pstride;
        for (int idx = t; idx < a.P + kExtra; idx += 256) outp[idx] = sink;
        if (blockIdx.x == 0 && t == 0 && a.step_dev) a.step_dev[0] += 1;
        return;
    }
#endif
    // (the next tile's inputs are fetched at the END of the body, not under an `if` at its top: with the reload on a side
    // path into the loop header hipcc's waitcnt bookkeeping merged two load histories and made the first product wait for
    // nearly every load; at B = 65 536 the body runs once per workgroup)
    for (int tile = blockIdx.x; tile < a.ntiles;) {
        VAEK_MSTAMP(1);
#include "mfma_chain_tile.inc"
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        tile += gridDim.x;
        if (tile < a.ntiles) load_inputs(tile);
    }
    VAEK_MSTAMP(5);

    // ---- epilogue: column sums over the 16 lanes of a row, cross-wave sum through LDS, one partial row ---
#include "mfma_chain_reduce.inc"
    if (!SINGLE) {
        float* out = a.partials + (long long)blockIdx.x * a.pstride;
        float ov[NOUT];
#pragma unroll
        for (int k = 0; k < NOUT; ++k) ov[k] = batch_sum_k(k);       // all reads in flight, then the stores
#pragma unroll
        for (int k = 0; k < NOUT; ++k) {
            const int idx = t + 256 * k;
            if (idx < a.P + kExtra) out[idx] = ov[k];
        }
        VAEK_MSTAMP(6);
        if (blockIdx.x == 0 && t == 0 && a.step_dev) a.step_dev[0] += 1;
        return;
    }
    // ---- single-launch step: this workgroup holds the whole batch, so its sums ARE the batch sums, and what
    // fused_finalize_kernel does in a second launch for bigger batches happens here: closed-form KL / log-variance terms,
    // the three means, Adam, the step counter, the loss ring.  All reads of params come before the barrier, all writes
    // after it.  (The two forms are never mixed for one context: grid == 1 always takes this one.)
    const int tstep = a.step_dev[0] + 1;
    const float s_mse_t = fetch_cs(G::NCS + 0), s_musq_t = fetch_cs(G::NCS + 1), s_deps_t = fetch_cs(G::NCS + 2);
    float gk[NOUT], pk[NOUT], mk[NOUT], vk[NOUT];
    float* const pother = a.params_rw;
#pragma unroll
    for (int k = 0; k < NOUT; ++k) {
        const int idx = t + 256 * k;
        gk[k] = 0.f; pk[k] = 0.f; mk[k] = 0.f; vk[k] = 0.f;
        if (idx >= a.P + kExtra) continue;
        float gq_ = batch_sum_k(k);
        if (idx < a.P) { pk[k] = a.params_rw[idx]; mk[k] = a.m[idx]; vk[k] = a.v[idx]; }
#include "mfma_chain_grad.inc"
        gk[k] = gq_;
    }
    __syncthreads();
    const float bc1 = -expm1f((float)tstep * -0.10536051565782628f);
    const float bc2 = -expm1f((float)tstep * -0.0010005003335835335f);
#pragma unroll
    for (int k = 0; k < NOUT; ++k) {
        const int idx = t + 256 * k;
        if (idx >= a.P + kExtra) continue;
        a.grads[idx] = gk[k];
        if (idx == a.P && a.loss_hist) a.loss_hist[(long long)(tstep - 1) % a.loss_hist_cap] = gk[k];
        if (idx < a.P) {
            adam_apply_f(pk[k], gk[k], mk[k], vk[k], a.lr, bc1, bc2);
            a.params_rw[idx] = pk[k]; a.m[idx] = mk[k]; a.v[idx] = vk[k];
        }
    }
    if (t == 0) a.step_dev[0] = tstep;
    VAEK_MSTAMP(6);
}

// ---- variant table ---------------------------------------------------------------------------------
typedef void (*MfmaKernel)(const float*, const FusedArgs);
struct MfmaVariant { int dp, lp, sig, exact; MfmaKernel fn, fn_single; size_t lds_bytes; };
#define VAEK_MFMA(DP, LP, SIG, EXACT) \
    {DP, LP, SIG, EXACT, fused_linear_mfma_kernel<DP, LP, (SIG) != 0, (EXACT) != 0, false>, \
     fused_linear_mfma_kernel<DP, LP, (SIG) != 0, (EXACT) != 0, true>, sizeof(float) * MGeom<DP, LP, (SIG) != 0>::LDS_FLOATS}

static const MfmaVariant kMfmaVariants[] = {
#define VAEK_MFMA_ROW(DP, LP, SIG, EXACT) VAEK_MFMA(DP, LP, SIG, EXACT),
    VAEK_MFMA_SHAPES(VAEK_MFMA_ROW)
#undef VAEK_MFMA_ROW
};

static const MfmaVariant* pick_mfma(const vaek_ctx* c) {
    if (c->cfg.n_enc_hidden != 0 || c->cfg.n_dec_hidden != 0 || c->cfg.dtype != VAEK_F32) return nullptr;
    return pick_shape(kMfmaVariants, c, &MfmaVariant::lds_bytes);
}

bool fused_mfma_supported(const vaek_ctx* c) { return pick_mfma(c) != nullptr; }

int fused_mfma_launch(const vaek_ctx* c, const float* params, const void* args_void, int grid, hipStream_t st) {
    const MfmaVariant* var = pick_mfma(c);
    if (!var) { set_error("mfma fused path not available"); return VAEK_ERR_INVALID; }
    const FusedArgs& a = *static_cast<const FusedArgs*>(args_void);
    static thread_local PerDeviceOnce attr_set[2][sizeof(kMfmaVariants) / sizeof(kMfmaVariants[0])];
    PerDeviceOnce& once = attr_set[a.single ? 1 : 0][var - kMfmaVariants];
    const MfmaKernel fn = a.single ? var->fn_single : var->fn;
    if (var->lds_bytes > 64 * 1024) VAEK_HIP_CHECK(set_max_dynamic_lds(once, fn, var->lds_bytes));
    {
        ProfScope ps(a.single ? "fused_linear_mfma_single" : "fused_linear_mfma", st);
        launch_k(ps, fn, dim3(grid), dim3(256), var->lds_bytes, st, params, a);
    }
    VAEK_HIP_CHECK(hipGetLastError());
    return VAEK_OK;
}

}  // namespace vaek
