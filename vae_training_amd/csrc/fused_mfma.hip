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
#include "mfma_geom.h"
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
    constexpr int NDB = AD::NB, NLB = AL::NB, NSUB = G::NSUB;
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
    // Every load is UNCONDITIONAL, from a clamped row (and, in the padded variants, a clamped column), and nothing is
    // zeroed afterwards: a sample past the batch end reads row B-1 again and a padded column reads column D-1 / L-1 --
    // finite values whose every contribution is already masked downstream (rr, dmu, mu^2 by `valid`; padded columns by
    // zero weights / zero e^{lv/2} and by rows of the gradient image nobody reads).  With the loads under `if (valid)`
    // hipcc merged each conditionally loaded float4 into its zero-initialised registers INSIDE the branch, i.e. put an
    // `s_waitcnt vmcnt` into every sub-tile's block, and a zeroing pass after the loads waits for all of them.  Now all 56
    // loads of a wave (24 parameter, 32 input) leave before the first wait.  Measured: 8.76 -> 8.64 us per launch only --
    // the load phase is bandwidth-, not latency-bound, and at 260 VGPRs hipcc still copies the z1 / z2 registers away early
    // enough that the first products wait for ~3/4 of the bytes.
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
            for (int db = 0; db < NDB; ++db) {
                if (AD::full(db) && vecD) {
                    const float4 u = *reinterpret_cast<const float4*>(px[s] + min(AD::feat(db, g, 0), D - 4));
                    xv[s][db][0] = u.x; xv[s][db][1] = u.y; xv[s][db][2] = u.z; xv[s][db][3] = u.w;
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) xv[s][db][r] = r < AD::nreg(db) ? px[s][min(AD::feat(db, g, r), D - 1)] : 0.f;
                }
            }
        if (what & 2)
#pragma unroll
        for (int s = 0; s < NSUB; ++s)
#pragma unroll
            for (int lb = 0; lb < NLB; ++lb) {
                if (AL::full(lb) && vecL) {
                    const float4 u = *reinterpret_cast<const float4*>(pz1[s] + min(AL::feat(lb, g, 0), L - 4));
                    z1v[s][lb][0] = u.x; z1v[s][lb][1] = u.y; z1v[s][lb][2] = u.z; z1v[s][lb][3] = u.w;
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) z1v[s][lb][r] = r < AL::nreg(lb) ? pz1[s][min(AL::feat(lb, g, r), L - 1)] : 0.f;
                }
            }
        if (what & 2)
#pragma unroll
        for (int s = 0; s < NSUB; ++s)
#pragma unroll
            for (int db = 0; db < NDB; ++db) {
                if (AD::full(db) && vecD) {
                    const float4 w = *reinterpret_cast<const float4*>(pz2[s] + min(AD::feat(db, g, 0), D - 4));
                    z2v[s][db][0] = w.x; z2v[s][db][1] = w.y; z2v[s][db][2] = w.z; z2v[s][db][3] = w.w;
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r) z2v[s][db][r] = r < AD::nreg(db) ? pz2[s][min(AD::feat(db, g, r), D - 1)] : 0.f;
                }
            }
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

    // ---- weights as MFMA A operands (lane = output row ai, k group akg), zero outside [D, L] -------
    // row ai of a block <-> (g', r') = (ai >> 2, ai & 3)
    auto latrow = [&](int lb) { return AL::feat(lb, ai >> 2, ai & 3); };
    auto datrow = [&](int db) { return AD::feat(db, ai >> 2, ai & 3); };
    float wmu[NLB][NDB][4], wy[NDB][NLB][4], wg[NLB][NDB][4], wys[SIG ? NDB : 1][NLB][4], wgs[SIG ? NLB : 1][NDB][4];
    // Like the inputs, every parameter load is unconditional (index 0 where the operand is padding) and the zeroing
    // selects come AFTER the input loads have been issued: a select inside the load sequence is an s_waitcnt there.
    auto w_ok1 = [&](int lb, int db, int s) { return s < AD::nreg(db) && (ai & 3) < AL::nreg(lb) && latrow(lb) < L && AD::feat(db, akg, s) < D; };
    auto w_ok2 = [&](int db, int lb, int s) { return s < AL::nreg(lb) && (ai & 3) < AD::nreg(db) && datrow(db) < D && AL::feat(lb, akg, s) < L; };
#pragma unroll
    for (int lb = 0; lb < NLB; ++lb)
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                // mu: out row = latent latrow(lb), k = data dim feat(db, akg, s);  g: same roles, weights Wd
                const int lo = latrow(lb), dk = AD::feat(db, akg, s);
                const bool ok = w_ok1(lb, db, s);
                wmu[lb][db][s] = params[ok ? dk * L + lo : 0];
                wg[lb][db][s] = params[ok ? off_wd + lo * D + dk : 0];
                if (SIG) wgs[lb][db][s] = params[ok ? off_ws + lo * D + dk : 0];
                // y: out row = data dim datrow(db), k = latent feat(lb, akg, s)
                const int dout = datrow(db), lk = AL::feat(lb, akg, s);
                const bool ok2 = w_ok2(db, lb, s);
                wy[db][lb][s] = params[ok2 ? off_wd + lk * D + dout : 0];
                if (SIG) wys[db][lb][s] = params[ok2 ? off_ws + lk * D + dout : 0];
            }
    // per-lane constants in accumulator layout (group g, register r)
    float c_be[NLB][4], c_sd[NLB][4], c_bd[NDB][4], c_bs[SIG ? NDB : 1][4];
#pragma unroll
    for (int lb = 0; lb < NLB; ++lb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int l = AL::feat(lb, g, r);
            const bool ok = r < AL::nreg(lb) && l < L;
            c_be[lb][r] = params[ok ? off_be + l : 0];
            c_sd[lb][r] = params[ok ? off_epsp + l : 0];                      // logvar_e now, e^{lv/2} below
        }
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int d = AD::feat(db, g, r);
            const bool ok = r < AD::nreg(db) && d < D;
            c_bd[db][r] = params[ok ? off_bd + d : 0];
            if (SIG) c_bs[db][r] = params[ok ? off_bs + d : 0];
        }
    const float eps_raw = a.off_eps >= 0 ? params[a.off_eps] : 0.f;

    // z1 / z2 AFTER the weights (loads return in order, and the first product needs the weights and x only); x went out
    // before the ~150 VALU of parameter indexing
    load_inputs(blockIdx.x, 2);
    if (G::ONE1) T[(G::FS + LP) * G::TS + t] = 1.f;          // each wave reads back only its own 64 columns: no barrier needed
    if (G::ONE2) T[(G::FX + DP) * G::TS + t] = 1.f;
    // Where each of this thread's outputs (flat-gradient index t, t + 256, ...) will sit in the cross-wave reduction image
    // of the epilogue -- worked out NOW, under the input loads' latency, instead of as ~40 VALU + divergent branches per
    // output on the kernel's tail.  0xffff = an output this kernel leaves zero.
    constexpr int PMAX = DP * LP + LP + (SIG ? 2 : 1) * (LP * DP + DP) + LP + 1 + kExtra;
    constexpr int NOUT = (PMAX + 255) / 256;
    unsigned short src_off[NOUT];
    {
        auto blk_off = [&](int gemm, int i, int jj) {
            const int blk = gemm == 1 ? (i >> 4) * G::JB1 + (jj >> 4) : G::IB1 * G::JB1 + (i >> 4) * G::JB2 + (jj >> 4);
            return (blk * 16 + (i & 15)) * 16 + (jj & 15);
        };
#pragma unroll
        for (int k = 0; k < NOUT; ++k) {
            const int idx = t + 256 * k;
            int o = 0xffff;
            if (idx < off_be) o = blk_off(2, idx / L, idx % L);                                   // dWe = x^T dmu
            else if (idx < off_wd) o = G::ONE2 ? blk_off(2, DP, idx - off_be) : G::NBLK * 256 + G::NB1 + idx - off_be;   // dbe = 1^T dmu
            else if (idx < off_bd) { const int kk = idx - off_wd; o = blk_off(1, kk / D, kk % D); }   // dWd = samples^T dy
            else if (idx < off_bd + D) o = G::ONE1 ? blk_off(1, LP, idx - off_bd) : G::NBLK * 256 + idx - off_bd;        // dbd = 1^T dy
            else if (SIG && idx < off_bs) { const int kk = idx - off_ws; o = blk_off(1, kk / D, DP + kk % D); }
            else if (SIG && idx < off_bs + D) o = G::ONE1 ? blk_off(1, LP, DP + idx - off_bs) : G::NBLK * 256 + DP + idx - off_bs;
            else if (idx >= off_epsp && idx < off_epsp + L) o = G::NBLK * 256 + G::NB1 + LP + idx - off_epsp;   // sum g*z1
            else if (idx >= a.P && idx < a.P + 3) o = G::NBLK * 256 + G::NCS + idx - a.P;
            src_off[k] = (unsigned short)o;
        }
    }
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

    f32x4 acc1[G::IB1][G::JB1], acc2[G::IB2][G::JB2];
#pragma unroll
    for (int i = 0; i < G::IB1; ++i)
#pragma unroll
        for (int jj = 0; jj < G::JB1; ++jj) acc1[i][jj] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < G::IB2; ++i)
#pragma unroll
        for (int jj = 0; jj < G::JB2; ++jj) acc2[i][jj] = f32x4{0.f, 0.f, 0.f, 0.f};
    float cs_dy[NDB][4], cs_dys[SIG ? NDB : 1][4], cs_dmu[NLB][4], cs_gz[NLB][4];
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
        for (int r = 0; r < 4; ++r) { cs_dy[db][r] = 0.f; if (SIG) cs_dys[db][r] = 0.f; }
#pragma unroll
    for (int lb = 0; lb < NLB; ++lb)
#pragma unroll
        for (int r = 0; r < 4; ++r) { cs_dmu[lb][r] = 0.f; cs_gz[lb][r] = 0.f; }
    float s_mse = 0.f, s_deps = 0.f, s_musq = 0.f;
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
        // ---- mu^T = We^T x^T + be : the four 16-sample sub-tiles are independent MFMA chains ----------
        f32x4 mu[NSUB][NLB];
#pragma unroll
        for (int s = 0; s < NSUB; ++s)
#pragma unroll
            for (int lb = 0; lb < NLB; ++lb) mu[s][lb] = f32x4{c_be[lb][0], c_be[lb][1], c_be[lb][2], c_be[lb][3]};
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
            for (int k = 0; k < AD::nreg(db); ++k)
#pragma unroll
                for (int s = 0; s < NSUB; ++s)
#pragma unroll
                    for (int lb = 0; lb < NLB; ++lb)
                        mu[s][lb] = __builtin_amdgcn_mfma_f32_16x16x4f32(wmu[lb][db][k], xv[s][db][k], mu[s][lb], 0, 0, 0);
        // ---- samples = mu + e^{lv/2} z1 (networks.py:73-74), in accumulator layout ---------------------
        float sv[NSUB][NLB][4];
#pragma unroll
        for (int s = 0; s < NSUB; ++s)
#pragma unroll
            for (int lb = 0; lb < NLB; ++lb)
#pragma unroll
                for (int r = 0; r < AL::nreg(lb); ++r) {
                    const float m = mu[s][lb][r];
                    sv[s][lb][r] = fmaf(c_sd[lb][r], z1v[s][lb][r], m);
                    s_musq = valid[s] ? fmaf(m, m, s_musq) : s_musq;
                }
        VAEK_MSTAMP(2);
        // ---- y^T = Wd^T samples^T + bd (and the sigmoid head): B operand = the registers above ----------
        f32x4 y[NSUB][NDB], ys[SIG ? NSUB : 1][NDB];
#pragma unroll
        for (int s = 0; s < NSUB; ++s)
#pragma unroll
            for (int db = 0; db < NDB; ++db) {
                y[s][db] = f32x4{c_bd[db][0], c_bd[db][1], c_bd[db][2], c_bd[db][3]};
                if (SIG) ys[s][db] = f32x4{c_bs[db][0], c_bs[db][1], c_bs[db][2], c_bs[db][3]};
            }
#pragma unroll
        for (int lb = 0; lb < NLB; ++lb)
#pragma unroll
            for (int k = 0; k < AL::nreg(lb); ++k)
#pragma unroll
                for (int s = 0; s < NSUB; ++s)
#pragma unroll
                    for (int db = 0; db < NDB; ++db) {
                        y[s][db] = __builtin_amdgcn_mfma_f32_16x16x4f32(wy[db][lb][k], sv[s][lb][k], y[s][db], 0, 0, 0);
                        if (SIG) ys[s][db] = __builtin_amdgcn_mfma_f32_16x16x4f32(wys[db][lb][k], sv[s][lb][k], ys[s][db], 0, 0, 0);
                    }
        // ---- residual, loss terms, dL/dx_hat (networks.py:81-83, :94-98) -------------------------------
        float dyv[NSUB][NDB][4], dysv[SIG ? NSUB : 1][NDB][4];
#pragma unroll
        for (int s = 0; s < NSUB; ++s)
#pragma unroll
            for (int db = 0; db < NDB; ++db)
#pragma unroll
                for (int r = 0; r < AD::nreg(db); ++r) {
                    const int d = AD::feat(db, g, r);
                    float xh = fmaf(sigma, z2v[s][db][r], y[s][db][r]);
                    float sg = 0.f;
                    if (SIG) { sg = 1.f / (1.f + expf(-ys[s][db][r])); xh += sg; }
                    const float rr = (valid[s] && d < D) ? xh - xv[s][db][r] : 0.f;
                    const float q = rr * rr * inv_var;
                    s_mse = fmaf(0.5f, q, s_mse);
                    s_deps += -0.5f * q + 0.5f * sigma * z2v[s][db][r] * rr * inv_var;
                    const float dyd = rr * dscale;
                    dyv[s][db][r] = dyd;
                    if (!G::ONE1) cs_dy[db][r] += dyd;
                    if (SIG) { const float ds = dyd * sg * (1.f - sg); dysv[s][db][r] = ds; if (!G::ONE1) cs_dys[db][r] += ds; }
                }
        VAEK_MSTAMP(3);
        // ---- g^T = Wd dy^T (+ Ws dys^T) ------------------------------------------------------------------
        f32x4 gq[NSUB][NLB];
#pragma unroll
        for (int s = 0; s < NSUB; ++s)
#pragma unroll
            for (int lb = 0; lb < NLB; ++lb) gq[s][lb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
            for (int k = 0; k < AD::nreg(db); ++k)
#pragma unroll
                for (int s = 0; s < NSUB; ++s)
#pragma unroll
                    for (int lb = 0; lb < NLB; ++lb) {
                        gq[s][lb] = __builtin_amdgcn_mfma_f32_16x16x4f32(wg[lb][db][k], dyv[s][db][k], gq[s][lb], 0, 0, 0);
                        if (SIG) gq[s][lb] = __builtin_amdgcn_mfma_f32_16x16x4f32(wgs[lb][db][k], dysv[s][db][k], gq[s][lb], 0, 0, 0);
                    }
        // ---- dmu, column sums, and the feature-major image for the batch-reduction GEMMs ------------------
#pragma unroll
        for (int s = 0; s < NSUB; ++s) {
            float* Tc = T + wave * 64 + s * 16 + j;
#pragma unroll
            for (int lb = 0; lb < NLB; ++lb)
#pragma unroll
                for (int r = 0; r < AL::nreg(lb); ++r) {
                    const int l = AL::feat(lb, g, r);
                    const float gl = gq[s][lb][r];
                    const float dmu = valid[s] ? fmaf(mu[s][lb][r], a.inv_bt, gl) : 0.f;     // dmu = g + mu/B
                    if (!G::ONE2) cs_dmu[lb][r] += dmu;
                    cs_gz[lb][r] = fmaf(gl, z1v[s][lb][r], cs_gz[lb][r]);                     // reparam part of d lv
                    if (l < LP) { Tc[(G::FS + l) * G::TS] = sv[s][lb][r]; Tc[(G::FDM + l) * G::TS] = dmu; }
                }
#pragma unroll
            for (int db = 0; db < NDB; ++db)
#pragma unroll
                for (int r = 0; r < AD::nreg(db); ++r) {
                    const int d = AD::feat(db, g, r);
                    if (d < DP) {
                        Tc[(G::FX + d) * G::TS] = xv[s][db][r];
                        Tc[(G::FDY + d) * G::TS] = dyv[s][db][r];
                        if (SIG) Tc[(G::FDY + DP + d) * G::TS] = dysv[s][db][r];
                    }
                }
        }
        // each wave reads back only its own 64 columns: wave-level ordering is enough (no s_barrier)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        VAEK_MSTAMP(4);
        // ---- dWd (+dWs) = samples^T [dy|dys],  dWe = x^T dmu : K = the wave's 64 samples ------------------
        {
            const float* Tk = T + wave * 64 + (lane >> 4) + (lane & 15) * G::TS;
            constexpr int NOP = G::IB1 + G::JB1 + G::IB2 + G::JB2;
            // Operand prefetch runs ONE group of GS k-steps ahead: lgkmcnt is a 4-bit counter, so the wait
            // in front of a group's MFMAs can only be exact while <= 15 younger reads are in flight.
            constexpr int GS = (2 * NOP <= 15) ? 2 : 1, NG = 16 / GS;
            float op[2][GS][NOP];
            auto load_group = [&](int gi, int which) {
#pragma unroll
                for (int u = 0; u < GS; ++u) {
                    const int s4 = 4 * (gi * GS + u);
                    int n = 0;
#pragma unroll
                    for (int i = 0; i < G::IB1; ++i) op[which][u][n++] = Tk[(G::FS + 16 * i) * G::TS + s4];
#pragma unroll
                    for (int jj = 0; jj < G::JB1; ++jj) op[which][u][n++] = Tk[(G::FDY + 16 * jj) * G::TS + s4];
#pragma unroll
                    for (int i = 0; i < G::IB2; ++i) op[which][u][n++] = Tk[(G::FX + 16 * i) * G::TS + s4];
#pragma unroll
                    for (int jj = 0; jj < G::JB2; ++jj) op[which][u][n++] = Tk[(G::FDM + 16 * jj) * G::TS + s4];
                }
            };
            load_group(0, 0);
#pragma unroll
            for (int gi = 0; gi < NG; ++gi) {
                if (gi + 1 < NG) load_group(gi + 1, (gi + 1) & 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < GS; ++u) {
                    const float* o = op[gi & 1][u];
#pragma unroll
                    for (int i = 0; i < G::IB1; ++i)
#pragma unroll
                        for (int jj = 0; jj < G::JB1; ++jj)
                            acc1[i][jj] = __builtin_amdgcn_mfma_f32_16x16x4f32(o[i], o[G::IB1 + jj], acc1[i][jj], 0, 0, 0);
#pragma unroll
                    for (int i = 0; i < G::IB2; ++i)
#pragma unroll
                        for (int jj = 0; jj < G::JB2; ++jj)
                            acc2[i][jj] = __builtin_amdgcn_mfma_f32_16x16x4f32(o[G::IB1 + G::JB1 + i], o[G::IB1 + G::JB1 + G::IB2 + jj],
                                                                               acc2[i][jj], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        tile += gridDim.x;
        if (tile < a.ntiles) load_inputs(tile);
    }
    VAEK_MSTAMP(5);

    // ---- epilogue: column sums over the 16 lanes of a row, cross-wave sum through LDS, one partial row ---
    // all-reduce over the 16 lanes of a DPP row (= the 16 sample columns of one row group): v += ror(v, n)
    // as ONE v_add_f32 with a row_ror modifier each -- __shfl_xor would go through the LDS crossbar
    auto rowsum = [&](float v) {
        v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xf, 0xf, false));   // row_ror:8
        v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x124, 0xf, 0xf, false));   // row_ror:4
        v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x122, 0xf, 0xf, false));   // row_ror:2
        v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x121, 0xf, 0xf, false));   // row_ror:1
        return v;
    };
    __syncthreads();           // every wave is done with its T columns before T is reused as R
    float* R = T + wave * G::R_PER_WAVE;
    {
        const int col = lane & 15, row0 = 4 * (lane >> 4);
        int blk = 0;
#pragma unroll
        for (int i = 0; i < G::IB1; ++i)
#pragma unroll
            for (int jj = 0; jj < G::JB1; ++jj, ++blk)
#pragma unroll
                for (int r = 0; r < 4; ++r) R[(blk * 16 + row0 + r) * 16 + col] = acc1[i][jj][r];
#pragma unroll
        for (int i = 0; i < G::IB2; ++i)
#pragma unroll
            for (int jj = 0; jj < G::JB2; ++jj, ++blk)
#pragma unroll
                for (int r = 0; r < 4; ++r) R[(blk * 16 + row0 + r) * 16 + col] = acc2[i][jj][r];
        float* CS = R + G::NBLK * 256;     // [dy (DP) | dys (DP)] [dmu (LP)] [gz (LP)]
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
            for (int r = 0; r < AD::nreg(db); ++r) {
                const int d = AD::feat(db, g, r);
                if (!G::ONE1) {
                    const float v = rowsum(cs_dy[db][r]);
                    float vs = 0.f;
                    if (SIG) vs = rowsum(cs_dys[db][r]);
                    if (j == 0 && d < DP) { CS[d] = v; if (SIG) CS[DP + d] = vs; }
                }
            }
#pragma unroll
        for (int lb = 0; lb < NLB; ++lb)
#pragma unroll
            for (int r = 0; r < AL::nreg(lb); ++r) {
                const int l = AL::feat(lb, g, r);
                const float w = rowsum(cs_gz[lb][r]);
                if (j == 0 && l < LP) CS[G::NB1 + LP + l] = w;
                if (!G::ONE2) {
                    const float v = rowsum(cs_dmu[lb][r]);
                    if (j == 0 && l < LP) CS[G::NB1 + l] = v;
                }
            }
        float m0 = rowsum(s_mse), m1 = rowsum(s_musq), m2 = rowsum(s_deps);      // 16 lanes by DPP, then the 4 rows
        // the four rows by two more DPP adds (row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3: lane 63 ends
        // up with the wave's total) -- __shfl_xor is two trips through the LDS crossbar per value
        auto rows4 = [&](float v) {
            v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x142, 0xa, 0xf, false));
            v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x143, 0xc, 0xf, false));
            return v;
        };
        m0 = rows4(m0); m1 = rows4(m1); m2 = rows4(m2);
        if (lane == 63) { CS[G::NCS + 0] = m0; CS[G::NCS + 1] = m1; CS[G::NCS + 2] = m2; }
    }
    __syncthreads();
    auto fetch_cs = [&](int k) -> float {
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < G::NW; ++w) v += T[w * G::R_PER_WAVE + G::NBLK * 256 + k];
        return v;
    };
    auto batch_sum_k = [&](int k) -> float {            // this thread's k-th output, summed over the workgroup's four waves
        const int o = src_off[k];
        const int oc = o != 0xffff ? o : 0;               // unconditional LDS reads, select afterwards
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < G::NW; ++w) v += T[w * G::R_PER_WAVE + oc];
        return o != 0xffff ? v : 0.f;
    };
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
#pragma unroll
    for (int k = 0; k < NOUT; ++k) {
        const int idx = t + 256 * k;
        gk[k] = 0.f; pk[k] = 0.f; mk[k] = 0.f; vk[k] = 0.f;
        if (idx >= a.P + kExtra) continue;
        float gq_ = batch_sum_k(k);
        if (idx < a.P) { pk[k] = a.params_rw[idx]; mk[k] = a.m[idx]; vk[k] = a.v[idx]; }
        if (idx >= off_epsp && idx < off_epsp + L) {
            const float lv = pk[k];
            gq_ = 0.5f * expf(0.5f * lv) * gq_ - 0.5f * (1.f - expf(lv)) * a.rows_over_bt;
        } else if (idx == a.off_eps) {
            gq_ = a.eps_cli * (s_deps_t + 0.5f * a.rows * (float)D) * a.inv_bt;
        } else if (idx >= a.P) {
            if (idx < a.P + 3) {
                float klc = 0.f;
                for (int l = 0; l < L; ++l) { const float lv = a.params_rw[off_epsp + l]; klc += 1.f + lv - expf(lv); }
                const float eps_s = a.off_eps >= 0 ? a.params_rw[a.off_eps] * a.eps_cli : a.eps_cli;
                const float dkl = (0.5f * s_musq_t - 0.5f * a.rows * klc) * a.inv_bt;
                const float mse = (s_mse_t + 0.5f * a.rows * (float)D * (kLog2Pi + eps_s)) * a.inv_bt;
                gq_ = idx == a.P ? dkl + mse : (idx == a.P + 1 ? dkl : mse);
            } else {
                gq_ = 0.f;
            }
        }
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
    const MfmaVariant* best = nullptr;
    for (const auto& v : kMfmaVariants) {
        if (v.sig != (c->cfg.sigmoid_decoder ? 1 : 0) || v.dp < c->D || v.lp < c->L || v.lds_bytes > 160 * 1024) continue;
        if (v.exact && (v.dp != c->D || v.lp != c->L)) continue;
        if (!best || v.dp * v.lp < best->dp * best->lp) best = &v;
    }
    return best;
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
