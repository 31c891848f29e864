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
// log-variance terms, the three means, Adam, the loss ring) are those of fused_linear_mfma_kernel<.., SINGLE>, operation for
// operation; that kernel's comments explain them and are not repeated.
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
#include "mfma_geom.h"
#include "rng_dev.h"
#include "vaek_internal.h"

namespace vaek {

constexpr int kResidentMaxSteps = 1024;      // steps per launch: bounds a launch to milliseconds on a shared machine while the
                                             // launch boundary stays under 1 % of it -- a cap, not a tuned value
constexpr size_t kLdsLimit = 160 * 1024;

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
    static constexpr int PMAX = DP * LP + LP + (SIG ? 2 : 1) * (LP * DP + DP) + LP + 1 + kExtra;
    static constexpr int NOUT = (PMAX + 255) / 256;
    static constexpr int T_ALLOC = (G::LDS_FLOATS + 3) & ~3;      // the T / R image of the chain
    static constexpr int P_ALLOC = (PMAX + 3) & ~3;               // the parameter image behind it
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
    constexpr int NDB = AD::NB, NLB = AL::NB, NSUB = G::NSUB, NOUT = RG::NOUT;
    extern __shared__ __attribute__((aligned(16))) float T[];
    float* const Pimg = T + RG::T_ALLOC;
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

    // ---- where each of this thread's outputs sits in the cross-wave reduction image (as the SINGLE kernel) ---------
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

    auto latrow = [&](int lb) { return AL::feat(lb, ai >> 2, ai & 3); };
    auto datrow = [&](int db) { return AD::feat(db, ai >> 2, ai & 3); };
    auto w_ok1 = [&](int lb, int db, int s) { return s < AD::nreg(db) && (ai & 3) < AL::nreg(lb) && latrow(lb) < L && AD::feat(db, akg, s) < D; };
    auto w_ok2 = [&](int db, int lb, int s) { return s < AL::nreg(lb) && (ai & 3) < AD::nreg(db) && datrow(db) < D && AL::feat(lb, akg, s) < L; };
    auto rowsum = [&](float v) {
        v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xf, 0xf, false));   // row_ror:8
        v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x124, 0xf, 0xf, false));   // row_ror:4
        v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x122, 0xf, 0xf, false));   // row_ror:2
        v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x121, 0xf, 0xf, false));   // row_ror:1
        return v;
    };
    auto rows4 = [&](float v) {
        v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x142, 0xa, 0xf, false));
        v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x143, 0xc, 0xf, false));
        return v;
    };

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
                        const float4 u = *reinterpret_cast<const float4*>(px[s] + min(AD::feat(db, g, 0), D - 4));
                        xv[s][db][0] = u.x; xv[s][db][1] = u.y; xv[s][db][2] = u.z; xv[s][db][3] = u.w;
                        const float4 w = *reinterpret_cast<const float4*>(pz2[s] + min(AD::feat(db, g, 0), D - 4));
                        z2v[s][db][0] = w.x; z2v[s][db][1] = w.y; z2v[s][db][2] = w.z; z2v[s][db][3] = w.w;
                    } else {
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            xv[s][db][r] = r < AD::nreg(db) ? px[s][min(AD::feat(db, g, r), D - 1)] : 0.f;
                            z2v[s][db][r] = r < AD::nreg(db) ? pz2[s][min(AD::feat(db, g, r), D - 1)] : 0.f;
                        }
                    }
                }
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
        }

        // ---- weights as MFMA A operands and per-lane constants, from the parameter image -----------------------
        float wmu[NLB][NDB][4], wy[NDB][NLB][4], wg[NLB][NDB][4], wys[SIG ? NDB : 1][NLB][4], wgs[SIG ? NLB : 1][NDB][4];
#pragma unroll
        for (int lb = 0; lb < NLB; ++lb)
#pragma unroll
            for (int db = 0; db < NDB; ++db)
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const int lo = latrow(lb), dk = AD::feat(db, akg, s);
                    const bool ok = w_ok1(lb, db, s);
                    wmu[lb][db][s] = ok ? Pimg[dk * L + lo] : 0.f;
                    wg[lb][db][s] = ok ? Pimg[off_wd + lo * D + dk] : 0.f;
                    if (SIG) wgs[lb][db][s] = ok ? Pimg[off_ws + lo * D + dk] : 0.f;
                    const int dout = datrow(db), lk = AL::feat(lb, akg, s);
                    const bool ok2 = w_ok2(db, lb, s);
                    wy[db][lb][s] = ok2 ? Pimg[off_wd + lk * D + dout] : 0.f;
                    if (SIG) wys[db][lb][s] = ok2 ? Pimg[off_ws + lk * D + dout] : 0.f;
                }
        float c_be[NLB][4], c_sd[NLB][4], c_bd[NDB][4], c_bs[SIG ? NDB : 1][4];
#pragma unroll
        for (int lb = 0; lb < NLB; ++lb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int l = AL::feat(lb, g, r);
                const bool ok = r < AL::nreg(lb) && l < L;
                c_be[lb][r] = ok ? Pimg[off_be + l] : 0.f;
                c_sd[lb][r] = ok ? expf(0.5f * Pimg[off_epsp + l]) : 0.f;                // e^{lv/2}, networks.py:73
            }
#pragma unroll
        for (int db = 0; db < NDB; ++db)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int d = AD::feat(db, g, r);
                const bool ok = r < AD::nreg(db) && d < D;
                c_bd[db][r] = ok ? Pimg[off_bd + d] : 0.f;
                if (SIG) c_bs[db][r] = ok ? Pimg[off_bs + d] : 0.f;
            }
        const float eps = a.off_eps >= 0 ? Pimg[a.off_eps] * a.eps_cli : a.eps_cli;
        const float inv_var = expf(-eps), sigma = expf(0.5f * eps);
        const float dscale = inv_var * a.inv_bt;
        // the ones rows: T doubles as the reduction image R at the end of every step, so they are written again
        if (G::ONE1) T[(G::FS + LP) * G::TS + t] = 1.f;          // each wave reads back only its own 64 columns
        if (G::ONE2) T[(G::FX + DP) * G::TS + t] = 1.f;

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

        // ---- mu^T = We^T x^T + be ---------------------------------------------------------------------------
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
        // ---- samples = mu + e^{lv/2} z1 (networks.py:73-74) -----------------------------------------------------
        float sv[NSUB][NLB][4];
#pragma unroll
        for (int s = 0; s < NSUB; ++s)
#pragma unroll
            for (int lb = 0; lb < NLB; ++lb)
#pragma unroll
                for (int r = 0; r < AL::nreg(lb); ++r) {
                    const float mm = mu[s][lb][r];
                    sv[s][lb][r] = fmaf(c_sd[lb][r], z1v[s][lb][r], mm);
                    s_musq = valid[s] ? fmaf(mm, mm, s_musq) : s_musq;
                }
        // ---- y^T = Wd^T samples^T + bd (and the sigmoid head) -----------------------------------------------------
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
        // ---- residual, loss terms, dL/dx_hat (networks.py:81-83, :94-98) ---------------------------------------------
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
        // ---- g^T = Wd dy^T (+ Ws dys^T) --------------------------------------------------------------------------
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
        // ---- dmu, column sums, and the feature-major image for the batch-reduction GEMMs ------------------------------
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
        // ---- dWd (+dWs) = samples^T [dy|dys],  dWe = x^T dmu : K = the wave's 64 samples ---------------------------------
        {
            const float* Tk = T + wave * 64 + (lane >> 4) + (lane & 15) * G::TS;
            constexpr int NOP = G::IB1 + G::JB1 + G::IB2 + G::JB2;
            constexpr int GS = (2 * NOP <= 15) ? 2 : 1, NG = 16 / GS;      // lgkmcnt is a 4-bit counter: see fused_mfma.hip
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

        // ---- column sums over the 16 lanes of a row, cross-wave sum through LDS ------------------------------------------
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
                        const float vv = rowsum(cs_dy[db][r]);
                        float vs = 0.f;
                        if (SIG) vs = rowsum(cs_dys[db][r]);
                        if (j == 0 && d < DP) { CS[d] = vv; if (SIG) CS[DP + d] = vs; }
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
                        const float vv = rowsum(cs_dmu[lb][r]);
                        if (j == 0 && l < LP) CS[G::NB1 + l] = vv;
                    }
                }
            float m0 = rowsum(s_mse), m1 = rowsum(s_musq), m2 = rowsum(s_deps);
            m0 = rows4(m0); m1 = rows4(m1); m2 = rows4(m2);
            if (lane == 63) { CS[G::NCS + 0] = m0; CS[G::NCS + 1] = m1; CS[G::NCS + 2] = m2; }
        }
        __syncthreads();
        auto fetch_cs = [&](int k) -> float {
            float vv = 0.f;
#pragma unroll
            for (int w = 0; w < G::NW; ++w) vv += T[w * G::R_PER_WAVE + G::NBLK * 256 + k];
            return vv;
        };
        auto batch_sum_k = [&](int k) -> float {
            const int o = src_off[k];
            const int oc = o != 0xffff ? o : 0;
            float vv = 0.f;
#pragma unroll
            for (int w = 0; w < G::NW; ++w) vv += T[w * G::R_PER_WAVE + oc];
            return o != 0xffff ? vv : 0.f;
        };

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
            if (idx >= off_epsp && idx < off_epsp + L) {
                const float lv = pk[k];
                gq_ = 0.5f * expf(0.5f * lv) * gq_ - 0.5f * (1.f - expf(lv)) * a.rows_over_bt;
            } else if (idx == a.off_eps) {
                gq_ = a.eps_cli * (s_deps_t + 0.5f * a.rows * (float)D) * a.inv_bt;
            } else if (idx >= a.P) {
                if (idx < a.P + 3) {
                    float klc = 0.f;
                    for (int l = 0; l < L; ++l) { const float lv = Pimg[off_epsp + l]; klc += 1.f + lv - expf(lv); }
                    const float eps_s = a.off_eps >= 0 ? Pimg[a.off_eps] * a.eps_cli : a.eps_cli;
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

static const ResidentVariant* pick_resident(const vaek_ctx* c) {
    const ResidentVariant* best = nullptr;
    for (const auto& v : kResidentVariants) {
        if (v.sig != (c->cfg.sigmoid_decoder ? 1 : 0) || v.dp < c->D || v.lp < c->L || v.base_bytes > kLdsLimit) continue;
        if (v.exact && (v.dp != c->D || v.lp != c->L)) continue;
        if (!best || v.dp * v.lp < best->dp * best->lp) best = &v;
    }
    return best;
}

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

int resident_train_loop(vaek_ctx* c, float* params, float* grads, float* m, float* v, int32_t* step_dev, const BatchArgs& gen,
                        int n_steps, float lr, void* ws, hipStream_t st, const TrajArgs* traj) {
    const ResidentVariant* var = c->resident ? pick_resident(c) : nullptr;
    if (!var) { set_error("resident train loop not available for this configuration"); return VAEK_ERR_INVALID; }
    const bool in_lds = stage_in_lds(c, var);
    const size_t lds = var->base_bytes + (in_lds ? stage_bytes(c) : 0);
    static thread_local PerDeviceOnce attr_set[2][sizeof(kResidentVariants) / sizeof(kResidentVariants[0])];      // [traced]: two kernels
    PerDeviceOnce& once = attr_set[traj ? 1 : 0][var - kResidentVariants];
    if (lds > 64 * 1024)      // the most this variant ever asks for (the batch image grows with the batch, which another context may have larger)
        VAEK_HIP_CHECK(set_max_dynamic_lds(once, traj ? (const void*)var->fn_traj : (const void*)var->fn, kLdsLimit));
    ResidentArgs a{};
    a.params = params; a.grads = grads; a.m = m; a.v = v; a.step_dev = step_dev;
    a.stage = in_lds ? nullptr : reinterpret_cast<float*>(static_cast<char*>(ws) + c->ws_resident);
    a.B = c->B; a.D = c->D; a.L = c->L; a.P = (int)c->P; a.off_epsp = (int)c->off_epsp; a.off_eps = (int)c->off_eps;
    a.inv_bt = (float)(1.0 / (double)c->Bt); a.eps_cli = c->cfg.eps_cli; a.lr = lr;
    a.rows_over_bt = (float)((double)c->B / (double)c->Bt); a.rows = (float)c->B;
    a.loss_hist = c->loss_hist; a.loss_hist_cap = c->loss_hist_cap;
    a.gen = gen;
    // every launch leaves params / m / v / grads / *step_dev / the ring in HBM: the next one starts from memory alone
    for (int left = n_steps; left > 0; left -= kResidentMaxSteps) {
        a.n_steps = left < kResidentMaxSteps ? left : kResidentMaxSteps;
        // the traced launch finds the slot of every record from the step counter it reads itself: nothing to carry between launches
        ProfScope ps(traj ? "linear_resident_traj" : "linear_resident", st);
        if (traj) launch_k(ps, var->fn_traj, dim3(1), dim3(256), lds, st, a, *traj);
        else launch_k(ps, var->fn, dim3(1), dim3(256), lds, st, a);
        VAEK_HIP_CHECK(hipGetLastError());
    }
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

int resident_train_loop_replicas(vaek_ctx* c, float* params, float* grads, float* m, float* v, int32_t* step_dev, const BatchArgs& gen,
                                 int n, long long state_stride, long long grads_stride, const unsigned long long* seeds, const float* lrs,
                                 long long a_stride, float* loss_hist, long long loss_hist_cap, int n_steps, float lr, void* ws,
                                 hipStream_t st, const TrajArgs* traj) {
    const ResidentVariant* var = c->resident ? pick_resident(c) : nullptr;
    if (!var) { set_error("resident train loop not available for this configuration"); return VAEK_ERR_INVALID; }
    const bool in_lds = stage_in_lds(c, var);
    const size_t lds = var->base_bytes + (in_lds ? stage_bytes(c) : 0);
    static thread_local PerDeviceOnce attr_set[2][sizeof(kResidentVariants) / sizeof(kResidentVariants[0])];      // [traced]: two kernels
    PerDeviceOnce& once = attr_set[traj ? 1 : 0][var - kResidentVariants];
    if (lds > 64 * 1024)
        VAEK_HIP_CHECK(set_max_dynamic_lds(once, traj ? (const void*)var->fn_replicas_traj : (const void*)var->fn_replicas, kLdsLimit));
    ResidentArgs a{};
    a.params = params; a.grads = grads; a.m = m; a.v = v; a.step_dev = step_dev;
    a.stage = in_lds ? nullptr : static_cast<float*>(ws);
    a.B = c->B; a.D = c->D; a.L = c->L; a.P = (int)c->P; a.off_epsp = (int)c->off_epsp; a.off_eps = (int)c->off_eps;
    a.inv_bt = (float)(1.0 / (double)c->Bt); a.eps_cli = c->cfg.eps_cli; a.lr = lr;
    a.rows_over_bt = (float)((double)c->B / (double)c->Bt); a.rows = (float)c->B;
    a.loss_hist = loss_hist; a.loss_hist_cap = loss_hist ? loss_hist_cap : 0;      // the caller's rings, never the context's
    a.gen = gen;
    ReplicaArgs rp{};
    rp.state_stride = state_stride; rp.grads_stride = grads_stride; rp.a_stride = a_stride;
    rp.stage_stride = stage_floats(c->B, c->D, c->L);
    rp.seeds = seeds; rp.lrs = lrs;
    for (int left = n_steps; left > 0; left -= kResidentMaxSteps) {
        a.n_steps = left < kResidentMaxSteps ? left : kResidentMaxSteps;
        ProfScope ps(traj ? "linear_resident_replicas_traj" : "linear_resident_replicas", st);
        if (traj) launch_k(ps, var->fn_replicas_traj, dim3((unsigned)n), dim3(256), lds, st, a, rp, *traj);
        else launch_k(ps, var->fn_replicas, dim3((unsigned)n), dim3(256), lds, st, a, rp);
        VAEK_HIP_CHECK(hipGetLastError());
    }
    return VAEK_OK;
}

}  // namespace vaek
