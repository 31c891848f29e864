// Whole-network train step for VAEs whose encoder and decoder have THREE hidden layers of 64 .. 256 units each, at small batch
// (sphere_vae_padding_expts.sh: 200|200|200 both ways, D = 6 .. 21, L = 6 .. 16, batch 100).  The layer-by-layer path takes ~27
// launches for such a step; here it is two, ordered by the stream alone -- no workgroup ever waits for another inside a launch:
//
//   1. mlp3_chain_kernel: one workgroup per 16 batch rows runs encoder forward -> reparameterisation (networks.py:73-74) ->
//      decoder forward -> ELBO terms (:94-98) -> decoder dX chain -> reparam backward -> encoder dX chain for ITS rows.  The
//      activations live in LDS as [unit][sample] images, overwritten in place by their gradients (as in fused_mlp1.hip); the
//      weights stream from L2 (every workgroup reads all of them twice: forward and dX).  Every product is
//      v_mfma_f32_16x16x4_f32 (exact f32): units on the rows, the 16 samples on the columns.  Each layer's input activation and
//      output gradient go to the workspace as [unit][padded batch], plus one row of partial sums per workgroup.
//   2. mlp3_grad_kernel: with a small batch the batch reduction dW|db = [h | 1]^T dY has K = B, so a workgroup OWNS a 16 x 64 tile
//      of one layer's [kernel | bias] gradient: it sums over all rows in a fixed order, writes grads and (train mode) applies
//      Adam.  One more workgroup does the closed-form tail (epsilon_p, epsilon, the loss slots, the loss ring); with
//      vaek_train_step_gen further workgroups draw the next batch.  No partial-gradient slabs exist.
//
// Rows past the batch (the last group's padding) carry zero gradients, so launch 2 sums whole padded rows without a mask.
// Every sum has a fixed order: bitwise repeatable from run to run.  No bf16, no atomics.
#include "vaek_internal.h"
#include "rng_dev.h"

namespace vaek {

using f32x4 = __attribute__((ext_vector_type(4))) float;

// Largest batch (rows of this rank) that takes this path: the largest size at which the graph loop was timed against the parent
// commit's layer-by-layer kernels (profiles/mlp3_loop.txt, DESIGN 3.7: batch 100 and 128).  256 and 512 are NOT measured against
// the parent, so they stay on the layer-by-layer kernels; the kernels themselves handle up to 512 rows (launch 2's K = B).
// tests/mlp3_cases.py holds a copy (MAX_BATCH).
constexpr int kMlp3MaxBatch = 128;

constexpr int M3_R = 16;             // samples per workgroup of the chain kernel = MFMA columns
constexpr int M3_NT = 256;           // threads of either kernel
constexpr int M3_W = 256;            // widest hidden layer
constexpr int M3_F = 32;             // widest D / L
constexpr int M3_NL = 8;             // Dense layers: encoder 0 .. 3, decoder 4 .. 7
constexpr int M3_PS = 40;            // floats per partial row: {sum mse terms, sum mu^2, sum d eps, 0}, then L sums of d samples * z1
constexpr int M3_TK = 16, M3_TJ = 64, M3_TB = 64;      // launch 2: tile of [kernel | bias] rows x columns, batch rows per chunk

struct Mlp3Layers {                  // per Dense layer; a_off / g_off: float offsets of its input activation / output gradient
    int n_in[M3_NL], n_out[M3_NL], w_off[M3_NL], a_off[M3_NL], g_off[M3_NL];
    int shift[M3_NL];                // w_off % 4 where dX can read the kernel's rows 16 bytes at a time, else -1 (m3_dense)
};

struct Mlp3ChainArgs {
    const float* x; const float* z1; const float* z2; const float* params;
    float* acts; float* part;
    int B, D, L, Bs;                 // Bs: padded batch = row pitch of the stored images
    float inv_bt, eps_cli;
    int off_epsp, off_eps, e_max;    // e_max: index of the last 16-byte aligned float4 inside the parameters
    Mlp3Layers ly;
    int32_t* step_dev;               // the Adam step counter: advanced here, read by launch 2
    unsigned long long* stamps;      // -DVAEK_M3_STAMPS builds: s_memrealtime at the phase boundaries of workgroup 0
};

#ifdef VAEK_M3_STAMPS
#define M3_STAMP(i)                                                                                          \
    do {                                                                                                     \
        __builtin_amdgcn_sched_barrier(0);                                                                   \
        unsigned long long _t;                                                                               \
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(_t)::"memory"); \
        if (a.stamps && blockIdx.x == 0 && threadIdx.x == 0) a.stamps[i] = _t;                               \
        __builtin_amdgcn_sched_barrier(0);                                                                   \
    } while (0)
#else
#define M3_STAMP(i) do {} while (0)
#endif

struct Mlp3Lds {
    float H[6][M3_W][M3_R];          // the six hidden activations, later their gradients
    float X[M3_F][M3_R], Z1[M3_F][M3_R], Z2[M3_F][M3_R];
    float MU[M3_F][M3_R];            // mu, later d mu
    float SMP[M3_F][M3_R];           // samples
    float XH[M3_F][M3_R];            // x_hat, later dL/dx_hat
    float DS[M3_F][M3_R];            // d samples, later d samples * z1
    float RED[4][4];
};

typedef float (*M3Img)[M3_R];

// out[m][sample] = sum_{k < K} A(m, k) * in[k][sample], m < M, handed to epi(m, sample, sum, bias[m]).
// Forward: A(m, k) = kernel[k][m] (M = n_out, K = n_in); dX: A(m, k) = kernel[m][k] (M = n_in, K = n_out); kernel = P + w_off,
// row pitch n_out.  Wave w owns the 16-unit blocks w, w + 4, .. (NB of them: 1 while M <= 64, else 4).  The operands of 8
// k-steps (a chunk) are fetched while the previous chunk is multiplied (hipcc left alone issues load, wait, v_mfma per step);
// every global load is unconditional at a clamped index, and k outside [0, K) is zeroed on the LDS operand, so a clamped weight
// meets a zero (while the parameters are finite -- 0 * Inf is NaN in the MFMA -- i.e. in any run that has not already diverged).
//   VEC = false: one dword per lane and product, any layout.  Forward, its 16 lanes of a block read 64 contiguous bytes.
//   VEC = true (dX only): a row of the kernel is contiguous along k, so lane (n, kq) loads the 16 bytes
//           kernel[m][32 c + 16 g + 4 kq - s .. + 3] and the k-slots of a chunk are permuted to match (the LDS operand follows).
//           s = w_off % 4 shifts the slots so that the address is 16-byte aligned (the flat layout aligns nothing); needs
//           n_out % 4 == 0.  A 16-byte load that holds one wanted element ends inside the kernel's bias at the latest, so the
//           clamp to e_max (the last aligned 16 bytes of the parameters) only ever moves loads nothing uses.
// Measured (profiles/mlp3_stamps.txt, builds A and B): dX of a 200 x 200 layer 25 us with dword loads (16 rows x 4 bytes per load
// instruction), 9.3 us with VEC.  Tried and backed out, neither moved the forward layers' 9 us (same file, builds B and C): 16-byte
// forward loads along the output units (one load feeding four blocks), and operands three chunks ahead in four register sets.
template <int NB, bool VEC, typename Epi>
__device__ __forceinline__ void m3_dense(const float* __restrict__ P, int w_off, const float* __restrict__ bias, int M, int K, int n_out,
                                         bool fwd, int s, int e_max, const float (*in)[M3_R], int wave, int lane, Epi&& epi) {
    const int n = lane & 15, kq = lane >> 4;
    auto kof = [&](int c, int j) { return VEC ? 32 * c + 16 * (j >> 2) + 4 * kq + (j & 3) - s : 32 * c + 4 * j + kq; };
    int wrow[NB];
    float bia[NB][4];
#pragma unroll
    for (int bi = 0; bi < NB; ++bi) {
        const int m = min(16 * (wave + 4 * bi) + n, M - 1);
        wrow[bi] = w_off + (fwd ? m : m * n_out);
#pragma unroll
        for (int r = 0; r < 4; ++r) bia[bi][r] = bias[min(16 * (wave + 4 * bi) + 4 * kq + r, M - 1)];
    }
    const int sk = fwd ? n_out : 1;
    f32x4 acc[NB];
#pragma unroll
    for (int bi = 0; bi < NB; ++bi) acc[bi] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int nchunks = (K + (VEC ? s : 0) + 31) / 32;
    float av0[NB][8], av1[NB][8], bv0[8], bv1[8];
    auto fetch = [&](float (&av)[NB][8], float (&bv)[8], int c) {
#pragma unroll
        for (int j = 0; j < 8; ++j) bv[j] = in[min(max(kof(c, j), 0), K - 1)][n];
        if constexpr (!VEC) {
#pragma unroll
            for (int j = 0; j < 8; ++j)
#pragma unroll
                for (int bi = 0; bi < NB; ++bi) av[bi][j] = P[wrow[bi] + min(kof(c, j), K - 1) * sk];
        } else {
#pragma unroll
            for (int g = 0; g < 2; ++g)
#pragma unroll
                for (int bi = 0; bi < NB; ++bi) {
                    const int e = min(wrow[bi] + 32 * c + 16 * g + 4 * kq - s, e_max);
                    const f32x4 v = *reinterpret_cast<const f32x4*>(P + e);
#pragma unroll
                    for (int i = 0; i < 4; ++i) av[bi][4 * g + i] = v[i];
                }
        }
    };
    auto mult = [&](float (&av)[NB][8], float (&bv)[8], int c) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = kof(c, j);
            const float b = (k >= 0 && k < K) ? bv[j] : 0.f;
#pragma unroll
            for (int bi = 0; bi < NB; ++bi) acc[bi] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[bi][j], b, acc[bi], 0, 0, 0);
        }
    };
    fetch(av0, bv0, 0);
    for (int c = 0; c < nchunks; c += 2) {
        fetch(av1, bv1, c + 1);                  // past the end: clamped loads, never multiplied
        __builtin_amdgcn_sched_barrier(0);
        mult(av0, bv0, c);
        __builtin_amdgcn_sched_barrier(0);
        fetch(av0, bv0, c + 2);
        __builtin_amdgcn_sched_barrier(0);
        if (c + 1 < nchunks) mult(av1, bv1, c + 1);
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int bi = 0; bi < NB; ++bi)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = 16 * (wave + 4 * bi) + 4 * kq + r;
            if (m < M) epi(m, n, acc[bi][r], bia[bi][r]);
        }
}

__device__ __forceinline__ M3Img m3_in_img(Mlp3Lds& s, int li) {       // input activation of layer li
    return li == 0 ? s.X : li == 4 ? s.SMP : s.H[li < 4 ? li - 1 : li - 2];
}
__device__ __forceinline__ M3Img m3_out_img(Mlp3Lds& s, int li) {      // its output, later the gradient w.r.t. that output
    return li == 3 ? s.MU : li == 7 ? s.XH : s.H[li < 3 ? li : li - 1];
}
// rows [0, n) of an image to the workspace tensor dst [n][Bs], this workgroup's 16 columns
__device__ __forceinline__ void m3_store_img(float* __restrict__ dst, const float (*img)[M3_R], int n, int Bs, int row0, int t) {
    const int cnt = n * M3_R;
    for (int e0 = t; e0 < cnt; e0 += 4 * M3_NT) {          // four independent LDS reads, then the stores
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = (&img[0][0])[min(e0 + u * M3_NT, cnt - 1)];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int e = e0 + u * M3_NT;
            if (e < cnt) dst[(long long)(e >> 4) * Bs + row0 + (e & 15)] = v[u];
        }
    }
}

__global__ __launch_bounds__(M3_NT) void mlp3_chain_kernel(const Mlp3ChainArgs a) {
    extern __shared__ __attribute__((aligned(16))) char m3_smem[];
    Mlp3Lds& s = *reinterpret_cast<Mlp3Lds*>(m3_smem);
    const int t = threadIdx.x, lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int D = a.D, L = a.L, Bs = a.Bs;
    const int row0 = blockIdx.x * M3_R, valid = min(M3_R, a.B - row0);
    const float* const P = a.params;
    if (blockIdx.x == 0 && t == 0 && a.step_dev) a.step_dev[0] += 1;
    M3_STAMP(0);
    // ---- inputs as [feature][sample] images, zero-padded; loads unconditional at clamped indices, selects at the LDS store
    float shl[2];
    {
        float xv[2], z1v[2], z2v[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int e = t + i * M3_NT, c = e >> 4, sm = e & 15;
            const long long row = row0 + min(sm, valid - 1);
            xv[i] = a.x[row * D + min(c, D - 1)]; z1v[i] = a.z1[row * L + min(c, L - 1)]; z2v[i] = a.z2[row * D + min(c, D - 1)];
            shl[i] = P[a.off_epsp + min(c, L - 1)];
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int e = t + i * M3_NT, c = e >> 4;
            (&s.X[0][0])[e] = c < D ? xv[i] : 0.f; (&s.Z1[0][0])[e] = c < L ? z1v[i] : 0.f; (&s.Z2[0][0])[e] = c < D ? z2v[i] : 0.f;
            shl[i] = expf(0.5f * shl[i]);
        }
    }
    const float eps_ld = P[a.off_eps >= 0 ? a.off_eps : 0];
    const float eps = a.off_eps >= 0 ? eps_ld * a.eps_cli : a.eps_cli;
    const float sigma = expf(0.5f * eps), inv_var = expf(-eps);
    float p_mse = 0.f, p_musq = 0.f, p_deps = 0.f;
    __syncthreads();
    M3_STAMP(1);

    // ---- forward: encoder 0 .. 3, reparameterisation, decoder 4 .. 7, ELBO
    for (int li = 0; li < M3_NL; ++li) {
        const int n_in = a.ly.n_in[li], n_out = a.ly.n_out[li];
        const int w_off = a.ly.w_off[li];
        const M3Img in = m3_in_img(s, li), out = m3_out_img(s, li);
        m3_store_img(a.acts + a.ly.a_off[li], in, n_in, Bs, row0, t);
        const bool relu = li != 3 && li != 7;
        auto epi = [&](int m, int n, float v, float b) { v += b; out[m][n] = relu ? fmaxf(v, 0.f) : v; };
        const float* const bias = P + w_off + n_in * n_out;
        if (n_out <= 64) m3_dense<1, false>(P, w_off, bias, n_out, n_in, n_out, true, 0, a.e_max, in, wave, lane, epi);
        else m3_dense<4, false>(P, w_off, bias, n_out, n_in, n_out, true, 0, a.e_max, in, wave, lane, epi);
        __syncthreads();
        if (li == 3) {               // samples = mu + e^{lv/2} z1
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int e = t + i * M3_NT, c = e >> 4, sm = e & 15;
                if (c < L) {
                    const float mu = (&s.MU[0][0])[e];
                    (&s.SMP[0][0])[e] = fmaf(shl[i], (&s.Z1[0][0])[e], mu);
                    if (sm < valid) p_musq = fmaf(mu, mu, p_musq);
                }
            }
            __syncthreads();
        }
        M3_STAMP(2 + li);
    }
    // ---- ELBO, elementwise over [feature][sample]: decoder noise, residual, dL/dx_hat (zero for rows past the batch), scalar sums
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int e = t + i * M3_NT, c = e >> 4, sm = e & 15;
        const bool in = sm < valid && c < D;
        const float z2v = (&s.Z2[0][0])[e];
        const float res = (&s.XH[0][0])[e] + z2v * sigma - (&s.X[0][0])[e];
        (&s.XH[0][0])[e] = in ? res * inv_var * a.inv_bt : 0.f;
        if (in) {
            const float q = 0.5f * res * res * inv_var;
            p_mse += q;
            p_deps += -q + 0.5f * sigma * z2v * res * inv_var;
        }
    }
    __syncthreads();
    M3_STAMP(10);
    m3_store_img(a.acts + a.ly.g_off[7], s.XH, D, Bs, row0, t);

    // ---- backward: dX of layer li from the gradient image of its output, through the relu of the layer below, in place
    for (int li = M3_NL - 1; li >= 1; --li) {
        const int n_in = a.ly.n_in[li], n_out = a.ly.n_out[li];
        const int w_off = a.ly.w_off[li], sh = a.ly.shift[li];
        const M3Img dy = m3_out_img(s, li);
        const M3Img dst = li == 4 ? s.DS : m3_out_img(s, li - 1);
        const bool mask = li != 4;
        auto epi = [&](int m, int n, float v, float) { dst[m][n] = (!mask || dst[m][n] > 0.f) ? v : 0.f; };
        if (sh >= 0 && n_in <= 64) m3_dense<1, true>(P, w_off, P, n_in, n_out, n_out, false, sh, a.e_max, dy, wave, lane, epi);
        else if (sh >= 0) m3_dense<4, true>(P, w_off, P, n_in, n_out, n_out, false, sh, a.e_max, dy, wave, lane, epi);
        else if (n_in <= 64) m3_dense<1, false>(P, w_off, P, n_in, n_out, n_out, false, 0, a.e_max, dy, wave, lane, epi);
        else m3_dense<4, false>(P, w_off, P, n_in, n_out, n_out, false, 0, a.e_max, dy, wave, lane, epi);
        __syncthreads();
        if (li == 4) {               // d mu = d samples + mu / Bt (zero for rows past the batch); DS becomes d samples * z1
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int e = t + i * M3_NT, c = e >> 4, sm = e & 15;
                if (c < L) {
                    const float ds = (&s.DS[0][0])[e];
                    (&s.MU[0][0])[e] = sm < valid ? fmaf((&s.MU[0][0])[e], a.inv_bt, ds) : 0.f;
                    (&s.DS[0][0])[e] = sm < valid ? ds * (&s.Z1[0][0])[e] : 0.f;
                }
            }
            __syncthreads();
        }
        m3_store_img(a.acts + a.ly.g_off[li - 1], m3_out_img(s, li - 1), a.ly.n_out[li - 1], Bs, row0, t);
        M3_STAMP(10 + (M3_NL - li));
    }

    // ---- this workgroup's partial row: the three scalar sums (lanes by xor-shuffle, the four waves in order), epsilon_p's sums
    float* const row = a.part + (long long)blockIdx.x * M3_PS;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        p_mse += __shfl_xor(p_mse, o, 64); p_musq += __shfl_xor(p_musq, o, 64); p_deps += __shfl_xor(p_deps, o, 64);
    }
    if (lane == 0) { s.RED[wave][0] = p_mse; s.RED[wave][1] = p_musq; s.RED[wave][2] = p_deps; }
    __syncthreads();
    if (t < 3) row[t] = (s.RED[0][t] + s.RED[1][t]) + (s.RED[2][t] + s.RED[3][t]);
    if (t == 3) row[3] = 0.f;
    if (t < L) {
        float g = 0.f;
#pragma unroll
        for (int r = 0; r < M3_R; ++r) g += s.DS[t][r];
        row[4 + t] = g;
    }
    M3_STAMP(18);
}

// ---- launch 2 ------------------------------------------------------------------------------------------------------------------
struct Mlp3GradArgs {
    const float* acts; const float* part; int G, Bs;
    Mlp3Layers ly; int tile0[M3_NL + 1];          // first tile of each layer; tile0[8] = tiles in all
    int P, off_epsp, off_eps, L, D;
    const float* params; float eps_cli, rows_over_bt, inv_bt, rows;
    float* grads;
    float* params_rw; float* m; float* v; const int32_t* step_dev; float lr;      // params_rw == nullptr: gradients only
    float* loss_hist; long long loss_hist_cap;    // optional: loss of Adam step t -> loss_hist[(t-1) % cap]
};

__device__ __forceinline__ float m3_wsum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// epsilon_p, epsilon, the three loss slots: closed-form terms exactly as fused_finalize_block (fused_small.hip) has them.
// One wave; every load is issued before the first store, so the parameters it updates are read before they are written.
__device__ __forceinline__ void m3_tail(const Mlp3GradArgs& a) {
    const int t = threadIdx.x;
    if (t >= 64) return;
    const int P = a.P, L = a.L, G = a.G;
    // lane < L: epsilon_p[lane]; lane 32: epsilon; lanes 33 .. 36: loss, mean Dkl, mean mse, 0
    const int idx = t < L ? a.off_epsp + t : t == 32 ? a.off_eps : (t >= 33 && t <= 36) ? P + (t - 33) : -1;
    const bool live = idx >= 0;
    const bool is_lv = t < L;
    const int ipc = (live && idx < P) ? idx : 0;
    const float* const ps = a.params_rw ? a.params_rw : a.params;
    float p_old = ps[ipc], m_old = (a.m ? a.m : a.params)[ipc], v_old = (a.v ? a.v : a.params)[ipc];
    const int tstep = a.step_dev ? a.step_dev[0] : 0;
    const float eps_ld = a.params[a.off_eps >= 0 ? a.off_eps : 0];
    float s_mse = 0.f, s_musq = 0.f, s_deps = 0.f, g = 0.f;
    const int tl = is_lv ? t : 0;
    for (int q = 0; q < G; ++q) {
        const float* const row = a.part + (long long)q * M3_PS;
        s_mse += row[0]; s_musq += row[1]; s_deps += row[2]; g += row[4 + tl];
    }
    const float lv_own = is_lv ? p_old : 0.f;
    const float e_lv = expf(lv_own), e_hlv = expf(0.5f * lv_own);
    const float klc = m3_wsum(is_lv ? 1.f + lv_own - e_lv : 0.f);
    const float bc1 = -expm1f((float)tstep * -0.10536051565782628f);
    const float bc2 = -expm1f((float)tstep * -0.0010005003335835335f);
    if (!live) return;
    if (is_lv) {
        g = 0.5f * e_hlv * g - 0.5f * (1.f - e_lv) * a.rows_over_bt;
    } else if (t == 32) {
        g = a.eps_cli * (s_deps + 0.5f * a.rows * (float)a.D) * a.inv_bt;
    } else if (idx < P + 3) {
        const float eps = a.off_eps >= 0 ? eps_ld * a.eps_cli : a.eps_cli;
        const float dkl = (0.5f * s_musq - 0.5f * a.rows * klc) * a.inv_bt;
        const float mse = (s_mse + 0.5f * a.rows * (float)a.D * (kLog2Pi + eps)) * a.inv_bt;
        g = idx == P ? dkl + mse : (idx == P + 1 ? dkl : mse);
    } else {
        g = 0.f;
    }
    a.grads[idx] = g;
    if (idx == P && a.loss_hist) a.loss_hist[(long long)(tstep - 1) % a.loss_hist_cap] = g;
    if (a.params_rw && idx < P) {
        adam_apply_f(p_old, g, m_old, v_old, a.lr, bc1, bc2);
        a.params_rw[idx] = p_old; a.m[idx] = m_old; a.v[idx] = v_old;
    }
}

__global__ __launch_bounds__(M3_NT) void mlp3_grad_kernel(const Mlp3GradArgs a, const BatchArgs b) {
    __shared__ float As[M3_TK][M3_TB];           // [kernel row | bias][batch row]
    __shared__ float Gs[M3_TB][M3_TJ + 1];       // [batch row][column]
    const int t = threadIdx.x, lane = t & 63, kq = __builtin_amdgcn_readfirstlane(t >> 6);
    const int bid = blockIdx.x, ntiles = a.tile0[M3_NL];
    if (bid > ntiles) {              // vaek_train_step_gen: the next step's batch does not depend on the weights
        const unsigned step = make_batch_step(b);
        make_batch_items(b, step, (long long)(bid - ntiles - 1) * M3_NT + t);
        make_batch_advance(b, step, bid == ntiles + 1 && t == 0);
        return;
    }
    if (bid == ntiles) { m3_tail(a); return; }
    int li = 0;
#pragma unroll
    for (int i = 1; i < M3_NL; ++i) li = bid >= a.tile0[i] ? i : li;
    const int n_in = a.ly.n_in[li], n_out = a.ly.n_out[li], Bs = a.Bs;
    const int tiles_j = (n_out + M3_TJ - 1) / M3_TJ, rel = bid - a.tile0[li];
    const int k0 = M3_TK * (rel / tiles_j), j0 = M3_TJ * (rel % tiles_j);
    const float* const ap = a.acts + a.ly.a_off[li];
    const float* const gp = a.acts + a.ly.g_off[li];
    // this thread's four outputs: rows k0 + 4 kq + i (row n_in is the bias), column j0 + lane; Adam state loaded up front
    const int j = j0 + lane;
    int idx[4]; bool ok[4];
    float p_old[4], m_old[4], v_old[4];
    const float* const ps = a.params_rw ? a.params_rw : a.params;
    const float* const ms = a.m ? a.m : a.params;
    const float* const vs = a.v ? a.v : a.params;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = k0 + 4 * kq + i;
        ok[i] = k <= n_in && j < n_out;
        idx[i] = a.ly.w_off[li] + (ok[i] ? k * n_out + j : 0);
        p_old[i] = ps[idx[i]]; m_old[i] = ms[idx[i]]; v_old[i] = vs[idx[i]];
    }
    const int tstep = a.step_dev ? a.step_dev[0] : 0;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c0 = 0; c0 < Bs; c0 += M3_TB) {
        const bool in = c0 + lane < Bs;
        const int bc = min(c0 + lane, Bs - 1);
        float gv[16], av[4];
#pragma unroll
        for (int r = 0; r < 16; ++r) gv[r] = gp[(long long)min(j0 + 16 * kq + r, n_out - 1) * Bs + bc];
#pragma unroll
        for (int r = 0; r < 4; ++r) av[r] = ap[(long long)min(k0 + 4 * kq + r, n_in - 1) * Bs + bc];
        __syncthreads();             // the previous chunk is no longer read
#pragma unroll
        for (int r = 0; r < 16; ++r) Gs[lane][16 * kq + r] = in ? gv[r] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) As[4 * kq + r][lane] = !in ? 0.f : (k0 + 4 * kq + r == n_in ? 1.f : av[r]);
        __syncthreads();
#pragma unroll 16
        for (int r = 0; r < M3_TB; ++r) {
            const float g = Gs[r][lane];
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] = fmaf(As[4 * kq + i][r], g, acc[i]);
        }
    }
    const float bc1 = -expm1f((float)tstep * -0.10536051565782628f);
    const float bc2 = -expm1f((float)tstep * -0.0010005003335835335f);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (ok[i]) {
            a.grads[idx[i]] = acc[i];
            if (a.params_rw) {
                adam_apply_f(p_old[i], acc[i], m_old[i], v_old[i], a.lr, bc1, bc2);
                a.params_rw[idx[i]] = p_old[i]; a.m[idx[i]] = m_old[i]; a.v[idx[i]] = v_old[i];
            }
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
bool mlp3_supported(const vaek_ctx* c) {
    const vaek_config& f = c->cfg;
    if (f.dtype != VAEK_F32 || f.sigmoid_decoder || f.force_generic || f.n_enc_hidden != 3 || f.n_dec_hidden != 3) return false;
    for (int i = 0; i < 3; ++i)
        if (f.enc_hidden[i] < 64 || f.enc_hidden[i] > M3_W || f.dec_hidden[i] < 64 || f.dec_hidden[i] > M3_W) return false;
    return c->D <= M3_F && c->L <= M3_F && c->B <= kMlp3MaxBatch;
}

static int mlp3_groups(const vaek_ctx* c) { return (c->B + M3_R - 1) / M3_R; }

// the layers with their places in the workspace region: 16 images of [units][padded batch], then the partial rows
static size_t mlp3_layout(const vaek_ctx* c, Mlp3Layers* ly) {
    const int Bs = mlp3_groups(c) * M3_R;
    size_t off = 0;
    int li = 0;
    for (const Net* net : {&c->enc, &c->dec})
        for (const Layer& l : net->layers) {
            if (ly) { ly->n_in[li] = l.n_in; ly->n_out[li] = l.n_out; ly->w_off[li] = (int)l.w_off; ly->a_off[li] = (int)off; }
            off += (size_t)l.n_in * Bs;
            if (ly) ly->g_off[li] = (int)off;
            off += (size_t)l.n_out * Bs;
            ++li;
        }
    return off;
}

size_t mlp3_workspace_bytes(const vaek_ctx* c) {
    if (!mlp3_supported(c)) return 0;
    return (mlp3_layout(c, nullptr) + (size_t)mlp3_groups(c) * M3_PS) * sizeof(float);
}

int mlp3_train_step(vaek_ctx* c, float* params, float* grads, float* m, float* v, int32_t* step_dev, const float* x, const float* z1,
                    const float* z2, float lr, bool apply_adam, void* ws, hipStream_t st, const BatchArgs* gen) {
    if (!mlp3_supported(c) || c->enc.layers.size() != 4 || c->dec.layers.size() != 4) {
        set_error("mlp3 path not available for this configuration");
        return VAEK_ERR_INVALID;
    }
    float* const region = reinterpret_cast<float*>(static_cast<char*>(ws) + c->ws_mlp3);
    const int G = mlp3_groups(c);
    Mlp3ChainArgs a{};
    const size_t acts_floats = mlp3_layout(c, &a.ly);
    a.x = x; a.z1 = z1; a.z2 = z2; a.params = params; a.acts = region; a.part = region + acts_floats;
    a.B = c->B; a.D = c->D; a.L = c->L; a.Bs = G * M3_R;
    a.inv_bt = (float)(1.0 / (double)c->Bt); a.eps_cli = c->cfg.eps_cli;
    a.off_epsp = (int)c->off_epsp; a.off_eps = (int)c->off_eps; a.e_max = (int)((c->P - 4) & ~3ll);
    for (int li = 0; li < M3_NL; ++li)
#ifdef VAEK_M3_NO_VEC                // diagnostic build (tools/m3_stamps.sh): dX with dword loads, for the A/B in profiles/mlp3_stamps.txt
        a.ly.shift[li] = -1;
#else
        a.ly.shift[li] = ((reinterpret_cast<uintptr_t>(params) & 15) == 0 && a.ly.n_out[li] % 4 == 0) ? a.ly.w_off[li] % 4 : -1;
#endif
    a.step_dev = step_dev; a.stamps = c->dbg_stamps;
    static thread_local PerDeviceOnce attr_set;
    if (attr_set.need()) {
        VAEK_HIP_CHECK(hipFuncSetAttribute((const void*)mlp3_chain_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(Mlp3Lds)));
        attr_set.mark();
    }
    {
        ProfScope ps("fused_mlp3_chain", st);
        launch_k(ps, mlp3_chain_kernel, dim3((unsigned)G), dim3(M3_NT), sizeof(Mlp3Lds), st, a);
        VAEK_HIP_CHECK(hipGetLastError());
    }
    Mlp3GradArgs f{};
    f.acts = a.acts; f.part = a.part; f.G = G; f.Bs = a.Bs; f.ly = a.ly;
    int ntiles = 0;
    for (int li = 0; li < M3_NL; ++li) {
        f.tile0[li] = ntiles;
        ntiles += ((a.ly.n_in[li] + 1 + M3_TK - 1) / M3_TK) * ((a.ly.n_out[li] + M3_TJ - 1) / M3_TJ);
    }
    f.tile0[M3_NL] = ntiles;
    f.P = (int)c->P; f.off_epsp = (int)c->off_epsp; f.off_eps = (int)c->off_eps; f.L = c->L; f.D = c->D;
    f.params = params; f.eps_cli = c->cfg.eps_cli;
    f.rows_over_bt = (float)((double)c->B / (double)c->Bt); f.inv_bt = a.inv_bt; f.rows = (float)c->B;
    f.grads = grads;
    f.params_rw = apply_adam ? params : nullptr; f.m = apply_adam ? m : nullptr; f.v = apply_adam ? v : nullptr;
    f.step_dev = step_dev; f.lr = lr;
    f.loss_hist = (apply_adam && c->cfg.world == 1) ? c->loss_hist : nullptr; f.loss_hist_cap = c->loss_hist_cap;
    BatchArgs none{};
    const long long ngen = gen ? (make_batch_item_count(*gen) + M3_NT - 1) / M3_NT : 0;
    ProfScope ps(gen ? "fused_mlp3_grads_adam_gen" : apply_adam ? "fused_mlp3_grads_adam" : "fused_mlp3_grads", st);
    launch_k(ps, mlp3_grad_kernel, dim3((unsigned)(ntiles + 1 + ngen)), dim3(M3_NT), 0, st, f, gen ? *gen : none);
    VAEK_HIP_CHECK(hipGetLastError());
    return VAEK_OK;
}

}  // namespace vaek
