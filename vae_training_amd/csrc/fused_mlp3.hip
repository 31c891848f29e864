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
//
// THE REPLICA FORM (vaek_train_step_gen_replicas).  Neither launch has a counter, a wait or an atomic, and workgroups of different
// models share nothing, so N independent models of one shape are the same two launches with gridDim.y = N: blockIdx.y = r runs
// the very body of the solo kernels (mlp3_chain_body.inc, mlp3_grad_body.inc) on replica r's slices of the caller's stacks.
//   Defining property: what replica r is left with -- params, m, v, grads, step_dev[r], its ring, its next batch, its counter pair
//           -- is BITWISE what vaek_train_step_gen (no-draw form: vaek_train_step) leaves when called alone on those slices.
//   Stride rule: state_stride % 4 == 0.  The VEC form of dX permutes the k-slots of a chunk, so it is not bitwise the dword form,
//           and the host picks it per layer from the BASE pointer's alignment; with that stride every replica's pointer has the
//           base's alignment and takes the form a solo call on its slice would take.
//   Workspace: the call's own buffer, one region of mlp3_replica_region_floats (the solo region rounded up to whole float4s) per
//           replica; the context's workspace and ring are not used.
//   Refusals (api.hip, before any launch): n outside 1 .. 256, state_stride < P or % 4 != 0, grads_stride < grad_len, a ring
//           with cap < 1, a_stride < 0, NULL seeds / counter in the drawing form, some but not all _next pointers NULL,
//           dd / did > 16, kind outside 0 .. 2 in the drawing form, a missing / misaligned workspace, a wrong struct_size, a
//           context off the mlp3 path or with world > 1.
//   The rule of linear_resident.hip, re-read: seeds[r], lrs[r] and counter[2 r + which] are tables or slots this launch does not
//           write at that address; step_dev[r] is written by the chain launch and read by the NEXT launch; nothing stored inside a
//           launch is read back inside it through a uniform-address or const __restrict__ load.
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

// What the replica form adds to the launch arguments of both kernels (vaek_train_step_gen_replicas): blockIdx.y = r trains replica r.
// The tables are never written by either launch, so the uniform-address loads of seeds[r] / lrs[r] below are safe from the scalar
// cache (the rule of linear_resident.hip); step_dev[r] is written by the chain launch and read by the NEXT launch.
struct Mlp3ReplicaArgs {
    long long state_stride, grads_stride, a_stride, region_floats;     // floats between two replicas' params / m / v, grads, A, workspace region
    const unsigned long long* seeds;                                   // [n], or nullptr in the no-draw form
    const float* lrs;                                                  // [n], or nullptr: Mlp3GradArgs::lr for every replica
};

// Replica r's view of the chain launch's arguments: Mlp3ChainArgs member for member, with its slices of the caller's buffers in place
// of the bases.  The layer table stays where it is, in the kernel-argument segment: a private copy indexed by the layer loop would
// live in scratch memory.  Slices of different replicas are disjoint (the host checks the strides against the lengths), and a
// workgroup reads and writes only its own.
struct Mlp3ChainSlice {
    const float* x; const float* z1; const float* z2; const float* params;
    float* acts; float* part;
    int B, D, L, Bs;
    float inv_bt, eps_cli;
    int off_epsp, off_eps, e_max;
    const Mlp3Layers& ly;
    int32_t* step_dev;
    unsigned long long* stamps;
};
__device__ __forceinline__ Mlp3ChainSlice m3_chain_slice(const Mlp3ChainArgs& a, const Mlp3ReplicaArgs& rp) {
    const long long r = blockIdx.y;
    return {a.x + r * a.B * a.D, a.z1 + r * a.B * a.L, a.z2 + r * a.B * a.D, a.params + r * rp.state_stride,
            a.acts + r * rp.region_floats, a.part + r * rp.region_floats,
            a.B, a.D, a.L, a.Bs, a.inv_bt, a.eps_cli, a.off_epsp, a.off_eps, a.e_max, a.ly, a.step_dev + r, a.stamps};
}

// The body of both forms is ONE text, mlp3_chain_body.inc, written in terms of `a`: the solo kernel is that text on its launch
// arguments as given (the kernel it was before the replica form existed, token for token); the replica kernel is a first statement
// that slices the arguments, then the same text.  The body has no cross-workgroup state -- no counter, no wait, no atomic -- so
// replicas share nothing but the code and the launch-wide arguments; blockIdx.x keeps its meaning within a replica.
__global__ __launch_bounds__(M3_NT) void mlp3_chain_kernel(const Mlp3ChainArgs a) {
#include "mlp3_chain_body.inc"
}

__global__ __launch_bounds__(M3_NT) void mlp3_chain_replicas_kernel(const Mlp3ChainArgs a0, const Mlp3ReplicaArgs rp) {
    const Mlp3ChainSlice a = m3_chain_slice(a0, rp);
#include "mlp3_chain_body.inc"
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
template <typename Args>             // Mlp3GradArgs, or a replica's Mlp3GradSlice
__device__ __forceinline__ void m3_tail(const Args& a) {
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

// Replica r's view of launch 2's arguments (Mlp3GradArgs member for member, the layer and tile tables left in the kernel-argument
// segment) and its generator arguments: its slices, its learning rate, seed, dataset matrix and counter pair.
struct Mlp3GradSlice {
    const float* acts; const float* part; int G, Bs;
    const Mlp3Layers& ly; const int (&tile0)[M3_NL + 1];
    int P, off_epsp, off_eps, L, D;
    const float* params; float eps_cli, rows_over_bt, inv_bt, rows;
    float* grads;
    float* params_rw; float* m; float* v; const int32_t* step_dev; float lr;
    float* loss_hist; long long loss_hist_cap;
};
struct Mlp3GradSlices { Mlp3GradSlice a; BatchArgs b; };
__device__ __forceinline__ Mlp3GradSlices m3_grad_slice(const Mlp3GradArgs& a, const BatchArgs& b0, const Mlp3ReplicaArgs& rp) {
    const long long r = blockIdx.y;
    BatchArgs b = b0;
    if (b.z1) {                      // the drawing form (the no-draw form launches no generator workgroup: b is all zero, seeds may be NULL)
        b.x += r * b.rows * b.D; b.z1 += r * b.rows * b.L; b.z2 += r * b.rows * b.D;
        b.seed = rp.seeds[r];
        if (b.A) b.A += r * rp.a_stride;
        b.counter += 2 * r;
    }
    return {{a.acts + r * rp.region_floats, a.part + r * rp.region_floats, a.G, a.Bs, a.ly, a.tile0, a.P, a.off_epsp, a.off_eps, a.L, a.D,
             a.params + r * rp.state_stride, a.eps_cli, a.rows_over_bt, a.inv_bt, a.rows, a.grads + r * rp.grads_stride,
             a.params_rw + r * rp.state_stride, a.m + r * rp.state_stride, a.v + r * rp.state_stride, a.step_dev + r,
             rp.lrs ? rp.lrs[r] : a.lr, a.loss_hist ? a.loss_hist + r * a.loss_hist_cap : nullptr, a.loss_hist_cap},
            b};
}

// As the chain kernel: one body text (mlp3_grad_body.inc, in terms of `a` and `b`) for the solo kernel, which is the kernel it was,
// and for the replica kernel behind its slicing statement.  blockIdx.x keeps its meaning within a replica: tiles, the tail, the
// generator items.
__global__ __launch_bounds__(M3_NT) void mlp3_grad_kernel(const Mlp3GradArgs a, const BatchArgs b) {
#include "mlp3_grad_body.inc"
}

__global__ __launch_bounds__(M3_NT) void mlp3_grad_replicas_kernel(const Mlp3GradArgs a0, const BatchArgs b0, const Mlp3ReplicaArgs rp) {
    const auto [a, b] = m3_grad_slice(a0, b0, rp);
#include "mlp3_grad_body.inc"
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

// Both forms of the step.  rep == nullptr: vaek_train_step* on the context's workspace region and ring (the solo kernels, grid.y = 1).
// rep != nullptr: n replicas, blockIdx.y = r, on the call's own workspace `ws` (n regions of mlp3_replica_region_floats) and the
// caller's rings; always a train step.
struct Mlp3ReplicaHost { int n; Mlp3ReplicaArgs rp; float* loss_hist; long long loss_hist_cap; };

static int mlp3_step_impl(vaek_ctx* c, float* params, float* grads, float* m, float* v, int32_t* step_dev, const float* x, const float* z1,
                          const float* z2, float lr, bool apply_adam, void* ws, hipStream_t st, const BatchArgs* gen,
                          const Mlp3ReplicaHost* rep) {
    if (!mlp3_supported(c) || c->enc.layers.size() != 4 || c->dec.layers.size() != 4) {
        set_error("mlp3 path not available for this configuration");
        return VAEK_ERR_INVALID;
    }
    float* const region = rep ? static_cast<float*>(ws) : reinterpret_cast<float*>(static_cast<char*>(ws) + c->ws_mlp3);
    const int G = mlp3_groups(c);
    Mlp3ChainArgs a{};
    const size_t acts_floats = mlp3_layout(c, &a.ly);
    a.x = x; a.z1 = z1; a.z2 = z2; a.params = params; a.acts = region; a.part = region + acts_floats;
    a.B = c->B; a.D = c->D; a.L = c->L; a.Bs = G * M3_R;
    a.inv_bt = (float)(1.0 / (double)c->Bt); a.eps_cli = c->cfg.eps_cli;
    a.off_epsp = (int)c->off_epsp; a.off_eps = (int)c->off_eps; a.e_max = (int)((c->P - 4) & ~3ll);
    // (replicas: state_stride % 4 == 0, so every replica's parameters have the base's alignment and take the form chosen here)
    for (int li = 0; li < M3_NL; ++li)
#ifdef VAEK_M3_NO_VEC                // diagnostic build (tools/m3_stamps.sh): dX with dword loads, for the A/B in profiles/mlp3_stamps.txt
        a.ly.shift[li] = -1;
#else
        a.ly.shift[li] = ((reinterpret_cast<uintptr_t>(params) & 15) == 0 && a.ly.n_out[li] % 4 == 0) ? a.ly.w_off[li] % 4 : -1;
#endif
    a.step_dev = step_dev; a.stamps = rep ? nullptr : c->dbg_stamps;
    static thread_local PerDeviceOnce attr_set[2];
    VAEK_HIP_CHECK(set_max_dynamic_lds(attr_set[rep ? 1 : 0], rep ? (const void*)mlp3_chain_replicas_kernel : (const void*)mlp3_chain_kernel,
                                       sizeof(Mlp3Lds)));
    const unsigned ny = rep ? (unsigned)rep->n : 1u;
    {
        ProfScope ps(rep ? "fused_mlp3_chain_replicas" : "fused_mlp3_chain", st);
        if (rep) launch_k(ps, mlp3_chain_replicas_kernel, dim3((unsigned)G, ny), dim3(M3_NT), sizeof(Mlp3Lds), st, a, rep->rp);
        else launch_k(ps, mlp3_chain_kernel, dim3((unsigned)G), dim3(M3_NT), sizeof(Mlp3Lds), st, a);
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
    if (rep) {                       // the caller's rings, never the context's
        f.loss_hist = rep->loss_hist; f.loss_hist_cap = rep->loss_hist ? rep->loss_hist_cap : 0;
    } else {
        f.loss_hist = (apply_adam && c->cfg.world == 1) ? c->loss_hist : nullptr; f.loss_hist_cap = c->loss_hist_cap;
    }
    BatchArgs none{};
    const long long ngen = gen ? (make_batch_item_count(*gen) + M3_NT - 1) / M3_NT : 0;
    const unsigned nx = (unsigned)(ntiles + 1 + ngen);
    if (rep) {
        ProfScope ps(gen ? "fused_mlp3_grads_adam_gen_replicas" : "fused_mlp3_grads_adam_replicas", st);
        launch_k(ps, mlp3_grad_replicas_kernel, dim3(nx, ny), dim3(M3_NT), 0, st, f, gen ? *gen : none, rep->rp);
    } else {
        ProfScope ps(gen ? "fused_mlp3_grads_adam_gen" : apply_adam ? "fused_mlp3_grads_adam" : "fused_mlp3_grads", st);
        launch_k(ps, mlp3_grad_kernel, dim3(nx), dim3(M3_NT), 0, st, f, gen ? *gen : none);
    }
    VAEK_HIP_CHECK(hipGetLastError());
    return VAEK_OK;
}

int mlp3_train_step(vaek_ctx* c, float* params, float* grads, float* m, float* v, int32_t* step_dev, const float* x, const float* z1,
                    const float* z2, float lr, bool apply_adam, void* ws, hipStream_t st, const BatchArgs* gen) {
    return mlp3_step_impl(c, params, grads, m, v, step_dev, x, z1, z2, lr, apply_adam, ws, st, gen, nullptr);
}

// ---- the replica form: vaek_train_step_gen_replicas ---------------------------------------------------------------------------
// 256 replicas = 1792 chain workgroups at batch 100, seven rounds on the MI355X's 256 CUs: a cap that bounds the length of one launch
// on a shared machine, not a tuned value.  36 replicas fill the first round; more is legal, the extra workgroups queue.
constexpr int kMlp3MaxReplicas = 256;
int mlp3_max_replicas() { return kMlp3MaxReplicas; }

// floats of one replica's region of the call's OWN workspace: the solo region, rounded up to whole float4s so that every replica's
// region keeps the 16-byte alignment of the base
size_t mlp3_replica_region_floats(const vaek_ctx* c) { return ((mlp3_workspace_bytes(c) / sizeof(float)) + 3) & ~(size_t)3; }
size_t mlp3_replicas_workspace_bytes(const vaek_ctx* c, int n) { return (size_t)n * mlp3_replica_region_floats(c) * sizeof(float); }

int mlp3_train_step_replicas(vaek_ctx* c, float* params, float* grads, float* m, float* v, int32_t* step_dev, const float* x,
                             const float* z1, const float* z2, float lr, void* ws, hipStream_t st, const BatchArgs* gen, const vaek_replicas& r) {
    Mlp3ReplicaHost rep{};
    rep.n = r.n;
    rep.rp.state_stride = r.state_stride; rep.rp.grads_stride = r.grads_stride; rep.rp.a_stride = r.a_stride;
    rep.rp.region_floats = (long long)mlp3_replica_region_floats(c);
    rep.rp.seeds = reinterpret_cast<const unsigned long long*>(r.seeds); rep.rp.lrs = r.lrs;
    rep.loss_hist = r.loss_hist; rep.loss_hist_cap = r.loss_hist_cap;
    return mlp3_step_impl(c, params, grads, m, v, step_dev, x, z1, z2, lr, true, ws, st, gen, &rep);
}

}  // namespace vaek
