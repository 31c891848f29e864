// The device text of vaek_train_steps (linear_moments.hip: what it computes and why) that its two translation units share: the
// launch's arguments, the streamer pieces, the reducers, both updaters and the two kernel templates.  Each unit instantiates its
// own kernels -- linear_moments.hip the three-block ones and the launch-per-step form, linear_moments4.hip the four-block persistent
// ones: in one device module the four-block kernels change how the three-block ones are compiled (module-wide attribute
// inference) and the metric's launch slows down.
#pragma once
#include <type_traits>

#include "comm_dev.h"
#include "rng_dev.h"
#include "vaek_internal.h"

namespace vaek {

using f32x4 = __attribute__((ext_vector_type(4))) float;
using d2 = __attribute__((ext_vector_type(2))) double;
typedef __attribute__((address_space(3))) void lds_void_t;
typedef const __attribute__((address_space(1))) void glb_void_t;

constexpr int LNT = 512, LNW = LNT / 64;          // threads / waves per workgroup, every role
constexpr int kLinMaxPersist = 64;                // batches a persistent launch streams
// Launches of ONE call are chained: a launch that is not the call's last leaves its last batch to the next launch's reducers and
// its last kLinCarry = 4 to the next launch's updater (the launch-per-step form shifts by one and two), so that launch starts reducing
// and updating at once, while its streamers fill, and all three roles end together.  Batch n of a call lives in slot n % kLinSlots
// (partial images, M, arrival counters): a launch's 64 streamed batches and the kLinCarry carried into it never share a slot.
// kLinCarry: the batches a launch leaves to the next launch's updater.  All but the last of them are reduced already, so that
// updater has kLinCarry - 1 steps of ready work (and one more as soon as its own reducers have run once) while its streamers
// fill their pipeline: the new launch's first own batch is reduced ~13 us after entry, its second ~22 us.  With 2 the updater
// waited twice in a later launch's first 28 us; with 4 it steps at its own pace from entry (profiles/lin_pace_roles.txt).
constexpr int kLinCarry = 4, kLinSlots = kLinMaxPersist + kLinCarry;
static_assert(kLinCarry >= 2 && kLinCarry < kLinMaxPersist, "the updater follows the reducers, which follow the streamers by one batch");
struct LinWindow { int first, count; };
struct LinWindows { LinWindow stream, reduce, update; };
// the batch windows of launch j of a call of K steps
constexpr LinWindows lin_windows(int K, int j) {
    const int s0 = kLinMaxPersist * j, s1 = s0 + kLinMaxPersist < K ? s0 + kLinMaxPersist : K;
    const bool last = s1 == K;
    const int r0 = s0 >= 1 ? s0 - 1 : 0, u0 = s0 >= kLinCarry ? s0 - kLinCarry : 0;
    return LinWindows{{s0, s1 - s0}, {r0, (last ? K : s1 - 1) - r0}, {u0, (last ? K : s1 - kLinCarry) - u0}};
}
constexpr int lin_launches(int K) { return (K + kLinMaxPersist - 1) / kLinMaxPersist; }
// every role covers [0, K) exactly once, in order; no role takes more batches than it may; a launch's live batches fit the slots
constexpr bool lin_windows_ok(int K) {
    int s = 0, r = 0, u = 0;
    for (int j = 0; j < lin_launches(K); ++j) {
        const LinWindows w = lin_windows(K, j);
        if (w.stream.first != s || w.reduce.first != r || w.update.first != u) return false;
        if (w.stream.count < 1 || w.stream.count > kLinMaxPersist || w.reduce.count < 1 || w.update.count < 1) return false;
        s += w.stream.count; r += w.reduce.count; u += w.update.count;
        if (r > s || u > r || s - w.update.first > kLinSlots) return false;      // nobody ahead of its producer; live batches <= slots
    }
    return s == K && r == K && u == K;
}
static_assert(lin_windows_ok(1) && lin_windows_ok(2) && lin_windows_ok(64) && lin_windows_ok(65) && lin_windows_ok(66) && lin_windows_ok(128) &&
              lin_windows_ok(129) && lin_windows_ok(130) && lin_windows_ok(132) && lin_windows_ok(960), "launch windows of a vaek_train_steps call");
static_assert(lin_windows(64, 0).update.count == 64 && lin_windows(130, 1).update.first == 64 - kLinCarry && lin_windows(130, 1).reduce.first == 63 &&
              lin_windows(130, 2).update.count == 2 + kLinCarry && lin_windows(65, 0).update.count == 64 - kLinCarry &&
              lin_windows(65, 1).update.count == 1 + kLinCarry, "launch windows of a vaek_train_steps call");
constexpr int kLinReduceSets = 1;                 // persistent form: reducer sets taking alternate batches (one set of 24 beat two of 12)
constexpr int kLinReduceWgs = 24;                 // workgroups per set, each summing NO / 32 / 24 slices of 32 outputs (more resident
                                                  // workgroups measurably slow the streamers: 48 per set cost 2 us per step)

// Data parallel (world > 1): the moment matrix is additive over ranks.  Each reducer publishes its slice of the rank's M to every
// rank's exchange buffer (comm_dev.h's scheme: 8-byte granules {tag = the batch's Adam step, 32 bits of payload} in uncached,
// IPC-mapped memory, one aligned system-scope store each -- the data is the flag), waits for the same slice from all ranks in
// its own buffer, and adds them in rank order: every rank ends with the same bits, and the updater never learns that other
// ranks exist.  A double travels as two granules.  A reducer cannot get more than one batch ahead of a peer's (it needs that
// peer's granules to finish a batch), so banks by tag & 3 are never overwritten before they are read.
constexpr int kLinCommBanks = 4;
struct LinComm { unsigned long long* peer[kMaxWorld]; int world, rank, ng2; };     // ng2 = granules per (bank, source rank) = 2 NO

constexpr int kLinShards = 8, kLinShardStride = 32;   // words
struct LinPtrs { const float* x[64]; const float* z1[64]; const float* z2[64]; };    // batch pointers of a persistent launch (kernarg)
struct LinArgs {
    // roles by blockIdx.x: [0, has_update) the updater, then n_reduce reducers, then n_stream streamers
    int has_update, n_reduce, n_stream;
    int B, D, L, ntiles, T;                       // T: samples per tile (a multiple of 32, <= 512)
    // ---- launch-per-step form: streamers take THE batch of this launch, reducers the one before, the updater the one before that
    const float* x; const float* z1; const float* z2; float* partial_out;        // [ntiles][NBLK * 256]
    const float* partial_in; double* M_out;                                       // [NBLK * 256]
    const double* M_in;
    // ---- persistent form: the updater takes n_steps batches, the reducers n_red, the streamers n_str (lin_windows), each from
    // its own first slot on, round the kLinSlots slots; pointer tables as kernel arguments, arrival counters per slot
    int persistent, n_steps, sets;                // sets: reducer sets taking alternate batches
    int n_red, n_str, slot_upd, slot_red, slot_str;
    int d_red, d_str;                             // the reducers' / streamers' first batch minus the updater's: step_dev[0] counts the updater's
    float* partial_base; double* M_base;                                          // slot s at + s * ntiles * NO resp. + s * NO
    // arrival counters.  cnt_stream: kLinShards shards per batch, each on a 128-byte line of its own (a streamer adds to shard
    // blockIdx & 7: 228 adders on ONE word serialise at the memory side -- the reducers woke 8 us after the last streamer had
    // signalled); cnt_reduce: one word per batch.  A slot's counters are zero when its batch is first streamed: the updater
    // re-zeroes those of the batches it updated as the launch's last act (everybody else is provably done with them by then --
    // a batch carried into the next launch keeps its counts, and that launch zeroes them), lin_init_kernel zeroes all once per
    // workspace.  After a call's last launch every counter is zero again.
    unsigned* cnt_stream; unsigned* cnt_reduce; unsigned* status;                 // status: sticky, outside the zeroed range
    // ---- updater
    float* params; float* grads; float* m; float* v; int32_t* step_dev; float lr;
    float inv_bt, eps_cli, rows, rows_over_bt; int off_eps, P;
    float* loss_hist; long long loss_hist_cap;
    int stagger;                                  // streamers: waves 4 .. 7 enter a tile's products this many 64-cycle sleeps late (see there)
    LinComm comm;
};

#ifndef VAEK_LIN_ABL         // diagnostic builds (tools/lin_ablate.sh): 1 pieces issued in front of the products, 2 no MFMAs, 4 no image store,
#define VAEK_LIN_ABL 0       //   8 no LDS-DMA at all (the slots keep whatever they hold).  Results are garbage unless 0.
#endif
#ifdef VAEK_LIN_STAMPS      // diagnostic build (tools/lin_stamps.sh): s_memtime at the updater's phase boundaries, into a buffer nothing reads
static __device__ unsigned long long* g_lin_stamp_buf = nullptr;     // one per translation unit: vaek_debug_lin_stamps and lin_stamps_four set them
int lin_stamps_four(unsigned long long* buf);
#define LIN_STAMP(i)                                                                                         \
    do {                                                                                                     \
        if (VAEK_LIN_STAMPS == 2) break;      /* light build: only the drain-free time stamps (LIN_NOWQ) */    \
        __builtin_amdgcn_sched_barrier(0);                                                                   \
        unsigned long long _t;                                                                               \
        unsigned long long _r;                                                                               \
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_memtime %0\n\ts_memrealtime %1\n\ts_waitcnt lgkmcnt(0)" : "=s"(_t), "=s"(_r)::"memory"); \
        if (g_lin_stamp_buf && threadIdx.x == 0) { g_lin_stamp_buf[i] = _t; g_lin_stamp_buf[16 + (i)] = _r; } \
        __builtin_amdgcn_sched_barrier(0);                                                                   \
    } while (0)
#define LIN_NOW(v)                                                                                           \
    do {                                                                                                     \
        __builtin_amdgcn_sched_barrier(0);                                                                   \
        if (VAEK_LIN_STAMPS == 2) asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v)::"memory");             \
        else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v)::"memory"); \
        __builtin_amdgcn_sched_barrier(0);                                                                   \
    } while (0)
#define LIN_NOWQ(v)  /* no vmcnt wait: does not drain the wave's stores */                                   \
    do {                                                                                                     \
        __builtin_amdgcn_sched_barrier(0);                                                                   \
        asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v)::"memory");                        \
        __builtin_amdgcn_sched_barrier(0);                                                                   \
    } while (0)
#define LIN_PUT(i, v) do { if (g_lin_stamp_buf && threadIdx.x == 0) g_lin_stamp_buf[i] = (v); } while (0)
#define LIN_PUTMAX(i, v) do { if (g_lin_stamp_buf && threadIdx.x == 0) atomicMax(&g_lin_stamp_buf[i], (v)); } while (0)
#else
#define LIN_STAMP(i) do {} while (0)
#define LIN_NOW(v) do {} while (0)
#define LIN_NOWQ(v) do {} while (0)
#define LIN_PUT(i, v) do {} while (0)
#define LIN_PUTMAX(i, v) do {} while (0)
#endif

__device__ __forceinline__ void lin_glds16(const void* gsrc, void* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((glb_void_t*)gsrc, (lds_void_t*)lds_wave_base, 16, 0, 0);
}
template <int N> __device__ __forceinline__ void lin_wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
// Workgroup barrier that leaves LDS-DMA loads in flight: __syncthreads() would drain them (its fence waits vmcnt(0) while a
// global_load_lds is pending: cdna guide, LDS-DMA rules); LDS traffic of this wave is waited for explicitly.
__device__ __forceinline__ void lin_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// wait until at most n (wave-uniform, <= 20) of this wave's memory operations are outstanding
__device__ __forceinline__ void lin_wait_vmcnt_upto(int n) {
    switch (n) {
        case 1: lin_wait_vmcnt<1>(); break;   case 2: lin_wait_vmcnt<2>(); break;   case 3: lin_wait_vmcnt<3>(); break;
        case 4: lin_wait_vmcnt<4>(); break;   case 5: lin_wait_vmcnt<5>(); break;   case 6: lin_wait_vmcnt<6>(); break;
        case 7: lin_wait_vmcnt<7>(); break;   case 8: lin_wait_vmcnt<8>(); break;   case 9: lin_wait_vmcnt<9>(); break;
        case 10: lin_wait_vmcnt<10>(); break; case 11: lin_wait_vmcnt<11>(); break; case 12: lin_wait_vmcnt<12>(); break;
        case 13: lin_wait_vmcnt<13>(); break; case 14: lin_wait_vmcnt<14>(); break; case 15: lin_wait_vmcnt<15>(); break;
        case 16: lin_wait_vmcnt<16>(); break; case 17: lin_wait_vmcnt<17>(); break; case 18: lin_wait_vmcnt<18>(); break;
        case 19: lin_wait_vmcnt<19>(); break; case 20: lin_wait_vmcnt<20>(); break;
        default: lin_wait_vmcnt<0>(); break;
    }
}

// block (b1, b2), b1 <= b2, of the upper block triangle -> its index in the packed image
__device__ __host__ constexpr int lin_blk(int NB, int b1, int b2) { return b1 * NB - b1 * (b1 - 1) / 2 + (b2 - b1); }

// write-through (sc1) accesses of the in-launch hand-offs: relaxed agent-scope atomics lower to global_store / global_load ... sc1
__device__ __forceinline__ void st_sc1(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_sc1(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float ld_sc1(const float* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double ld_sc1(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// All threads call; thread 0 polls `*cnt >= target` (relaxed, with s_sleep; bounded: ~2 s, then the status word is set and
// every later wait of the launch returns at once so the grid drains), the workgroup barrier publishes the outcome.  The first
// wait to expire records who it was: 0x80000000 | role << 28 (1 updater, 2 reducer) | batch << 16 | the count it last saw.
__device__ __forceinline__ void lin_wait_count(const unsigned* cnt, unsigned target, unsigned* status, unsigned tag) {
    if (threadIdx.x == 0) {
        unsigned spins = 0, seen;
        while ((seen = __hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) < target) {
            __builtin_amdgcn_s_sleep(16);
            if ((++spins & 1023u) == 0) {
                if (__hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
                if (spins > (1u << 21)) {
                    unsigned expect = 0;
                    __hip_atomic_compare_exchange_strong(status, &expect, 0x80000000u | tag | (seen & 0xffffu), __ATOMIC_RELAXED,
                                                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    break;
                }
            }
        }
    }
    __syncthreads();
}

// the same on a batch's SHARDED streamer counter: thread 0 keeps all shards' loads in flight together and compares their sum
__device__ __forceinline__ void lin_wait_shards(const unsigned* cnt, unsigned target, unsigned* status, unsigned tag) {
    if (threadIdx.x == 0) {
        unsigned spins = 0, seen;
        for (;;) {
            unsigned v[kLinShards];
#pragma unroll
            for (int k = 0; k < kLinShards; ++k) v[k] = __hip_atomic_load(cnt + k * kLinShardStride, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            seen = 0;
#pragma unroll
            for (int k = 0; k < kLinShards; ++k) seen += v[k];
            if (seen >= target) break;
            __builtin_amdgcn_s_sleep(4);
            if ((++spins & 1023u) == 0) {
                if (__hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
                if (spins > (1u << 21)) {
                    unsigned expect = 0;
                    __hip_atomic_compare_exchange_strong(status, &expect, 0x80000000u | tag | (seen & 0xffffu), __ATOMIC_RELAXED,
                                                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    break;
                }
            }
        }
    }
    __syncthreads();
}

// one output of M across the ranks: publish this rank's value, collect everybody's, add in rank order (bounded spins)
__device__ __forceinline__ double lin_sum_over_ranks(const LinComm& c, unsigned epoch, int o, double v, unsigned* status) {
    const unsigned long long bits = (unsigned long long)__double_as_longlong(v), tag = (unsigned long long)epoch << 32;
    const long long bank = (long long)(epoch & (kLinCommBanks - 1)) * c.world * c.ng2;
    for (int p = 0; p < c.world; ++p) {
        unsigned long long* q = c.peer[p] + bank + (long long)c.rank * c.ng2 + 2 * o;
        __hip_atomic_store(q, tag | (bits & 0xffffffffull), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(q + 1, tag | (bits >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    const unsigned long long* own = c.peer[c.rank] + bank + 2 * o;
    double sum = 0.0;
    unsigned spins = 0;
    bool dead = false;
    for (int r = 0; r < c.world; ++r) {
        unsigned long long lo = 0, hi = 0;
        for (;;) {
            lo = __hip_atomic_load(own + (long long)r * c.ng2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            hi = __hip_atomic_load(own + (long long)r * c.ng2 + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            if (((unsigned)(lo >> 32) == epoch && (unsigned)(hi >> 32) == epoch) || dead) break;
            __builtin_amdgcn_s_sleep(8);
            if ((++spins & 1023u) == 0) {
                if (__hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) dead = true;
                else if (spins > (1u << 21)) {
                    unsigned expect = 0;
                    __hip_atomic_compare_exchange_strong(status, &expect, 0x80000000u | (3u << 28) | ((unsigned)r << 16) | (epoch & 0xffffu),
                                                         __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    dead = true;
                }
            }
        }
        sum += __longlong_as_double((long long)((hi << 32) | (lo & 0xffffffffull)));
    }
    return sum;
}

// ---- streamer pieces ------------------------------------------------------------------------------------------------------------
// LDS image of one T-sample tile: the three tensors' tiles exactly as they lie in HBM (row-major [T][L] / [T][D]), each region a
// whole number of 1 KB PIECES (one LDS-DMA wave-instruction: 64 lanes x 16 bytes).  Piece p of a tile goes to wave p % 8.  The
// validity column V[T] (the "1" feature; 0 for rows past the batch end) and a zero word live outside the slots: a full tile's
// column is all ones and is written once per launch.
struct LinTile {
    int nz1, nx, np, oX, oZ2, bytes;
    __device__ __host__ LinTile(int D, int L, int T) {
        nz1 = (L * 4 * T + 1023) >> 10; nx = (D * 4 * T + 1023) >> 10; np = nz1 + 2 * nx;
        oX = (nz1 << 10) + 80;      // + 20 banks: the feature block that mixes z1 and x columns then reads conflict-free in 3 k-steps of 4 (was 2 of 4)
        oZ2 = oX + (nx << 10); bytes = (oZ2 + (nx << 10) + 255) & ~255;
    }
};

// piece p (wave-uniform) of tile `tile`: 1 KB of z1 / x / z2 from HBM straight into the slot
__device__ __forceinline__ void lin_issue_piece(const LinArgs& a, const LinTile& tl, const float* x, const float* z1, const float* z2,
                                                int tile, int p, char* slot, int lane) {
    const float* src; int cols, idx, lds_off;
    if (p < tl.nz1) { src = z1; cols = a.L; idx = p; lds_off = 0; }
    else if (p < tl.nz1 + tl.nx) { src = x; cols = a.D; idx = p - tl.nz1; lds_off = tl.oX; }
    else { src = z2; cols = a.D; idx = p - tl.nz1 - tl.nx; lds_off = tl.oZ2; }
    const long long tot = (long long)a.B * cols * 4, base = (long long)tile * a.T * cols * 4;
    // the last 16-byte piece this tile may fetch: the tile's own (a region's padding up to whole pieces re-reads it -- a line this
    // CU has just fetched -- instead of pulling the NEXT tile's rows through another XCD's L2), and never past the tensor's last
    // whole 16 bytes; what a clamped piece brings lands in LDS nobody reads, in rows that are zeroed afterwards, or in the
    // tensor's last <= 3 floats, which lin_fix_ragged rewrites
    const long long last = min(tot & ~15ll, base + (long long)a.T * cols * 4) - 16;
    long long off = base + idx * 1024 + lane * 16;
    off = off <= last ? off : last;
    lin_glds16(reinterpret_cast<const char*>(src) + off, slot + lds_off + idx * 1024);
}

// The same with everything that does not depend on the piece worked out once per tile (the persistent streamers issue the pieces
// of a tile one by one between the k-steps of an earlier one: what is left per piece is a handful of scalar selects, one 64-bit
// add, one clamp).  All members are wave-uniform.
struct LinTileSrc {
    const char *z1, *x, *z2; long long baseL, lastL, baseD, lastD; char* slot; bool on;
    __device__ __forceinline__ void prepare(const LinArgs& a, const float* px, const float* pz1, const float* pz2, int tile, char* slot_) {
        auto uni = [](const float* q) {
            const unsigned long long u = (unsigned long long)q;
            // (readfirstlane returns int: through unsigned, or a low word >= 2^31 sign-extends into the high one)
            return reinterpret_cast<const char*>((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)u) |
                                                 ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)(u >> 32)) << 32));
        };
        z1 = uni(pz1); x = uni(px); z2 = uni(pz2); slot = slot_; on = true;
        const long long rows = (long long)tile * a.T;
        const long long totL = (long long)a.B * a.L * 4, totD = (long long)a.B * a.D * 4;
        baseL = rows * a.L * 4; baseD = rows * a.D * 4;
        lastL = min(totL & ~15ll, baseL + (long long)a.T * a.L * 4) - 16;
        lastD = min(totD & ~15ll, baseD + (long long)a.T * a.D * 4) - 16;
    }
    __device__ __forceinline__ void issue(const LinTile& tl, int p, int lane) const {      // piece p (wave-uniform)
        const char* src; long long base, last; int idx, lds_off;
        if (p < tl.nz1) { src = z1; base = baseL; last = lastL; idx = p; lds_off = 0; }
        else if (p < tl.nz1 + tl.nx) { src = x; base = baseD; last = lastD; idx = p - tl.nz1; lds_off = tl.oX; }
        else { src = z2; base = baseD; last = lastD; idx = p - tl.nz1 - tl.nx; lds_off = tl.oZ2; }
        long long off = base + idx * 1024 + lane * 16;
        off = off <= last ? off : last;
        lin_glds16(src + off, slot + lds_off + idx * 1024);
    }
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"      // (M0 on the clobber list: it is what the LDS-DMA takes its LDS address from)
    __device__ __forceinline__ void issue_tile(const LinTile& tl, int lw, int NLW, int lane) const {
        auto region = [&](const char* src, long long base, long long last, int n, int lds_off) __attribute__((always_inline)) {
            const long long b2 = base <= last ? base : last;           // (a last tile shorter than 16 bytes: every lane reads the tensor's last 16)
            const char* sbase = src + b2;
            const unsigned lastrel = (unsigned)(last - b2), degenerate = base <= last ? 0xffffffffu : 0u;
            const unsigned m0_0 = (unsigned)(size_t)(lds_void_t*)(slot + lds_off);
            for (int idx = lw; idx < n; idx += NLW) {
                unsigned off = ((unsigned)idx * 1024u + (unsigned)lane * 16u) & degenerate;
                off = off <= lastrel ? off : lastrel;
                asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(off), "s"(sbase), "s"(m0_0 + (unsigned)idx * 1024u) : "memory", "m0");
            }
        };
        region(z1, baseL, lastL, tl.nz1, 0);
        region(x, baseD, lastD, tl.nx, tl.oX);
        region(z2, baseD, lastD, tl.np - tl.nz1 - tl.nx, tl.oZ2);
    }
#pragma clang diagnostic pop
};

// the last tile of a ragged batch, after it has landed: the tensors' last floats behind their last whole 16 bytes, zeros in the
// rows past the batch end
__device__ __forceinline__ void lin_fix_ragged(const LinArgs& a, const LinTile& tl, const float* x, const float* z1, const float* z2,
                                               int tile, char* slot, int t) {
    const int T = a.T;
    const long long row0 = (long long)tile * T;
    const int valid = (int)min((long long)T, (long long)a.B - row0), D = a.D, L = a.L;
    if (valid < T) {
        auto patch_tail = [&](const float* src, int cols, int lds_off) {     // floats behind the tensor's last whole 16 bytes
            const long long tot = (long long)a.B * cols * 4, full = tot & ~15ll, base = row0 * cols * 4;
            if (t < (int)((tot - full) / 4) && full >= base) reinterpret_cast<float*>(slot + lds_off)[(full - base) / 4 + t] = src[full / 4 + t];
        };
        patch_tail(z1, L, 0); patch_tail(x, D, tl.oX); patch_tail(z2, D, tl.oZ2);
        for (int e = valid * L + t; e < T * L; e += LNT) reinterpret_cast<float*>(slot)[e] = 0.f;
        for (int e = valid * D + t; e < T * D; e += LNT) { reinterpret_cast<float*>(slot + tl.oX)[e] = 0.f; reinterpret_cast<float*>(slot + tl.oZ2)[e] = 0.f; }
    }
    lin_barrier();
}
// validity column of a tile with `valid` rows
__device__ __forceinline__ void lin_write_vcol(float* v, int T, int valid, int t) {
    for (int r = t; r < T; r += LNT) v[r] = r < valid ? 1.f : 0.f;
}

// 16-byte write-through store (the compiler does not count it: every wait on it is ours)
__device__ __forceinline__ void st_sc1_x4(float* p, f32x4 v) {
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}

// M_tile = U^T U.  The SAMPLES are dealt to the waves: wave w takes samples (T / 8) w .. -- T / 32 k-steps of 4 samples -- for
// every block of the upper block triangle, so each operand register read from LDS feeds NB (+1) MFMAs, the matrix pipes of
// the four SIMDs carry equal loads and the NBLK accumulator chains are independent.  hook(j) runs between the operand reads
// and the products of k-step j (the persistent streamers issue the LDS-DMA pieces of a later tile there: in the shadow of the
// matrix pipe).  JT > 0: the k-step count at compile time -- the loop unrolls, the reads carry immediate offsets and the waits
// are counted (with a run-time count hipcc waits lgkmcnt(0) before every group of products, prefetched operands included).
constexpr int lin_scratch_bytes(int NB) { return LNW * (NB * (NB + 1) / 2) * 1024; }       // (at 8 images; the persistent form's 4 need half)
// what a slot of the persistent streamers' ring reserves for that scratch: four blocks take the half they need (80 KB would put
// three slots over the LDS), three keep the size their plans were made with
constexpr int lin_ring_scratch_bytes(int NB) { return NB == 3 ? lin_scratch_bytes(NB) : lin_scratch_bytes(NB) / 2; }
constexpr int kLinCW = 4;      // persistent form: waves 0 .. 3 multiply (one per SIMD), waves 4 .. 7 load
// Where a lane's feature 16 u + (lane & 15) lives: byte offset of sample 0 and byte stride per sample.  Which tensor a feature
// belongs to does not change from tile to tile -- only the slot and (for the "1" feature) the validity column do -- so the
// persistent streamers work the lane's map out ONCE per launch and form a tile's offsets from it with two masked adds per block:
// per tile the five-way select (D and L are run-time values here) is ~200 instructions with ~20 exec-mask branches on each
// multiplying wave, between the tile's barrier and its first operand read (profiles/lin_blocks_roles.txt B).  Same addresses:
// the results are bitwise what they were.  in_slot / is_v: all ones where the feature lies in the tile's slot / is the
// validity column, else zero.
template <int NB> struct LinFeatMap {
    int fb[NB], fs[NB], in_slot[NB], is_v[NB];
    // v_off, c_off: byte offsets of the validity column of a full tile and of the zero word (neither lies in a slot)
    __device__ __forceinline__ void init(const LinArgs& a, const LinTile& tl, int v_off, int c_off, int lane) {
        const int D = a.D, L = a.L;
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            const int f = 16 * u + (lane & 15);
            in_slot[u] = f < L + 2 * D ? -1 : 0; is_v[u] = f == L + 2 * D ? -1 : 0;
            if (f < L) { fb[u] = f * 4; fs[u] = L * 4; }
            else if (f < L + D) { fb[u] = tl.oX + (f - L) * 4; fs[u] = D * 4; }
            else if (f < L + 2 * D) { fb[u] = tl.oZ2 + (f - L - D) * 4; fs[u] = D * 4; }
            else if (f == L + 2 * D) { fb[u] = v_off; fs[u] = 4; }
            else { fb[u] = c_off; fs[u] = 0; }
        }
    }
    // the tile in the slot at slot_off, its validity column v_delta bytes behind v_off
    __device__ __forceinline__ void at(int slot_off, int v_delta, int (&fb_out)[NB]) const {
#pragma unroll
        for (int u = 0; u < NB; ++u) fb_out[u] = fb[u] + (slot_off & in_slot[u]) + (v_delta & is_v[u]);
    }
};

template <int NB, int JT, int CW, typename Hook>
__device__ __forceinline__ void lin_tile_products_at(const LinArgs& a, const char* smem, const int (&fb)[NB], const int (&fs)[NB],
                                                     f32x4 (&acc)[NB * (NB + 1) / 2], int lane, int wave, Hook&& hook);

template <int NB, int JT, int CW, typename Hook>
__device__ __forceinline__ void lin_tile_products(const LinArgs& a, const LinTile& tl, const char* smem, int slot_off, int v_off, int c_off,
                                                  f32x4 (&acc)[NB * (NB + 1) / 2], int lane, int wave, Hook&& hook) {
    LinFeatMap<NB> map;
    map.init(a, tl, v_off, c_off, lane);
    int fb[NB];
    map.at(slot_off, 0, fb);
    lin_tile_products_at<NB, JT, CW>(a, smem, fb, map.fs, acc, lane, wave, hook);
}

// the products proper: fb / fs, this lane's byte offset of sample 0 and byte stride per sample of feature 16 u + (lane & 15)
template <int NB, int JT, int CW, typename Hook>
__device__ __forceinline__ void lin_tile_products_at(const LinArgs& a, const char* smem, const int (&fb)[NB], const int (&fs)[NB],
                                                     f32x4 (&acc)[NB * (NB + 1) / 2], int lane, int wave, Hook&& hook) {
    constexpr int NBLK = NB * (NB + 1) / 2;
    const int g = lane >> 4;
#pragma unroll
    for (int k = 0; k < NBLK; ++k) acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
    // Wave w takes samples (T / CW) w .. + T / CW - 1 in J = T / (4 CW) k-steps of 4.  Within a run of 16 samples lane group g takes sample
    // s + 4 g in step s: four rows apart, i.e. 16 banks with 80- and 48-byte rows, so the lane groups one ds_read_b32 services
    // together never collide; a run shorter than 16 (T / 8 not a multiple of 16: its last r < 4 steps) takes s + r g.
    // (CW: the waves that share a tile's samples -- all 8 of the launch-per-step form, the 4 compute waves of the persistent one)
    const int J = JT ? JT : a.T / (4 * CW), wbase = (a.T / CW) * wave, jfull = J & ~3;
    auto products = [&](const float (&op)[NB]) __attribute__((always_inline)) {
        int k = 0;
#pragma unroll
        for (int b1 = 0; b1 < NB; ++b1)
#pragma unroll
            for (int b2 = b1; b2 < NB; ++b2, ++k) {
                if (VAEK_LIN_ABL & 2) acc[k][0] += op[b1] * op[b2];
                else acc[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(op[b1], op[b2], acc[k], 0, 0, 0);
            }
    };
    if constexpr (JT > 0) {
        // per-lane address of every feature's operand, advanced from k-step to k-step by adds only: + one sample inside a run of
        // four steps, + 13 samples from one run to the next, the short last run from its own base
        constexpr int JF = JT & ~3;
        int cur[NB], fs13[NB], tail[NB];
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            cur[u] = fb[u] + (wbase + 4 * g) * fs[u]; fs13[u] = 13 * fs[u];
            tail[u] = fb[u] + (wbase + 4 * JF + (JT - JF) * g) * fs[u];
        }
        float op[JT][NB];
        auto fetch = [&](int j) __attribute__((always_inline)) {                              // called for j = 0, 1, 2, ... in order
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                if (j == JF) cur[u] = tail[u];
                op[j][u] = *reinterpret_cast<const float*>(smem + cur[u]);
                cur[u] += (j < JF && (j & 3) == 3) ? fs13[u] : fs[u];
            }
        };
        fetch(0);
        if (JT > 1) fetch(1);
#pragma unroll
        for (int j = 0; j < JT; ++j) {
            if (j + 2 < JT) fetch(j + 2);                      // operands two k-steps ahead
            hook(j);
            __builtin_amdgcn_sched_barrier(0);
            products(op[j]);
            __builtin_amdgcn_sched_barrier(0);
        }
    } else {
        // Operands run one step ahead in a second register set, and the scheduler is told to keep it that way: left alone hipcc
        // reuses one register set and waits out the full LDS latency before every MFMA.
        float op[2][NB];
        auto fetch = [&](int set, int j) __attribute__((always_inline)) {
            const int sample = wbase + (j < jfull ? 16 * (j >> 2) + (j & 3) + 4 * g : 4 * jfull + (j - jfull) + (J - jfull) * g);
#pragma unroll
            for (int u = 0; u < NB; ++u) op[set][u] = *reinterpret_cast<const float*>(smem + fb[u] + sample * fs[u]);
        };
        fetch(0, 0);
        for (int j = 0; j < J; j += 2) {
            if (j + 1 < J) fetch(1, j + 1);
            hook(j);
            __builtin_amdgcn_sched_barrier(0);                 // the reads of step j + 1 are issued before the MFMAs of step j
            products(op[0]);
            __builtin_amdgcn_sched_barrier(0);
            if (j + 1 < J) {
                if (j + 2 < J) fetch(0, j + 2);
                hook(j + 1);
                __builtin_amdgcn_sched_barrier(0);
                products(op[1]);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
}

// The eight per-wave images are summed through LDS (in wave order: deterministic) in `scratch` -- the tile's own slot, dead once
// every wave has passed the barrier behind its products -- and leave as ONE image in the accumulators' own layout
// [block][lane][4] (image element (row, col) of a block sits at ((row >> 2) * 16 + col) * 4 + (row & 3): lin_img_index), so the
// sum reads and the store are 16 bytes per lane.
template <int NB, bool SC1, int CW>
__device__ __forceinline__ void lin_tile_combine(const f32x4 (&acc)[NB * (NB + 1) / 2], char* scratch, float* out, int t, int wave, int lane) {
    constexpr int NBLK = NB * (NB + 1) / 2;
    f32x4* scr = reinterpret_cast<f32x4*>(scratch);       // [wave][block][lane]
    if (wave < CW) {
#pragma unroll
        for (int k = 0; k < NBLK; ++k) scr[(wave * NBLK + k) * 64 + lane] = acc[k];
    }
    lin_barrier();
    for (int q = t; q < NBLK * 64; q += LNT) {
        f32x4 sum = scr[q];
#pragma unroll
        for (int w = 1; w < CW; ++w) sum += scr[w * NBLK * 64 + q];
        if ((VAEK_LIN_ABL & 4) && sum[0] != 12345.f) continue;
        if (SC1) st_sc1_x4(out + 4 * q, sum); else *reinterpret_cast<f32x4*>(out + 4 * q) = sum;
    }
}
// (block, row, col) of image element e in that layout
__device__ __forceinline__ void lin_img_coords(int e, int& blk, int& i, int& j) {
    blk = e >> 8; const int ln = (e >> 2) & 63; i = ((ln >> 4) << 2) + (e & 3); j = ln & 15;
}

// ---- reducer: 32 outputs x 16 row groups per workgroup, float64, fixed order ------------------------------------------------
template <bool SC1>
__device__ __forceinline__ void lin_reduce(const float* partial_in, double* M_out, int ntiles, char* smem, int rb, int no,
                                           const LinComm* cm = nullptr, unsigned epoch = 0, unsigned* status = nullptr) {
    double* sums = reinterpret_cast<double*>(smem);       // [16][32]
    const int t = threadIdx.x, o = rb * 32 + (t & 31), rg = t >> 5;
    const int rpg = (ntiles + 15) / 16, r_lo = rg * rpg, r_hi = min(ntiles, r_lo + rpg);
    double s = 0.0;
    if (o < no)
        for (int r0 = r_lo; r0 < r_hi; r0 += 16) {
            float tv[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) {                 // unconditional, clamped
                const float* q = partial_in + (long long)min(r0 + u, r_hi - 1) * no + o;
                tv[u] = SC1 ? ld_sc1(q) : *q;
            }
#pragma unroll
            for (int u = 0; u < 16; ++u) s += r0 + u < r_hi ? (double)tv[u] : 0.0;
        }
    sums[rg * 32 + (t & 31)] = s;
    __syncthreads();
    if (t < 32 && o < no) {
        double tot = 0.0;
#pragma unroll
        for (int k = 0; k < 16; ++k) tot += sums[k * 32 + t];
        if (cm && cm->world > 1) tot = lin_sum_over_ranks(*cm, epoch, o, tot, status);
        if (SC1) st_sc1(M_out + o, tot); else M_out[o] = tot;
    }
}

// two 32-output slices at once (the persistent form's reducers own two each): both slices' loads are in flight together, one
// memory round trip per batch instead of two.  Same row groups, same order of additions as lin_reduce: bitwise its sums.
__device__ __forceinline__ void lin_reduce_pair(const float* partial_in, double* M_out, int ntiles, char* smem, int rb0, int rb1, int no,
                                                const LinComm& cm, unsigned epoch, unsigned* status) {
    double* sums = reinterpret_cast<double*>(smem);       // [2][16][32]
    const int t = threadIdx.x, q = t & 31, rg = t >> 5, o0 = rb0 * 32 + q, o1 = rb1 * 32 + q;
    const int rpg = (ntiles + 15) / 16, r_lo = rg * rpg, r_hi = min(ntiles, r_lo + rpg);
    double s0 = 0.0, s1 = 0.0;
    for (int r0 = r_lo; r0 < r_hi; r0 += 16) {
        float ta[16], tb[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {                     // unconditional, clamped
            const float* row = partial_in + (long long)min(r0 + u, r_hi - 1) * no;
            ta[u] = ld_sc1(row + o0); tb[u] = ld_sc1(row + o1);
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) { s0 += r0 + u < r_hi ? (double)ta[u] : 0.0; s1 += r0 + u < r_hi ? (double)tb[u] : 0.0; }
    }
    sums[rg * 32 + q] = s0; sums[512 + rg * 32 + q] = s1;
    __syncthreads();
    if (t < 64) {
        const int which = t >> 5;
        double tot = 0.0;
#pragma unroll
        for (int k = 0; k < 16; ++k) tot += sums[which * 512 + k * 32 + q];
        if (cm.world > 1) tot = lin_sum_over_ranks(cm, epoch, which ? o1 : o0, tot, status);
        st_sc1(M_out + (which ? o1 : o0), tot);
    }
}

// ---- updater: gradients and loss from (M, parameters), Adam -----------------------------------------------------------------
// R and E are never formed.  With S = E + [diag(s) | 0 | 0 | 0] (samples = S u) and r = Wd^T samples + bd - x + sigma z2:
//     SM = S M                      (L x NF; S has D + 2 non-zeros per row)          Q = E M = SM - diag(s) M[z1 rows]
//     P1 = R M = Wd^T SM - M[x rows] + sigma M[z2 rows] + bd M[one row]              (D x NF)
//     G  = Wd P1                    (L x NF)          dwd[l][d] = S[l,:] . P1[d,:]   (= sum_b samples_bl r_bd)
//     sum_b |r_b|^2 = tr(R M R^T) = sum_{l,d} Wd[l][d] dwd[l][d] + sum_d (-P1[d][x_d] + sigma P1[d][z2_d] + bd_d P1[d][one])
//     sum_b |mu_b|^2 = tr(E M E^T) = sum_l (sum_dd We[dd][l] Q[l][x_dd] + be_l Q[l][one])
// DT, LT > 0: the dimensions at compile time (the metric's 12 / 20: fully unrolled inner products); 0: run-time.
// The parameters and Adam moments of this thread's outputs (idx = t + 512 k) live in its registers; the float64 copies the
// products read live in LDS and are refreshed by the owning thread after each update, so a persistent updater touches global
// memory per step only for M, the loss and (at the end) the results.
constexpr int LKOUT = 4;                              // P + 4 <= 2 048 at L + 2 D + 1 <= 64
template <int NB, int DT, int LT>
struct LinUpd {
    static constexpr int NFP = 16 * NB, NBLK = NB * (NB + 1) / 2;
    int D, L, P, fone, off_be, off_wd, off_bd, off_epsp, off_eps;
    double *Mf, *SM, *P1, *G, *Wed, *Wdd, *bed, *bdd, *sd, *elv, *lvd, *dwd, *red, *epsv;
    float p[LKOUT], m[LKOUT], v[LKOUT];

    __device__ __forceinline__ void carve(const LinArgs& a, char* smem) {
        D = DT ? DT : a.D; L = LT ? LT : a.L; P = a.P; fone = L + 2 * D; off_eps = a.off_eps;
        off_be = D * L; off_wd = off_be + L; off_bd = off_wd + L * D; off_epsp = off_bd + D;
        Mf = reinterpret_cast<double*>(smem);             // [NFP][NFP] symmetric
        SM = Mf + NFP * NFP; P1 = SM + L * NFP; G = P1 + D * NFP;
        Wed = G + L * NFP; Wdd = Wed + D * L; bed = Wdd + L * D; bdd = bed + L; sd = bdd + D; elv = sd + L; lvd = elv + L;
        dwd = lvd + L; red = dwd + L * D; epsv = red + 4 * LNW;
    }
    static __host__ size_t lds_bytes(int D, int L) {
        return sizeof(double) * ((size_t)NFP * NFP + (size_t)(D + 2 * L) * NFP + 3 * (size_t)D * L + 5 * L + D + 4 * LNW + 2);
    }
    __device__ __forceinline__ void load_state(const LinArgs& a) {
        const int t = threadIdx.x;
#pragma unroll
        for (int k = 0; k < LKOUT; ++k) {
            const int idx = min(t + LNT * k, P - 1);
            p[k] = a.params[idx]; m[k] = a.m[idx]; v[k] = a.v[idx];
        }
    }
    // float64 copies of this thread's own parameters into the arrays the products read
    __device__ __forceinline__ void publish_params() {
        const int t = threadIdx.x;
#pragma unroll
        for (int k = 0; k < LKOUT; ++k) {
            const int i = t + LNT * k;
            const double pv = (double)p[k];
            if (i < off_be) Wed[i] = pv;
            else if (i < off_wd) bed[i - off_be] = pv;
            else if (i < off_bd) Wdd[i - off_wd] = pv;
            else if (i < off_epsp) bdd[i - off_bd] = pv;
            else if (i < off_epsp + L) { const double sl = exp(0.5 * pv); sd[i - off_epsp] = sl; elv[i - off_epsp] = sl * sl; lvd[i - off_epsp] = pv; }
            else if (i == off_eps) epsv[0] = pv;
        }
    }
    template <bool SC1>
    __device__ __forceinline__ void expand_M(const double* M_in) {
        for (int e = threadIdx.x; e < NBLK * 256; e += LNT) {
            int k, i, j;
            lin_img_coords(e, k, i, j);
            int b1 = 0, rem = k;
            while (rem >= NB - b1) { rem -= NB - b1; ++b1; }
            const int b2 = b1 + rem;
            const double val = SC1 ? ld_sc1(M_in + e) : M_in[e];
            Mf[(16 * b1 + i) * NFP + 16 * b2 + j] = val;
            Mf[(16 * b2 + j) * NFP + 16 * b1 + i] = val;   // (diagonal blocks are bitwise symmetric: same products, same order)
        }
    }
    // the same in two halves (persistent form): the loads of batch n + 1's M ride under step n when its reducers are already done
    static constexpr int MPT = (NBLK * 256 + LNT - 1) / LNT;
    __device__ __forceinline__ void fetch_M(const double* M_in, double (&r)[MPT]) {
#pragma unroll
        for (int k = 0; k < MPT; ++k) r[k] = ld_sc1(M_in + min((int)threadIdx.x + LNT * k, NBLK * 256 - 1));
    }
    __device__ __forceinline__ void scatter_M(const double (&r)[MPT]) {
#pragma unroll
        for (int k = 0; k < MPT; ++k) {
            const int e = threadIdx.x + LNT * k;
            if (e < NBLK * 256) {
                int blk, i, j;
                lin_img_coords(e, blk, i, j);
                int b1 = 0, rem = blk;
                while (rem >= NB - b1) { rem -= NB - b1; ++b1; }
                const int b2 = b1 + rem;
                Mf[(16 * b1 + i) * NFP + 16 * b2 + j] = r[k];
                Mf[(16 * b2 + j) * NFP + 16 * b1 + i] = r[k];
            }
        }
    }
    // one step: Mf and the parameter copies are in LDS (a barrier behind them); returns with this thread's p / m / v updated,
    // its gradients in gout[], and nothing in LDS that the next publish_params / expand_M may not overwrite after a barrier
    __device__ __forceinline__ void step(const LinArgs& a, int tstep, float (&gout)[LKOUT]) {
        const int t = threadIdx.x;
        const double eps = off_eps >= 0 ? epsv[0] * (double)a.eps_cli : (double)a.eps_cli;
        const double sigma = exp(0.5 * eps), inv_var = 1.0 / (sigma * sigma);       // (one float64 exp on the chain, not two)
        LIN_STAMP(1);
        if constexpr (DT > 0 && LT > 0 && (DT % 2 == 0) && (LT % 2 == 0) && LT * (NFP / 2) <= LNT && LT * DT <= LNT / 2) {
            // The metric's shape.  Each thread owns 2 (SM, P1) or 4 (G) neighbouring columns of one output row, so that the M / SM /
            // P1 operands arrive as 16-byte LDS reads, every phase is ONE round of the workgroup, and all operands of a thread
            // are in registers before its first FMA (hipcc otherwise waits out the LDS latency once per product).
            constexpr int HP = NFP / 2;
            {   // SM = S M: thread (l, f .. f + 1)
                const int l = min(t / HP, LT - 1), f = (t % HP) * 2;
                double w[DT + 2]; d2 mv[DT + 2];
                w[0] = sd[l]; mv[0] = *reinterpret_cast<const d2*>(Mf + l * NFP + f);
                w[1] = bed[l]; mv[1] = *reinterpret_cast<const d2*>(Mf + fone * NFP + f);
#pragma unroll
                for (int dd = 0; dd < DT; ++dd) { w[2 + dd] = Wed[dd * LT + l]; mv[2 + dd] = *reinterpret_cast<const d2*>(Mf + (LT + dd) * NFP + f); }
                __builtin_amdgcn_sched_barrier(0);
                d2 s2 = w[0] * mv[0];
#pragma unroll
                for (int k = 1; k < DT + 2; ++k) s2 += w[k] * mv[k];
                if (t < LT * HP) *reinterpret_cast<d2*>(SM + l * NFP + f) = s2;
            }
            __syncthreads();
            LIN_STAMP(2);
            {   // P1 = R M: thread (d, f .. f + 1)
                const int d = min(t / HP, DT - 1), f = (t % HP) * 2;
                double w[LT + 1]; d2 mv[LT + 3];
                mv[LT] = *reinterpret_cast<const d2*>(Mf + (LT + DT + d) * NFP + f);
                mv[LT + 1] = *reinterpret_cast<const d2*>(Mf + (LT + d) * NFP + f);
                mv[LT + 2] = *reinterpret_cast<const d2*>(Mf + fone * NFP + f);
                w[LT] = bdd[d];
#pragma unroll
                for (int l = 0; l < LT; ++l) { w[l] = Wdd[l * DT + d]; mv[l] = *reinterpret_cast<const d2*>(SM + l * NFP + f); }
                __builtin_amdgcn_sched_barrier(0);
                d2 s2 = sigma * mv[LT] - mv[LT + 1] + w[LT] * mv[LT + 2];
#pragma unroll
                for (int l = 0; l < LT; ++l) s2 += w[l] * mv[l];
                if (t < DT * HP) *reinterpret_cast<d2*>(P1 + d * NFP + f) = s2;
            }
            __syncthreads();
            LIN_STAMP(3);
            if (t < LNT / 2) {   // G = Wd P1: thread (l, f .. f + 3), the lower half of the workgroup
                constexpr int QP = NFP / 4;
                const int l = min(t / QP, LT - 1), f = (t % QP) * 4;
                d2 wv[DT / 2], pa[DT], pb[DT];
#pragma unroll
                for (int d = 0; d < DT / 2; ++d) wv[d] = *reinterpret_cast<const d2*>(Wdd + l * DT + 2 * d);
#pragma unroll
                for (int d = 0; d < DT; ++d) { pa[d] = *reinterpret_cast<const d2*>(P1 + d * NFP + f); pb[d] = *reinterpret_cast<const d2*>(P1 + d * NFP + f + 2); }
                __builtin_amdgcn_sched_barrier(0);
                d2 sa = {0.0, 0.0}, sb = {0.0, 0.0};
#pragma unroll
                for (int d = 0; d < DT; ++d) { const double wd = wv[d / 2][d & 1]; sa += wd * pa[d]; sb += wd * pb[d]; }
                if (t < LT * QP) { *reinterpret_cast<d2*>(G + l * NFP + f) = sa; *reinterpret_cast<d2*>(G + l * NFP + f + 2) = sb; }
            } else {             // dwd[l][d] = S[l,:] . P1[d,:]: the upper half
                const int e = min(t - LNT / 2, LT * DT - 1), l = e / DT, d = e % DT;
                double w[DT]; d2 pv[DT / 2];
                const double s_l = sd[l], b_l = bed[l], p_l = P1[d * NFP + l], p_o = P1[d * NFP + fone];
#pragma unroll
                for (int dd = 0; dd < DT; ++dd) w[dd] = Wed[dd * LT + l];
#pragma unroll
                for (int dd = 0; dd < DT / 2; ++dd) pv[dd] = *reinterpret_cast<const d2*>(P1 + d * NFP + LT + 2 * dd);
                __builtin_amdgcn_sched_barrier(0);
                double sx = s_l * p_l + b_l * p_o;
#pragma unroll
                for (int dd = 0; dd < DT; ++dd) sx += w[dd] * pv[dd / 2][dd & 1];
                if (t - LNT / 2 < LT * DT) dwd[e] = sx;
            }
        } else {
        for (int e = t; e < L * NFP; e += LNT) {              // SM = S M
            const int l = e / NFP, f = e % NFP;
            double s = sd[l] * Mf[l * NFP + f] + bed[l] * Mf[fone * NFP + f];
#pragma unroll
            for (int dd = 0; dd < (DT ? DT : 32); ++dd) if (DT || dd < D) s += Wed[dd * L + l] * Mf[(L + dd) * NFP + f];
            SM[e] = s;
        }
        __syncthreads();
        LIN_STAMP(2);
        for (int e = t; e < D * NFP; e += LNT) {              // P1 = R M
            const int d = e / NFP, f = e % NFP;
            double s = sigma * Mf[(L + D + d) * NFP + f] - Mf[(L + d) * NFP + f] + bdd[d] * Mf[fone * NFP + f];
            // (the latent index runs to L <= 61 here -- L + 2 D + 1 <= 64 with D >= 1 -- where the data index of the other loops stops
            // at D <= 31: bounded by 32 this sum lost the latents 32 .. L - 1 of every model lin_plan sends here with L > 32)
            if constexpr (LT > 0) {
#pragma unroll
                for (int l = 0; l < LT; ++l) s += Wdd[l * D + d] * SM[l * NFP + f];
            } else {
                for (int l = 0; l < L; ++l) s += Wdd[l * D + d] * SM[l * NFP + f];
            }
            P1[e] = s;
        }
        __syncthreads();
        LIN_STAMP(3);
        for (int e = t; e < L * NFP; e += LNT) {              // G = Wd P1
            const int l = e / NFP, f = e % NFP;
            double s = 0.0;
#pragma unroll
            for (int d = 0; d < (DT ? DT : 32); ++d) if (DT || d < D) s += Wdd[l * D + d] * P1[d * NFP + f];
            G[e] = s;
        }
        for (int e = t; e < L * D; e += LNT) {                // dwd[l][d] = S[l,:] . P1[d,:]
            const int l = e / D, d = e % D;
            double s = sd[l] * P1[d * NFP + l] + bed[l] * P1[d * NFP + fone];
#pragma unroll
            for (int dd = 0; dd < (DT ? DT : 32); ++dd) if (DT || dd < D) s += Wed[dd * L + l] * P1[d * NFP + L + dd];
            dwd[e] = s;
        }
        }
        __syncthreads();
        LIN_STAMP(4);
        double ssq = 0.0, musq = 0.0, z2r = 0.0, klc = 0.0;
        if constexpr (DT > 0 && LT > 0 && (DT % 2 == 0) && (LT % 2 == 0) && LT * (NFP / 2) <= LNT && LT * DT <= LNT / 2) {
            // Only d loss / d epsilon and the three loss means need the four scalar sums, and wave 0 owns those outputs (index
            // P - 1 .. P + 2 < LNT + 64): it forms the sums by itself -- strided shares per lane, operands batched, xor-shuffles --
            // while the other waves are already at their gradients and Adam.  No barrier, no workgroup-wide reduction.
            static_assert(DT * LT + LT + LT * DT + DT + LT + 1 + 3 <= LNT + 64, "wave 0 must own the scalar outputs");
            if (t < 64) {
                constexpr int NS = (LT * DT + 63) / 64, NM = (LT * (DT + 1) + 63) / 64;
                double wa[NS], da[NS], qw[NM], qs[NM], qd[NM], qm[NM];
#pragma unroll
                for (int j = 0; j < NS; ++j) { const int e = min(t + 64 * j, LT * DT - 1); wa[j] = Wdd[e]; da[j] = dwd[e]; }
#pragma unroll
                for (int j = 0; j < NM; ++j) {
                    const int e = min(t + 64 * j, LT * (DT + 1) - 1), l = e / (DT + 1), dd = e % (DT + 1), f = dd < DT ? LT + dd : fone;
                    qw[j] = dd < DT ? Wed[dd * LT + l] : bed[l]; qs[j] = SM[l * NFP + f]; qd[j] = sd[l]; qm[j] = Mf[l * NFP + f];
                }
                const int dq = min(t, DT - 1), lq = min(t, LT - 1);
                const double px = P1[dq * NFP + LT + dq], pz = P1[dq * NFP + LT + DT + dq], po = P1[dq * NFP + fone], bq = bdd[dq];
                const double lvq = lvd[lq], evq = elv[lq];
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int j = 0; j < NS; ++j) ssq += t + 64 * j < LT * DT ? wa[j] * da[j] : 0.0;
#pragma unroll
                for (int j = 0; j < NM; ++j) musq += t + 64 * j < LT * (DT + 1) ? qw[j] * (qs[j] - qd[j] * qm[j]) : 0.0;
                if (t < DT) { ssq += -px + sigma * pz + bq * po; z2r = pz; }
                if (t < LT) klc = 1.0 + lvq - evq;                                     // 1 + lv - e^{lv}
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    ssq += __shfl_xor(ssq, o, 64); musq += __shfl_xor(musq, o, 64);
                    z2r += __shfl_xor(z2r, o, 64); klc += __shfl_xor(klc, o, 64);
                }
            }
        } else {
        // the four scalar sums: each thread a strided share, lanes by xor-shuffle, the waves in order (all fixed order)
        double p_ssq = 0.0, p_musq = 0.0, p_z2r = 0.0, p_klc = 0.0;
        for (int e = t; e < L * D; e += LNT) p_ssq += Wdd[e] * dwd[e];
        if (t < D) {
            p_ssq += -P1[t * NFP + L + t] + sigma * P1[t * NFP + L + D + t] + bdd[t] * P1[t * NFP + fone];
            p_z2r = P1[t * NFP + L + D + t];
        }
        for (int e = t; e < L * (D + 1); e += LNT) {
            const int l = e / (D + 1), dd = e % (D + 1);
            const int f = dd < D ? L + dd : fone;
            const double q = SM[l * NFP + f] - sd[l] * Mf[l * NFP + f];            // Q = E M
            p_musq += (dd < D ? Wed[dd * L + l] : bed[l]) * q;
        }
        if (t < L) p_klc = 1.0 + lvd[t] - elv[t];                                  // 1 + lv - e^{lv}
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            p_ssq += __shfl_xor(p_ssq, o, 64); p_musq += __shfl_xor(p_musq, o, 64);
            p_z2r += __shfl_xor(p_z2r, o, 64); p_klc += __shfl_xor(p_klc, o, 64);
        }
        if ((t & 63) == 0) { red[t >> 6] = p_ssq; red[LNW + (t >> 6)] = p_musq; red[2 * LNW + (t >> 6)] = p_z2r; red[3 * LNW + (t >> 6)] = p_klc; }
        __syncthreads();
#pragma unroll
        for (int w = 0; w < LNW; ++w) { ssq += red[w]; musq += red[LNW + w]; z2r += red[2 * LNW + w]; klc += red[3 * LNW + w]; }
        }
        LIN_STAMP(5);
        const double inv_bt = (double)a.inv_bt, rows = (double)a.rows, c0 = inv_var * inv_bt;
        const float bc1 = -expm1f((float)tstep * -0.10536051565782628f), bc2 = -expm1f((float)tstep * -0.0010005003335835335f);
#pragma unroll
        for (int k = 0; k < LKOUT; ++k) {
            const int idx = t + LNT * k;
            double gd = 0.0;
            if (idx < off_be) { const int d = idx / L, l = idx % L; gd = c0 * G[l * NFP + L + d] + (SM[l * NFP + L + d] - sd[l] * Mf[l * NFP + L + d]) * inv_bt; }
            else if (idx < off_wd) { const int l = idx - off_be; gd = c0 * G[l * NFP + fone] + (SM[l * NFP + fone] - sd[l] * Mf[l * NFP + fone]) * inv_bt; }
            else if (idx < off_bd) gd = c0 * dwd[idx - off_wd];
            else if (idx < off_epsp) gd = c0 * P1[(idx - off_bd) * NFP + fone];
            else if (idx < off_epsp + L) {
                const int l = idx - off_epsp;
                gd = 0.5 * sd[l] * c0 * G[l * NFP + l] - 0.5 * (1.0 - elv[l]) * (double)a.rows_over_bt;
            } else if (idx == off_eps) {
                gd = (double)a.eps_cli * (-0.5 * ssq * inv_var + 0.5 * rows * D + 0.5 * sigma * z2r * inv_var) * inv_bt;
            } else if (idx >= P && idx < P + 3) {
                const double dkl = (0.5 * musq - 0.5 * rows * klc) * inv_bt;
                const double mse = (0.5 * ssq * inv_var + 0.5 * rows * D * ((double)kLog2Pi + eps)) * inv_bt;
                gd = idx == P ? dkl + mse : (idx == P + 1 ? dkl : mse);
            }
            const float gf = (float)gd;
            gout[k] = gf;
            if (idx == P && a.loss_hist) a.loss_hist[(long long)(tstep - 1) % a.loss_hist_cap] = gf;
            if (idx < P) adam_apply_f(p[k], gf, m[k], v[k], a.lr, bc1, bc2);
        }
        LIN_STAMP(6);
    }
    __device__ __forceinline__ void store_state(const LinArgs& a, const float (&gout)[LKOUT], int tstep) {
        const int t = threadIdx.x;
#pragma unroll
        for (int k = 0; k < LKOUT; ++k) {
            const int idx = t + LNT * k;
            if (idx < P + kExtra) a.grads[idx] = gout[k];
            if (idx < P) { a.params[idx] = p[k]; a.m[idx] = m[k]; a.v[idx] = v[k]; }
        }
        if (t == 0) a.step_dev[0] = tstep;
    }
};

// ---- updater on the float64 matrix cores (persistent form; L <= 32 and three feature blocks with D <= 16, or four) --------------------
// The same algebra as LinUpd, laid out so that the dependent chain SM -> P1 -> G never leaves the registers: with the FEATURE index
// on the MFMA column (lane & 15) every product is  Out = Weights x Prev  and an accumulator tile of v_mfma_f64_16x16x4_f64
// (lane (col, g), register r = row g + 4 r) is exactly the B operand of the next product's k-step r in natural k order (probed
// with exact integers: tools/mfma_f64_probe.hip; 64 cycles per instruction, dependent or not).  Wave w < NB owns feature block w:
//     SM[:, blk]  = diag(s) M[z1 rows, blk] + be (x) M[one, blk]  (accumulator init)  +  We^T . M[x rows, blk]        (2 row tiles x KD k-steps)
//     P1[:, blk]  = -M[x rows] + sigma M[z2 rows] + bd (x) M[one]  (init)              +  Wd^T . SM                     (4 + RL1 k-steps)
//     G[:, blk]   =                                                                       Wd . P1                       (2 x KD)
// and every gradient that is an ELEMENT of those tiles is finished in place: dWe / dbe = c0 G + (SM - s M[z1 row]) / B on the x and
// "one" columns, d lv on the diagonal of the z1 columns, dbd = c0 P1[:, one].  Only dWd = S P1^T sums over the feature index, i.e.
// across lanes: the chain waves drop P1 (4.6 KB) into LDS and wave NB forms dwd^T = P1[:, x cols] We + ... with 2 x KD MFMAs while
// the chain waves run G; wave NB + 1 sums the KL term.  The four scalar sums are wave reductions of values the lanes hold anyway.
// Four blocks (49 .. 64 features, D up to 31): P1 gets a second row tile (d = 16 .. 31: PT = 2, its own 4 + RL1 k-steps), G takes
// KD <= 8 k-steps, the first four from P1's first tile and the rest from its second, and dWd has two output row tiles.  Per step: 3 barriers,
// ~17 dependent MFMAs (1.1 k cycles) instead of ~7 k cycles of LDS-bound float64 FMAs.  M arrives straight from the reducers'
// image into registers (17 write-through loads per lane at offsets fixed for the launch, prefetched a step ahead when the
// reducers are ahead): no symmetric copy in LDS.
using d4 = __attribute__((ext_vector_type(4))) double;
// Sum over the wave, the same value in every lane.  Four DPP stages inside each row of 16 lanes (the two dwords of a double move
// separately; xor 1, xor 2, half mirror, mirror: every lane ends with its row's total), then the four rows by v_readlane -- ~25
// instructions where six __shfl_xor stages are twelve ds_bpermute round trips (the three sums of a step cost 1.8 k cycles that way).
template <int CTRL>
__device__ __forceinline__ double lin_dpp_add(double x) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), CTRL, 0xf, 0xf, false);
    return x + __hiloint2double(hi, lo);
}
__device__ __forceinline__ double lin_wave_sum(double x) {
    x = lin_dpp_add<0xB1>(x);          // quad_perm [1, 0, 3, 2]
    x = lin_dpp_add<0x4E>(x);          // quad_perm [2, 3, 0, 1]
    x = lin_dpp_add<0x141>(x);         // row_half_mirror
    x = lin_dpp_add<0x140>(x);         // row_mirror
    double tot = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r)
        tot += __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), 16 * r), __builtin_amdgcn_readlane(__double2loint(x), 16 * r));
    return tot;
}
// e^x in float64 (|x| < 700): k = round(x / ln 2), degree-13 Taylor polynomial on |r| <= ln 2 / 2 (truncation 5e-18), one ldexp.
// ~20 fused multiply-adds on the updater's critical path instead of the library routine's ~3x that.
template <bool InLoop = false>
__device__ __forceinline__ double lin_exp(double x) {
    // InLoop: every coefficient through an empty asm that pins it to scalar registers (the four-block updater's step loop: left
    // alone, hoisted out of the loop into vector registers, the 14 float64 constants pushed the run-time instantiation into scratch)
    auto c = [](double v) __attribute__((always_inline)) { if constexpr (InLoop) asm volatile("" : "+s"(v)); return v; };
    const double k = rint(x * c(1.4426950408889634));
    double r = fma(-k, c(6.93147180369123816490e-01), x);
    r = fma(-k, c(1.90821492927058770002e-10), r);
    double p = c(1.0 / 6227020800.0);
    p = fma(p, r, c(1.0 / 479001600.0)); p = fma(p, r, c(1.0 / 39916800.0)); p = fma(p, r, c(1.0 / 3628800.0)); p = fma(p, r, c(1.0 / 362880.0));
    p = fma(p, r, c(1.0 / 40320.0)); p = fma(p, r, c(1.0 / 5040.0)); p = fma(p, r, c(1.0 / 720.0)); p = fma(p, r, c(1.0 / 120.0));
    p = fma(p, r, c(1.0 / 24.0)); p = fma(p, r, c(1.0 / 6.0)); p = fma(p, r, 0.5); p = fma(p, r, 1.0); p = fma(p, r, 1.0);
    return ldexp(p, (int)k);
}
// element (r, c) of the symmetric moment matrix in the packed image (upper block triangle, accumulator layout)
__device__ __forceinline__ int lin_m_index(int NB, int r, int c) {
    const int br = r >> 4, bc = c >> 4;
    const int b1 = br <= bc ? br : bc, b2 = br <= bc ? bc : br, i = br <= bc ? (r & 15) : (c & 15), j = br <= bc ? (c & 15) : (r & 15);
    return lin_blk(NB, b1, b2) * 256 + (((i >> 2) * 16 + j) << 2) + (i & 3);
}
// ONE updater for three and four feature blocks.  Where the two differ, a compile-time policy below says how and why; everything
// else -- carve, the M offset rows, the SM -> P1 -> G chain, the element gradients, the dWd wave, the KL wave, the Adam phase,
// store_state -- is one text.
template <int NB, int DT, int LT>
struct LinUpdM {
    static_assert(NB == 3 || NB == 4, "three or four feature blocks");
    static constexpr int NFP = 16 * NB;
    static constexpr int KD = DT ? (DT + 3) / 4 : (NB == 3 ? 4 : 8);                   // k-steps over the data dimension (run-time: D <= 16 resp. 31)
    static constexpr int RL1 = LT ? (LT > 16 ? (LT - 16 + 3) / 4 : 0) : 4;             // registers of the second latent row tile that can hold a row
    static constexpr int NM = 4 + RL1 + 2 * KD + 1;                                    // M values per chain lane
    // ---- policies ----
    static constexpr int PT = KD > 4 ? 2 : 1;                                          // row tiles of P1 (d = 16 pt + g + 4 r) and of dWd^T
    // part[]: the chain waves' three sums at 3 w .. 3 w + 2, the dWd wave's at 3 NB, the KL sum at 3 NB + 3, the bias corrections behind it
    static constexpr int NPART = NB == 3 ? 16 : 20;
    // the next batch's M loaded under this step when its reducers are done already: three blocks only (four have no registers
    // left for a second set of up to 25 values -- they would go to scratch)
    static constexpr bool PREFETCH = NB == 3;
    // this thread's parameters and Adam moments behind pk / mk / vk: three blocks in registers; four in LDS, [3][LKOUT][512] -- in
    // registers they went to scratch
    static constexpr bool PMV_LDS = NB == 4;
    // chain lanes: image offsets of their M values.  Three blocks in registers; four [NM][64 NB] in LDS -- formed once per launch,
    // read back per step (held in registers across the step loop, up to 25 of them, they pushed the run-time instantiation into scratch)
    static constexpr bool MO_LDS = NB == 4;
    // the output map: three blocks out_index's special lanes (see there; -1: no output), four the plain idx = t + 512 k (no holes)
    static constexpr bool SPECIAL_LANES = NB == 3;
    // publish_params: with the special lanes a thread has at most ONE output behind an exponential, formed once behind the loop;
    // the plain map forms it where it meets one
    static constexpr bool DEFER_EXP = SPECIAL_LANES;
    // four blocks: the thread index laundered, so that the LDS addresses of a step are formed in it and not hoisted out of the
    // launch's step loop, where they would occupy the registers the chain needs
    static constexpr bool LAUNDER_T = NB == 4;
    // the chain waves' s_l / be_l for the element gradients: one row tile reads them in front of G's products (read again: held
    // across the barrier they spill), two behind the products -- in front, next to G's 2 KD weights, they spill
    static constexpr bool SLBL_FIRST = PT == 1;
    // load_state's two exponentials (no epsilon leaf) with their coefficients in scalar registers, as in the step loop: four blocks
    static constexpr bool LOAD_EXP_SCALAR = NB == 4;

    int D, L, P, fone, off_be, off_wd, off_bd, off_epsp, off_eps;
    double *Wed, *Wdd, *bed, *bdd, *sd, *elv, *lvd, *scal, *part, *P1s, *gq;
    float p[LKOUT], m[LKOUT], v[LKOUT];                                                // !PMV_LDS
    float* pmv;                                                                        // PMV_LDS
    int mo[NM];                                                                        // !MO_LDS
    int* mos;                                                                          // MO_LDS
    __device__ __forceinline__ float& pk(int k) { if constexpr (PMV_LDS) return pmv[k * LNT + threadIdx.x]; else return p[k]; }
    __device__ __forceinline__ float& mk(int k) { if constexpr (PMV_LDS) return pmv[(LKOUT + k) * LNT + threadIdx.x]; else return m[k]; }
    __device__ __forceinline__ float& vk(int k) { if constexpr (PMV_LDS) return pmv[(2 * LKOUT + k) * LNT + threadIdx.x]; else return v[k]; }

    // (L > 32 would need a third latent row tile; D <= 4 KD: 16 at three blocks, where four row registers hold P1, 32 at four)
    static __host__ __device__ constexpr bool shape_ok(int D, int L) { return L <= 32 && L + 2 * D + 1 <= NFP && D <= 4 * KD; }
    static __host__ __device__ constexpr size_t lds_bytes(int D, int L, int P) {
        return sizeof(double) * ((size_t)2 * D * L + 4 * L + D + 8 + NPART + 16 * PT * NFP + (size_t)(P + kExtra + 7)) +
               (MO_LDS ? sizeof(int) * NM * 64 * NB : 0) + (PMV_LDS ? sizeof(float) * 3 * LKOUT * LNT : 0);
    }
    // Which output lives in slot k of thread t (-1: none).  With SPECIAL_LANES the special outputs -- the loss slots P .. P + 3 and
    // epsilon, the ones behind float64 scalar chains (the four sums; e^{eps/2} and 1 / sigma^2 when the parameters are published) --
    // are the ONLY output of the first lanes of the last wave; the plain outputs fill slot 0 of every other thread in order, and
    // those that are left over go to further slots from thread kOvfTop down (the wave in front of the special one: no chain wave,
    // no special lane), so no wave runs a plain Adam update and a special lane's chain one behind the other.  load_state,
    // publish_params, step and store_state all go through this map.
    static constexpr int kSpecT0 = LNT - 64, kOvfTop = kSpecT0 - 1;
    static_assert(LNT - (kExtra + 1) - kOvfTop > 32 && kOvfTop + 1 > 32, "publish_params: one exponential per thread needs two slots of a thread more than L <= 32 outputs apart");
    __device__ __forceinline__ int out_index(int t, int k) const {
        if constexpr (!SPECIAL_LANES) return t + LNT * k;
        const int ns = kExtra + (off_eps >= 0 ? 1 : 0), np = P - (off_eps >= 0 ? 1 : 0);        // special lanes; plain outputs
        int r;
        if (k == 0) {
            if (t >= kSpecT0 && t < kSpecT0 + ns) return t - kSpecT0 < kExtra ? P + (t - kSpecT0) : off_eps;
            r = t < kSpecT0 ? t : t - ns;
        } else {
            if (t > kOvfTop) return -1;
            r = LNT - ns + (kOvfTop + 1) * (k - 1) + (kOvfTop - t);
        }
        if (r >= np) return -1;
        return r + ((off_eps >= 0 && r >= off_eps) ? 1 : 0);
    }
    // (uniform) does any thread hold an output in slot k?
    __device__ __forceinline__ bool slot_used(int k) const {
        if constexpr (!SPECIAL_LANES) return LNT * k < P + 3;
        return k == 0 || LNT - (kExtra + (off_eps >= 0 ? 1 : 0)) + (kOvfTop + 1) * (k - 1) < P - (off_eps >= 0 ? 1 : 0);
    }

    __device__ __forceinline__ void carve(const LinArgs& a, char* smem) {
        D = DT ? DT : a.D; L = LT ? LT : a.L; P = a.P; fone = L + 2 * D; off_eps = a.off_eps;
        off_be = D * L; off_wd = off_be + L; off_bd = off_wd + L * D; off_epsp = off_bd + D;
        Wed = reinterpret_cast<double*>(smem); Wdd = Wed + D * L; bed = Wdd + L * D; bdd = bed + L; sd = bdd + D; elv = sd + L; lvd = elv + L;
        scal = lvd + L; part = scal + 8; P1s = part + NPART; gq = P1s + 16 * PT * NFP;
        if constexpr (MO_LDS) mos = reinterpret_cast<int*>(gq + P + kExtra + 7);
        if constexpr (PMV_LDS) pmv = reinterpret_cast<float*>(smem + sizeof(double) * (size_t)(gq + P + kExtra + 7 - Wed) + (MO_LDS ? sizeof(int) * NM * 64 * NB : 0));
    }
    __device__ __forceinline__ void load_state(const LinArgs& a) {
        const int t = threadIdx.x;
#pragma unroll
        for (int k = 0; k < LKOUT; ++k) {
            const int o = out_index(t, k), idx = (!SPECIAL_LANES || o >= 0) && o < P ? o : P - 1;
            pk(k) = a.params[idx]; mk(k) = a.m[idx]; vk(k) = a.v[idx];
        }
        if (off_eps < 0 && t == 0) { const double e = (double)a.eps_cli; scal[0] = e; scal[1] = lin_exp<LOAD_EXP_SCALAR>(0.5 * e); scal[2] = lin_exp<LOAD_EXP_SCALAR>(-e); }
        // image offsets of this lane's M values (chain waves: wave w = feature block w)
        if (!MO_LDS || t < 64 * NB) {
            const int lane = t & 63, j = lane & 15, g = lane >> 4, f = min(16 * (t >> 6) + j, NFP - 1);
            int k = 0;
            auto put = [&](int row) __attribute__((always_inline)) {
                if constexpr (MO_LDS) mos[(k++) * 64 * NB + t] = lin_m_index(NB, row, f); else mo[k++] = lin_m_index(NB, row, f);
            };
#pragma unroll
            for (int r = 0; r < 4; ++r) put(g + 4 * r);                                  // z1 rows 0 .. 15
#pragma unroll
            for (int r = 0; r < RL1; ++r) put(min(16 + g + 4 * r, NFP - 1));             // z1 rows 16 ..
#pragma unroll
            for (int r = 0; r < KD; ++r) put(min(L + g + 4 * r, NFP - 1));               // x rows
#pragma unroll
            for (int r = 0; r < KD; ++r) put(min(L + D + g + 4 * r, NFP - 1));           // z2 rows
            put(fone);
        }
    }
    // (chain lanes only; MO_LDS: each reads back the offsets it wrote itself)
    __device__ __forceinline__ void fetch_M(const double* M_in, double (&r)[NM]) const {
        int o[NM];
        if constexpr (MO_LDS) {
            const int* mt = mos + threadIdx.x;
#pragma unroll
            for (int k = 0; k < NM; ++k) o[k] = mt[k * 64 * NB];
        } else {
#pragma unroll
            for (int k = 0; k < NM; ++k) o[k] = mo[k];
        }
#pragma unroll
        for (int k = 0; k < NM; ++k) r[k] = ld_sc1(M_in + o[k]);
    }
    // float64 copies of this thread's own parameters into the arrays the products read
    __device__ __forceinline__ void publish_params(const LinArgs& a) {
        int t = threadIdx.x;
        if constexpr (LAUNDER_T) asm volatile("" : "+v"(t));
        // e^{lv / 2} and e^{eps / 2}, e^{-eps}: the same instruction stream for the latent lanes and the epsilon lane
        auto publish_exp = [&](int i, double pv) __attribute__((always_inline)) {
            const bool is_eps = i == off_eps;
            const double e = is_eps ? pv * (double)a.eps_cli : pv, h = lin_exp<true>(0.5 * e);      // (coefficients in scalar registers: hoisted into vector registers they push the step loop into scratch)
            if (is_eps) {
                const double q = h * h;
                double r = __builtin_amdgcn_rcp(q);                    // 1 / sigma^2: hardware seed, two Newton steps (full double precision)
                r = fma(fma(-q, r, 1.0), r, r); r = fma(fma(-q, r, 1.0), r, r);
                scal[0] = e; scal[1] = h; scal[2] = r;
            }
            else { sd[i - off_epsp] = h; elv[i - off_epsp] = h * h; lvd[i - off_epsp] = pv; }
        };
        int ei = -1;                                                   // DEFER_EXP: the ONE output of this thread behind an exponential, if any
        double epv = 0.0;
#pragma unroll
        for (int k = 0; k < LKOUT; ++k) {
            if (SPECIAL_LANES && !slot_used(k)) break;
            const int i = out_index(t, k);
            const double pv = (double)pk(k);
            if (SPECIAL_LANES && (i < 0 || i >= P)) continue;
            if (i < off_be) Wed[i] = pv;
            else if (i < off_wd) bed[i - off_be] = pv;
            else if (i < off_bd) Wdd[i - off_wd] = pv;
            else if (i < off_epsp) bdd[i - off_bd] = pv;
            // (DEFER_EXP, at most ONE such output per thread: the latent lanes are L <= 32 consecutive plain outputs, and two slots of
            // one thread hold plain outputs at least 2 (kOvfTop - t) + LNT - kOvfTop - 5 >= 60 apart -- slot 0 holds rank t, slot 1 rank
            // LNT - ns + kOvfTop - t with t <= kOvfTop, later slots kOvfTop + 1 further each; the epsilon lane has slot 0 only)
            else if (i < off_epsp + L || i == off_eps) {
                if constexpr (DEFER_EXP) { ei = i; epv = pv; } else publish_exp(i, pv);
            }
        }
        if constexpr (DEFER_EXP) { if (ei >= 0) publish_exp(ei, epv); }
    }
    // one step.  In: parameters published and a barrier behind them; mreg = this lane's values of the batch's M (chain waves).
    // Out: p / m / v updated, gout[] this thread's gradients.  Ends WITHOUT a barrier: the caller's next publish_params writes arrays
    // that only the phases before this step's last barrier read.
    // next_cnt / M_next: the NEXT batch's reducer counter and M (nullptr: none); if its reducers are done already, its M is loaded
    // into mnext under this step's second half and have_next says so (PREFETCH).
    __device__ __forceinline__ void step(const LinArgs& a, int tstep, const double (&mreg)[NM], float (&gout)[LKOUT], const unsigned* next_cnt,
                                         unsigned per_set, const double* M_next, double (&mnext)[NM], bool& have_next) {
        int t = threadIdx.x;
        if constexpr (LAUNDER_T) asm volatile("" : "+v"(t));
        const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63, j = lane & 15, g = lane >> 4;
        LIN_STAMP(1);
        if (PREFETCH && t == 64 * (NB + 2)) scal[4] = (next_cnt && __hip_atomic_load(next_cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= per_set) ? 1.0 : 0.0;
        const double eps = scal[0], sigma = scal[1], inv_var = scal[2], inv_bt = (double)a.inv_bt, c0 = inv_var * inv_bt;
        d4 sm[2], p1;
        [[maybe_unused]] d4 p1b;                                       // PT == 2: P1's second row tile, d = 16 + g + 4 r
        auto p1row = [&](int r) -> double { return r < 4 ? p1[r & 3] : p1b[r & 3]; };     // P1 rows 4 r + g, r < 4 PT
        double musq_p = 0.0, ssq_p = 0.0, z2r_p = 0.0;
        const int f = 16 * wave + j;                                   // chain waves: this lane's feature column
        // The chain's WEIGHT operands (functions of the published parameters only) are read from LDS up front: left where they are
        // used, hipcc issues each ds_read right in front of its MFMA and waits for it -- ds_read, s_waitcnt lgkmcnt(0), v_mfma, 17
        // times: an LDS round trip (~130 cycles) on top of every 64-cycle product of the dependent chain.
        // (SM's and P1's weights here; G's and the dWd wave's operands in ONE batch behind the barrier: held across it they spill)
        double awSMr[KD][2], awP1r[PT][4 + (RL1 ? RL1 : 1)];
        auto awSM = [&](int kk, int lt) -> double& { return awSMr[kk][lt]; };
        auto awP1 = [&](int r) -> double& { return awP1r[0][r]; };
        if (wave < NB) {
#pragma unroll
            for (int kk = 0; kk < KD; ++kk)
#pragma unroll
                for (int lt = 0; lt < 2; ++lt) {
                    const int dd = 4 * kk + g, l = 16 * lt + j;
                    const double w1 = Wed[min(dd, D - 1) * L + min(l, L - 1)];
                    awSM(kk, lt) = (dd < D && l < L && (lt == 0 || RL1 > 0)) ? w1 : 0.0;
                }
#pragma unroll
            for (int r = 0; r < 4 + RL1; ++r) {
                const int l = (r < 4 ? 4 * r : 16 + 4 * (r - 4)) + g;
                const double w = Wdd[min(l, L - 1) * D + min(j, D - 1)];
                awP1(r) = (j < D && l < L) ? w : 0.0;
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        if (wave < NB) {
            const double* Mz = mreg; const double* Mx = mreg + 4 + RL1; const double* Mz2 = Mx + KD; const double Mone = mreg[NM - 1];
            // ---- SM ----
#pragma unroll
            for (int lt = 0; lt < 2; ++lt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int l = 16 * lt + g + 4 * r;
                    const bool ok = l < L && (lt == 0 || r < RL1);
                    const double sv = sd[min(l, L - 1)], bv = bed[min(l, L - 1)];
                    const double slv = ok ? sv : 0.0, blv = ok ? bv : 0.0;
                    sm[lt][r] = (lt == 0 || r < RL1) ? slv * Mz[lt == 0 ? r : min(4 + r, 3 + RL1)] + blv * Mone : 0.0;
                }
#pragma unroll
            for (int kk = 0; kk < KD; ++kk) {
#pragma unroll
                for (int lt = 0; lt < 2; ++lt) {
                    if (lt == 1 && RL1 == 0) continue;
                    sm[lt] = __builtin_amdgcn_mfma_f64_16x16x4f64(awSM(kk, lt), Mx[kk], sm[lt], 0, 0, 0);
                }
            }
            // ---- P1 ----
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int d = g + 4 * r;
                p1[r] = (r < KD && d < D) ? -Mx[min(r, KD - 1)] + sigma * Mz2[min(r, KD - 1)] + bdd[min(d, D - 1)] * Mone : 0.0;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) p1 = __builtin_amdgcn_mfma_f64_16x16x4f64(awP1(r), sm[0][r], p1, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < RL1; ++r) p1 = __builtin_amdgcn_mfma_f64_16x16x4f64(awP1(4 + r), sm[1][r], p1, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) P1s[(g + 4 * r) * NFP + f] = p1[r];
            if constexpr (PT == 2) {                                   // rows d = 16 .. 31: the same k-steps with the second tile's weights
                // (read here, behind the first tile's products: read up front with the others they went to scratch)
#pragma unroll
                for (int r = 0; r < 4 + RL1; ++r) {
                    const int l = (r < 4 ? 4 * r : 16 + 4 * (r - 4)) + g;
                    const double w = Wdd[min(l, L - 1) * D + min(16 + j, D - 1)];
                    awP1r[1][r] = (16 + j < D && l < L) ? w : 0.0;
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int d = 16 + g + 4 * r;
                    p1b[r] = (4 + r < KD && d < D) ? -Mx[min(4 + r, KD - 1)] + sigma * Mz2[min(4 + r, KD - 1)] + bdd[min(d, D - 1)] * Mone : 0.0;
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) p1b = __builtin_amdgcn_mfma_f64_16x16x4f64(awP1r[1][r], sm[0][r], p1b, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < RL1; ++r) p1b = __builtin_amdgcn_mfma_f64_16x16x4f64(awP1r[1][4 + r], sm[1][r], p1b, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r) P1s[(16 + g + 4 * r) * NFP + f] = p1b[r];
            }
        } else if (wave == NB + 1) {
            // 1 + lv - e^{lv} summed over the latent dimension (the closed-form KL term of the loss)
            const double kl = lane < L ? 1.0 + lvd[min(lane, L - 1)] - elv[min(lane, L - 1)] : 0.0;
            const double tot = lin_wave_sum(kl);
            if (lane == 0) {
                part[3 * NB + 3] = tot;
                // Adam's bias corrections 1 - beta^t for everybody (float, as the other paths compute them)
                part[3 * NB + 4] = (double)(-expm1f((float)tstep * -0.10536051565782628f)); part[3 * NB + 5] = (double)(-expm1f((float)tstep * -0.0010005003335835335f));
            }
        }
        LIN_STAMP(2);
        __syncthreads();                                               // P1 is in LDS
        LIN_STAMP(3);
        have_next = PREFETCH && scal[4] != 0.0;
        if (wave < NB) {
            if (have_next) fetch_M(M_next, mnext);
            // ---- G = Wd P1 ---- (its 2 KD weights in one batch of LDS reads first)
            double awGr[KD][2];
#pragma unroll
            for (int kk = 0; kk < KD; ++kk)
#pragma unroll
                for (int lt = 0; lt < 2; ++lt) {
                    const int dd = 4 * kk + g, l = 16 * lt + j;
                    const double w2 = Wdd[min(l, L - 1) * D + min(dd, D - 1)];
                    awGr[kk][lt] = (l < L && dd < D && (lt == 0 || RL1 > 0)) ? w2 : 0.0;
                }
            double sl[2][4], bl[2][4];
            auto read_sl_bl = [&]() __attribute__((always_inline)) {
#pragma unroll
                for (int lt = 0; lt < 2; ++lt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int l = 16 * lt + g + 4 * r;
                        const bool ok = l < L && (lt == 0 || r < RL1);
                        const double sv = sd[min(l, L - 1)], bv = bed[min(l, L - 1)];
                        sl[lt][r] = ok ? sv : 0.0; bl[lt][r] = ok ? bv : 0.0;
                    }
            };
            if constexpr (SLBL_FIRST) read_sl_bl();
            __builtin_amdgcn_sched_barrier(0);
            d4 G[2];
            G[0] = d4{0.0, 0.0, 0.0, 0.0}; G[1] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int r = 0; r < KD; ++r) {
#pragma unroll
                for (int lt = 0; lt < 2; ++lt) {
                    if (lt == 1 && RL1 == 0) continue;
                    G[lt] = __builtin_amdgcn_mfma_f64_16x16x4f64(awGr[r][lt], p1row(r), G[lt], 0, 0, 0);
                }
            }
            if constexpr (!SLBL_FIRST) read_sl_bl();
            // ---- the gradients that are elements of these tiles ----
            const double* Mz = mreg;
            const bool is_x = f >= L && f < L + D, is_z2 = f >= L + D && f < fone, is_one = f == fone, is_z1 = f < L;
            if (is_x || is_one) {
                const int base = is_x ? (f - L) * L : off_be;          // dWe[dd][:] resp. dbe
#pragma unroll
                for (int lt = 0; lt < 2; ++lt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        if (lt == 1 && r >= RL1) continue;
                        const int l = 16 * lt + g + 4 * r;
                        if (l < L) {
                            const double q = sm[lt][r] - sl[lt][r] * Mz[lt == 0 ? r : min(4 + r, 3 + RL1)];           // Q = E M
                            gq[base + l] = c0 * G[lt][r] + q * inv_bt;
                            musq_p += (is_x ? Wed[base + l] : bl[lt][r]) * q;
                        }
                    }
            }
            if (is_one) {
#pragma unroll
                for (int r = 0; r < 4 * PT; ++r) {
                    const int d = g + 4 * r;
                    if (d < D) { gq[off_bd + d] = c0 * p1row(r); ssq_p += bdd[d] * p1row(r); }
                }
            }
            if (is_z1 && (j & 3) == g) {                               // the lane that holds G[f][f]
                const int lt = f >> 4, r = j >> 2;
                double gll = 0.0;
#pragma unroll
                for (int q2 = 0; q2 < 2; ++q2)
#pragma unroll
                    for (int r2 = 0; r2 < 4; ++r2) gll = (q2 == lt && r2 == r) ? G[q2][r2] : gll;
                gq[off_epsp + f] = 0.5 * sd[f] * c0 * gll - 0.5 * (1.0 - elv[f]) * (double)a.rows_over_bt;
            }
            if (is_x || is_z2) {                                       // the diagonal entries P1[d][x_d], P1[d][z2_d] of the residual sums
                const int d = is_x ? f - L : f - L - D;
                if ((d & 3) == g) {
                    double pd = 0.0;
#pragma unroll
                    for (int r2 = 0; r2 < 4 * PT; ++r2) { const bool hit = r2 == (d >> 2); const double pr = p1row(r2); pd = hit ? pr : pd; }
                    if (is_x) ssq_p -= pd; else { ssq_p += sigma * pd; z2r_p += pd; }
                }
            }
            musq_p = lin_wave_sum(musq_p); ssq_p = lin_wave_sum(ssq_p); z2r_p = lin_wave_sum(z2r_p);
            if (lane == 0) { part[3 * wave] = ssq_p; part[3 * wave + 1] = musq_p; part[3 * wave + 2] = z2r_p; }
        } else if (wave == NB) {
            // ---- dwd^T[d][l] = s_l P1[d][l] + be_l P1[d][one] + sum_dd P1[d][x_dd] We[dd][l]  (rows d = 16 dt + g + 4 r, columns l = 16 ct + j) ----
            // (every LDS operand first -- We was read in front of the barrier --, then the products back to back: see the chain waves;
            // PT row tiles one after the other)
            double wsum = 0.0;
#pragma unroll
            for (int dt = 0; dt < PT; ++dt) {
                d4 C[2];
                double avk[KD], p1l[2][4], p1o[4], dw_sr[2], dw_br[2], dw_wr[KD][2], dw_dr[2][4];
                auto dw_s = [&](int ct) -> double& { return dw_sr[ct]; };
                auto dw_b = [&](int ct) -> double& { return dw_br[ct]; };
                auto dw_w = [&](int kk, int ct) -> double& { return dw_wr[kk][ct]; };
                auto dw_d = [&](int ct, int r) -> double& { return dw_dr[ct][r]; };
                const int d0 = 16 * dt;
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) {
                    const int l = 16 * ct + j, lc = min(l, L - 1);
                    const double s_l = sd[lc], b_l = bed[lc];
                    dw_s(ct) = l < L ? s_l : 0.0; dw_b(ct) = l < L ? b_l : 0.0;
#pragma unroll
                    for (int kk = 0; kk < KD; ++kk) {
                        const int dd = 4 * kk + g;
                        const double w = Wed[min(dd, D - 1) * L + lc];
                        dw_w(kk, ct) = (dd < D && l < L) ? w : 0.0;
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) dw_d(ct, r) = Wdd[lc * D + min(d0 + g + 4 * r, D - 1)];
                }
#pragma unroll
                for (int kk = 0; kk < KD; ++kk) avk[kk] = P1s[(d0 + j) * NFP + min(L + 4 * kk + g, NFP - 1)];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    p1o[r] = P1s[(d0 + g + 4 * r) * NFP + fone];
#pragma unroll
                    for (int ct = 0; ct < 2; ++ct) p1l[ct][r] = P1s[(d0 + g + 4 * r) * NFP + min(16 * ct + j, L - 1)];
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) {
                    if (ct == 1 && RL1 == 0) continue;
                    const int l = 16 * ct + j;
#pragma unroll
                    for (int r = 0; r < 4; ++r) C[ct][r] = dw_s(ct) * p1l[ct][r] + dw_b(ct) * p1o[r];
#pragma unroll
                    for (int kk = 0; kk < KD; ++kk) C[ct] = __builtin_amdgcn_mfma_f64_16x16x4f64(avk[kk], dw_w(kk, ct), C[ct], 0, 0, 0);
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int d = d0 + g + 4 * r;
                        if (l < L && d < D) { gq[off_wd + l * D + d] = c0 * C[ct][r]; wsum += dw_d(ct, r) * C[ct][r]; }
                    }
                }
            }
            wsum = lin_wave_sum(wsum);
            if (lane == 0) part[3 * NB] = wsum;
        }
        LIN_STAMP(4);
        __syncthreads();                                               // every gradient and partial sum is in LDS
        LIN_STAMP(5);
        const double rows = (double)a.rows;
        const float bc1 = (float)part[3 * NB + 4], bc2 = (float)part[3 * NB + 5];
#pragma unroll
        for (int k = 0; k < LKOUT; ++k) {
            if (!slot_used(k)) break;                                  // (uniform) nothing lives up here
            const int idx = out_index(t, k);
            double gd = 0.0;
            if ((!SPECIAL_LANES || idx >= 0) && idx < P && idx != off_eps) gd = gq[idx];
            else if ((!SPECIAL_LANES || (k == 0 && idx >= 0)) && (idx == off_eps || (idx >= P && idx < P + 3))) {
                // in wave order: ssq from the NB chain waves and the dWd wave (slots 0, 3 .. 3 NB), musq and z2r from the chain waves
                double ssq = part[0] + part[3] + part[6] + part[9], musq = part[1] + part[4] + part[7], z2r = part[2] + part[5] + part[8];
                if constexpr (NB == 4) { ssq += part[12]; musq += part[10]; z2r += part[11]; }
                const double klc = part[3 * NB + 3];
                if (idx == off_eps) gd = (double)a.eps_cli * (-0.5 * ssq * inv_var + 0.5 * rows * D + 0.5 * sigma * z2r * inv_var) * inv_bt;
                else {
                    const double dkl = (0.5 * musq - 0.5 * rows * klc) * inv_bt;
                    const double mse = (0.5 * ssq * inv_var + 0.5 * rows * D * ((double)kLog2Pi + eps)) * inv_bt;
                    gd = idx == P ? dkl + mse : (idx == P + 1 ? dkl : mse);
                }
            }
            const float gf = (float)gd;
            gout[k] = gf;
            if (idx == P && a.loss_hist) a.loss_hist[(long long)(tstep - 1) % a.loss_hist_cap] = gf;
            if ((!SPECIAL_LANES || idx >= 0) && idx < P) adam_apply_f(pk(k), gf, mk(k), vk(k), a.lr, bc1, bc2);
        }
        LIN_STAMP(6);
    }
    __device__ __forceinline__ void store_state(const LinArgs& a, const float (&gout)[LKOUT], int tstep) {
        const int t = threadIdx.x;
#pragma unroll
        for (int k = 0; k < LKOUT; ++k) {
            const int idx = out_index(t, k);
            if ((!SPECIAL_LANES || idx >= 0) && idx < P + kExtra) a.grads[idx] = gout[k];
            if ((!SPECIAL_LANES || idx >= 0) && idx < P) { a.params[idx] = pk(k); a.m[idx] = mk(k); a.v[idx] = vk(k); }
        }
        if (t == 0) a.step_dev[0] = tstep;
    }
};
// what lin_plan asks of the run-time instantiations.  The LDS request keeps one workgroup per CU: the byte counts are those of the
// two formulas this struct replaced, at P = 2 D L + 2 L + D + 1 (the epsilon leaf included)
static_assert(LinUpdM<3, 0, 0>::shape_ok(12, 20) && LinUpdM<3, 0, 0>::shape_ok(16, 1) && !LinUpdM<3, 0, 0>::shape_ok(17, 1) && !LinUpdM<3, 0, 0>::shape_ok(1, 33) &&
              LinUpdM<4, 0, 0>::shape_ok(20, 20) && LinUpdM<4, 0, 0>::shape_ok(20, 10) && LinUpdM<4, 0, 0>::shape_ok(31, 1) && !LinUpdM<4, 0, 0>::shape_ok(1, 33),
              "shapes of the matrix-core updater");
static_assert(LinUpdM<3, 0, 0>::lds_bytes(12, 20, 533) == 15264 && LinUpdM<3, 0, 0>::lds_bytes(16, 1, 51) == 7248 &&
              LinUpdM<4, 0, 0>::lds_bytes(20, 20, 861) == 80960 && LinUpdM<4, 0, 0>::lds_bytes(31, 1, 96) == 68416, "LDS request of the matrix-core updater");

// ---- launch-per-step form ---------------------------------------------------------------------------------------------------------
template <int NB, int DT, int LT>
__global__ __launch_bounds__(LNT) void lin_step_kernel(const LinArgs a) {
    extern __shared__ __attribute__((aligned(16))) char lin_smem[];
    const int b = blockIdx.x, t = threadIdx.x;
    constexpr int NO = NB * (NB + 1) / 2 * 256;
    if (b < a.has_update) {
        LinUpd<NB, DT, LT> u;
        u.carve(a, lin_smem);
        LIN_STAMP(0);
        const int tstep = a.step_dev[0] + 1;
        u.load_state(a);
        u.publish_params();
        u.template expand_M<false>(a.M_in);
        __syncthreads();
        float g[LKOUT];
        u.step(a, tstep, g);
        u.store_state(a, g, tstep);
        LIN_STAMP(7);
    } else if (b < a.has_update + a.n_reduce) {
        lin_reduce<false>(a.partial_in, a.M_out, a.ntiles, lin_smem, b - a.has_update, NO);
    } else {
        const int tile = b - a.has_update - a.n_reduce;
        const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
        const LinTile tl(a.D, a.L, a.T);
        const int stride = max(tl.bytes, lin_scratch_bytes(NB)), v_off = stride, c_off = v_off + 4 * a.T;
        for (int p = wave; p < tl.np; p += LNW) lin_issue_piece(a, tl, a.x, a.z1, a.z2, tile, p, lin_smem, lane);
        lin_write_vcol(reinterpret_cast<float*>(lin_smem + v_off), a.T, (int)min((long long)a.T, (long long)a.B - (long long)tile * a.T), t);
        if (t == 0) *reinterpret_cast<float*>(lin_smem + c_off) = 0.f;
        lin_wait_vmcnt<0>();
        lin_barrier();
        lin_fix_ragged(a, tl, a.x, a.z1, a.z2, tile, lin_smem, t);
        f32x4 acc[NB * (NB + 1) / 2];
        lin_tile_products<NB, 0, LNW>(a, tl, lin_smem, 0, v_off, c_off, acc, lane, wave, [](int) {});
        lin_barrier();                                         // every wave has read its last operand: the slot turns into scratch
        lin_tile_combine<NB, false, LNW>(acc, lin_smem, a.partial_out + (long long)tile * NO, t, wave, lane);
    }
}

// ---- persistent form: up to kLinMaxPersist steps in one launch ----------------------------------------------------------------
// GEN: the batches are not read from HBM but DRAWN by the streamers, tile by tile, straight into the LDS slots: the Philox work
// items of vaek_make_batch (rng_dev.h: same counters, same functions, same bits) for the rows of a tile, dealt to the 512
// threads and issued between the k-steps of an earlier tile exactly where the other form issues its LDS-DMA pieces -- the loop
// body of model.py:221-222 (get_batch, sample_latent, train_step) with no batch ever in HBM.  The RNG step of the batch that
// takes the Adam counter from t to t + 1 is t, as in trainer.GraphLoop / vaek_train_step_gen.
template <int NB, int DT, int LT, int JT, bool GEN>
__global__ __launch_bounds__(LNT, 2) void lin_persist_kernel(const LinArgs a, const std::conditional_t<GEN, BatchArgs, LinPtrs> src) {       // one workgroup per CU (its LDS request sees to that)
    extern __shared__ __attribute__((aligned(16))) char lin_smem[];
    const int b = blockIdx.x, t = threadIdx.x, N = a.n_steps;
    constexpr int NO = NB * (NB + 1) / 2 * 256;
    const int per_set = a.n_reduce / a.sets;                  // reducer workgroups per set
    if (b < a.has_update) {
        // ---- the updater: one workgroup, parameters and Adam state in registers / LDS across all N steps (the host sends only
        // shapes the matrix-core updater covers into this form: LinPlan::persist) ------------------------------------------------
        LinUpdM<NB, DT, LT> u;
        u.carve(a, lin_smem);
        int tstep = a.step_dev[0];
        u.load_state(a);
        float g[LKOUT];
#pragma unroll
        for (int k = 0; k < LKOUT; ++k) g[k] = 0.f;
        constexpr int NM = LinUpdM<NB, DT, LT>::NM;
        double mreg[NM], mnext[NM];
        bool have_next = false;
        LIN_STAMP(10);
        int sl = a.slot_upd;                                  // the slot of batch n, and of the batch after it
        for (int n = 0; n < N; ++n) {
            const int sl_next = sl + 1 == kLinSlots ? 0 : sl + 1;
            LIN_STAMP(0);
            u.publish_params(a);
            LIN_STAMP(9);
            if (!have_next) {
                lin_wait_count(a.cnt_reduce + sl, (unsigned)per_set, a.status, (1u << 28) | ((unsigned)n << 16));     // (also the barrier behind publish_params)
                if (t < 64 * NB) u.fetch_M(a.M_base + (long long)sl * NO, mreg);
            } else {
                __syncthreads();
#pragma unroll
                for (int k = 0; k < NM; ++k) mreg[k] = mnext[k];
            }
            LIN_STAMP(8);
            ++tstep;
            u.step(a, tstep, mreg, g, n + 1 < N ? a.cnt_reduce + sl_next : nullptr, (unsigned)per_set, a.M_base + (long long)sl_next * NO, mnext, have_next);
            LIN_STAMP(7);
            { [[maybe_unused]] unsigned long long te = 0; LIN_NOWQ(te); LIN_PUT(64 + n, te); }
            sl = sl_next;
        }
        u.store_state(a, g, tstep);
        // every reducer has added to the counter of the last batch updated here, every streamer long before: nobody reads or writes
        // the arrival counters of the batches this launch UPDATED any more -- zero them for the slots' next batches (write-through;
        // the kernel boundary orders them).  Batches streamed here and left to the next launch keep theirs.
        for (int k = t; k < N * kLinShards; k += LNT) {
            int s = a.slot_upd + k / kLinShards;
            s = s >= kLinSlots ? s - kLinSlots : s;
            __hip_atomic_store(a.cnt_stream + (s * kLinShards + k % kLinShards) * kLinShardStride, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        for (int k = t; k < N; k += LNT) {
            int s = a.slot_upd + k;
            s = s >= kLinSlots ? s - kLinSlots : s;
            __hip_atomic_store(a.cnt_reduce + s, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    } else if (b < a.has_update + a.n_reduce) {
        // ---- reducers: set (rb / per_set) takes batches set, set + 2, ... ------------------------------------------------------
        const int rb = b - a.has_update, set = rb / per_set, ro = rb % per_set;
        const int tstep0 = a.step_dev[0];              // (the updater stores the counter at the very end of the launch)
        [[maybe_unused]] unsigned long long r0 = 0, r1 = 0, r2 = 0, racc_w = 0, racc_r = 0;
        int sl = a.slot_red + set;                            // the slot of batch n (set < kLinSlots, sets <= kLinSlots)
        sl = sl >= kLinSlots ? sl - kLinSlots : sl;
        for (int n = set; n < a.n_red; n += a.sets, sl = sl + a.sets >= kLinSlots ? sl + a.sets - kLinSlots : sl + a.sets) {
            LIN_NOWQ(r0);
            lin_wait_shards(a.cnt_stream + sl * kLinShards * kLinShardStride, (unsigned)a.ntiles, a.status, (2u << 28) | ((unsigned)n << 16));
            LIN_NOWQ(r1);
            // 32-output slices, two at a time where there are two (a 128-output form reading 16 bytes per lane with sc1 buffer loads
            // measured 8 % SLOWER per step)
            for (int sub = ro; sub < NO / 32; sub += 2 * per_set) {
                if (sub != ro) __syncthreads();                         // the previous slices' LDS sums have been read
                const float* pin = a.partial_base + (long long)sl * a.ntiles * NO;
                const unsigned epoch = (unsigned)(tstep0 + a.d_red + n + 1);          // the batch's Adam step: the tag of its exchange granules
                if (sub + per_set < NO / 32)
                    lin_reduce_pair(pin, a.M_base + (long long)sl * NO, a.ntiles, lin_smem, sub, sub + per_set, NO, a.comm, epoch, a.status);
                else lin_reduce<true>(pin, a.M_base + (long long)sl * NO, a.ntiles, lin_smem, sub, NO, &a.comm, epoch, a.status);
            }
            lin_wait_vmcnt<0>();                               // every storing wave drains its write-through stores ...
            __syncthreads();                                   // ... before the one lane that signals for the workgroup
            LIN_NOWQ(r2);
            racc_w += r1 - r0; racc_r += r2 - r1;
            if (rb == 5) { LIN_PUT(40, racc_w); LIN_PUT(41, racc_r); }
            if (rb == 5 && n < 3) { LIN_PUT(56 + 2 * n, r1); LIN_PUT(57 + 2 * n, r2); }
            if (t == 0) __hip_atomic_fetch_add(a.cnt_reduce + sl, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            { [[maybe_unused]] unsigned long long te = 0; LIN_NOW(te); LIN_PUTMAX(136 + n, te); }      // (64 .. 131: the updater's, up to kLinSlots batches)
        }
    } else {
        // ---- streamers: workgroup sid takes tiles sid, sid + S, ... of every batch, in batch order, through a ring of THREE LDS
        // slots.  Iteration i multiplies item i while the LDS-DMA pieces of item i + 2 are issued between its k-steps (the issue
        // cost hides behind the matrix pipe) and item i + 1 is in flight.  Per wave the memory operations retire in issue order
        //     ... P(i) | S(i - 2) | P(i + 1) | S(i - 1) | [iteration i:] P(i + 2) | S(i)        (P: pieces, S: the partial image's store)
        // so ONE counted wait at the top of iteration i -- all but P(i + 1) and S(i - 1) -- says that tile i has landed and that
        // this wave's share of image i - 2 has left; the barrier behind it makes both true for the workgroup, and one lane signals
        // image i - 2.  The batch pointers come in as kernel arguments and live in LDS.
        const int sid = b - a.has_update - a.n_reduce, S = a.n_stream;
        { [[maybe_unused]] unsigned long long te = 0; LIN_NOWQ(te); if (sid == 0) LIN_PUT(50, te); if (sid == S / 2) LIN_PUT(51, te); if (sid == S - 1) LIN_PUT(52, te); }
        const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
        const LinTile tl(a.D, a.L, a.T);
        const int stride = max(tl.bytes, lin_ring_scratch_bytes(NB));   // a slot doubles as the combine's cross-wave scratch
        const int v_off = 3 * stride, vr_off = v_off + 4 * a.T, c_off = vr_off + 4 * a.T;
        const float** tab = reinterpret_cast<const float**>(lin_smem + c_off + 16);            // [3][kLinMaxPersist]
        if constexpr (!GEN) {
            if (t < 3 * kLinMaxPersist) {
                const int which = t / kLinMaxPersist, n = t % kLinMaxPersist;
                tab[t] = n < a.n_str ? (which == 0 ? src.x : which == 1 ? src.z1 : src.z2)[n] : nullptr;
            }
        }
        [[maybe_unused]] float* const Amat = reinterpret_cast<float*>(lin_smem + c_off + 16);     // GEN: the dataset's mixing matrix (<= 16 x 16), where the other form keeps its pointer tables
        if constexpr (GEN) {
            if (src.kind == 0 && t < src.dd * src.did) Amat[t] = src.A[t];
        }
        const int valid_last = a.B - (a.ntiles - 1) * a.T;              // rows of a batch's last tile
        lin_write_vcol(reinterpret_cast<float*>(lin_smem + v_off), a.T, a.T, t);
        lin_write_vcol(reinterpret_cast<float*>(lin_smem + vr_off), a.T, valid_last, t);
        if (t == 0) { *reinterpret_cast<float*>(lin_smem + c_off) = 0.f; *reinterpret_cast<unsigned*>(lin_smem + c_off + 8) = 0u; }      // the zero word; the draw's ticket counter
        __syncthreads();
        const int per_batch = sid < a.ntiles ? (a.ntiles - sid + S - 1) / S : 0, items = a.n_str * per_batch;
        // Wave roles inside a streamer: waves 0 .. 3 (one per SIMD) multiply, waves 4 .. 7 load (LDS-DMA pieces of the tile two ahead,
        // or its Philox draw): with all 8 waves doing both, each wave's ~650 scalar / vector / LDS instructions per tile and its 54
        // MFMAs simply added up (streamers alone 4.7 us per tile; without the MFMAs 3.4, without the LDS-DMA 3.2, without both 2.1:
        // tools/lin_ablate.sh) -- a wave cannot issue anything else while it waits for the matrix pipe to take its next MFMA.
        const bool loader = wave >= kLinCW;
        const int lw = wave - kLinCW;                                                            // loader waves: 0 .. NLW - 1
        constexpr int NLW = LNW - kLinCW;
        auto share = [&](int n) { return lw < n ? (n - lw + NLW - 1) / NLW : 0; };
        const int npw = (GEN || !loader) ? 0 : share(tl.nz1) + share(tl.nx) + share(tl.np - tl.nz1 - tl.nx);  // this wave's pieces of a tile: its share of each tensor's
        const int sw = wave < (NO / 4 + 63) / 64 ? 1 : 0;                                        // does this wave store a share of an image?
        // item i = tile sid + (i % per_batch) S of batch i / per_batch, in slot i % 3: walked by cursors (a run-time integer division
        // costs ~40 instructions, and the loop wanted a dozen per tile).  n counts the launch's streamed batches (pointer tables, the
        // draw's step); bs is the batch's workspace slot (image, arrival counter), round the kLinSlots from the launch's first.
        struct Pos {
            int idx, n, r, slot, bs;
            __device__ __forceinline__ void advance(int per_batch) {
                ++idx; slot = slot == 2 ? 0 : slot + 1;
                if (++r == per_batch) { r = 0; ++n; bs = bs == kLinSlots - 1 ? 0 : bs + 1; }
            }
        };
        auto pos_tile = [&](const Pos& q) { return sid + q.r * S; };
        Pos p_cur{0, 0, 0, 0, a.slot_str}, p_load{0, 0, 0, 0, a.slot_str}, p_sig{0, 0, 0, 0, a.slot_str};      // the item being multiplied / the next to load or draw / the next to signal
        LinTileSrc nxt;                                       // the item whose pieces are being issued
        nxt.on = false;
        auto prepare = [&]() __attribute__((always_inline)) {             // the next item in order (p_load), which it advances
            if constexpr (!GEN) {
                nxt.on = false;
                if (p_load.idx < items) {
                    const int n = p_load.n;
                    nxt.prepare(a, tab[n], tab[kLinMaxPersist + n], tab[2 * kLinMaxPersist + n], pos_tile(p_load), lin_smem + p_load.slot * stride);
                }
                p_load.advance(per_batch);
            }
        };
        auto issue_pieces = [&]() __attribute__((always_inline)) {      // this wave's share of that item
            if constexpr (!GEN) { if (!(VAEK_LIN_ABL & 8) && nxt.on) nxt.issue_tile(tl, lw, NLW, lane); }
        };
        // GEN: the draw of item i in ROUNDS dealt to the GT = 256 threads of the loader waves.  A unit of work is a row of x or one
        // latent block (4 normals: block z = row * nzb + q holds columns 4 q .. of the row's [z1 | z2]): first the rows of x (thread =
        // row, ceil(T / GT) rounds), then rounds that give every thread TWO latent blocks (two independent Philox chains), then what
        // is left, one block per thread.  Rows past the batch end are written as zeros.  WHO draws: a unit of 64 draw threads of one
        // round goes to whichever wave takes the next ticket (an LDS counter) -- the loading waves from the barrier on, the multiplying
        // waves once their products are done: the draw is vector-ALU work (9 Philox blocks + Box-Muller per sample: 8.7 us per tile on
        // four waves), the products keep a wave's matrix pipe busy for 2.2 us of it.  What a unit writes depends on the unit alone.
        constexpr int GT = NLW * 64;
        [[maybe_unused]] const int gD = DT ? DT : a.D, gL = LT ? LT : a.L, nzb = (gL + gD + 3) / 4;
        [[maybe_unused]] const int nlat = a.T * nzb, xr = (a.T + GT - 1) / GT, npair = nlat / (2 * GT), rem = nlat - 2 * GT * npair;
        [[maybe_unused]] const int gen_rounds = xr + npair + (rem + GT - 1) / GT;
        [[maybe_unused]] const unsigned step0 = (unsigned)(a.step_dev[0] + a.d_str);     // the first streamed batch's (the updater, d_str batches behind, stores the counter at the very end of the launch)
        // (copies: read through `src` the generator's scalars are re-fetched from the kernel-argument segment inside the loops)
        [[maybe_unused]] int g_kind = 0, g_dd = 0, g_did = 0; [[maybe_unused]] float g_noise = 0.f; [[maybe_unused]] unsigned g_tag = 0;
        if constexpr (GEN) { g_kind = src.kind; g_dd = src.dd; g_did = src.did; g_noise = src.noise_std; g_tag = src.tag; }
        auto gen_round = [&](const Pos& q, int k, int gt) __attribute__((always_inline)) {       // round k of item q, as draw thread gt of GT
            if constexpr (GEN) {
                if (q.idx < items && k < gen_rounds) {
                    const uint2 key = make_uint2((unsigned)src.seed, (unsigned)(src.seed >> 32));
                    const long long row_lo = (long long)pos_tile(q) * a.T;
                    const unsigned step = step0 + (unsigned)q.n;
                    char* slot = lin_smem + q.slot * stride;
                    auto put = [&](int z, const float (&n4)[4]) __attribute__((always_inline)) {      // latent block z of the tile
                        const int r = z / nzb, q = z - r * nzb, c0 = 4 * q;
                        const bool live = row_lo + r < a.B;
                        const f32x4 v4 = live ? f32x4{n4[0], n4[1], n4[2], n4[3]} : f32x4{0.f, 0.f, 0.f, 0.f};
                        float* z1r = reinterpret_cast<float*>(slot) + r * gL;
                        float* z2r = reinterpret_cast<float*>(slot + tl.oZ2) + r * gD;
                        if (c0 + 3 < gL && gL % 4 == 0) *reinterpret_cast<f32x4*>(z1r + c0) = v4;
                        else if (c0 >= gL && (c0 - gL) + 3 < gD && gD % 4 == 0 && gL % 4 == 0) *reinterpret_cast<f32x4*>(z2r + (c0 - gL)) = v4;
                        else {
#pragma unroll
                            for (int c = 0; c < 4; ++c) {
                                if (c0 + c < gL) z1r[c0 + c] = v4[c];
                                else if (c0 + c < gL + gD) z2r[c0 + c - gL] = v4[c];
                            }
                        }
                    };
                    auto draw = [&](int z, float (&n4)[4]) __attribute__((always_inline)) {
                        const int r = z / nzb;
                        latent_block(src, step, src.row0 + row_lo + r, key, z - r * nzb, n4);
                    };
                    if (k >= xr && k < xr + npair) {
                        const int za = 2 * GT * (k - xr) + gt;
                        float na[4], nb[4];
                        draw(za, na); draw(za + GT, nb);
                        put(za, na); put(za + GT, nb);
                    } else if (k >= xr + npair) {
                        const int z = 2 * GT * npair + GT * (k - xr - npair) + gt;
                        if (z < nlat) {
                            float n4[4];
                            draw(z, n4);
                            put(z, n4);
                        }
                    } else {
                        const int row = gt + GT * k;
                        if (row < a.T) {
                            // the row of x (datasets.py:183-195 / :75-84), the arithmetic of rng_dev.h's dataset_cols4 step for step --
                            // with the mixing matrix read from LDS (through the scalar cache its loads cost 2.8 us per tile)
                            const long long lrow = row_lo + row, grow = src.row0 + lrow;
                            const bool live = lrow < a.B;
                            float nrm[16];
                            dataset_normals(src, step, grow, key, nrm);
                            float* xr_ = reinterpret_cast<float*>(slot + tl.oX) + row * gD;
                            float inv = 0.f;
                            if (g_kind == 2) {
                                float nsq = 0.f;
#pragma unroll
                                for (int d = 0; d < 16; ++d) if (d < g_dd) nsq = fmaf(nrm[d], nrm[d], nsq);
                                inv = 1.f / sqrtf(nsq);
                            }
                            for (int c0 = 0; c0 < gD; c0 += 4) {
                                float o[4] = {0.f, 0.f, 0.f, 0.f};
                                if (c0 < g_dd) {
#pragma unroll
                                    for (int c = 0; c < 4; ++c) {
                                        const int d = c0 + c;
                                        float v = 0.f;
                                        if (d < g_dd) {
                                            if (g_kind == 0) {
#pragma unroll
                                                for (int kk = 0; kk < 16; ++kk) if (kk < g_did) v = fmaf(Amat[d * g_did + kk], nrm[kk], v);
                                            } else {
#pragma unroll
                                                for (int kk = 0; kk < 16; ++kk) v = (kk == d) ? nrm[kk] : v;
                                                v *= inv;
                                            }
                                        }
                                        o[c] = v;
                                    }
                                }
                                if (g_kind == 0 && g_noise > 0.f) {      // noise normals: blocks (did+3)/4 .. of the same stream
                                    float n4[4];
                                    normals4(philox4x32_10(make_uint4((unsigned)grow, (unsigned)((g_did + 3) / 4 + c0 / 4), step, g_tag), key), n4);
#pragma unroll
                                    for (int c = 0; c < 4; ++c) o[c] = fmaf(g_noise, n4[c], o[c]);
                                }
                                const f32x4 v4 = live ? f32x4{o[0], o[1], o[2], o[3]} : f32x4{0.f, 0.f, 0.f, 0.f};
                                if (gD % 4 == 0) *reinterpret_cast<f32x4*>(xr_ + c0) = v4;
                                else {
#pragma unroll
                                    for (int c = 0; c < 4; ++c) if (c0 + c < gD) xr_[c0 + c] = v4[c];
                                }
                            }
                        }
                    }
                }
            }
        };
        [[maybe_unused]] unsigned* const ticket = reinterpret_cast<unsigned*>(lin_smem + c_off + 8);       // zeroed between two barriers before every use
        // every wave: units of the draw of q0 (and then of q1, nitems == 2) until the tickets run out
        auto gen_share = [&](const Pos& q0, const Pos& q1, int nitems) __attribute__((always_inline)) {
            if constexpr (GEN) {
                const unsigned units = (unsigned)gen_rounds * NLW, total = units * (unsigned)nitems;
#pragma unroll 1
                for (;;) {
                    unsigned u = 0;
                    if (lane == 0) u = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    u = (unsigned)__builtin_amdgcn_readfirstlane((int)u);
                    if (u >= total) break;
                    const bool second = u >= units;
                    const unsigned v = second ? u - units : u;
                    gen_round(second ? q1 : q0, (int)(v / NLW), (int)(v % NLW) * 64 + lane);
                }
            }
        };
        unsigned* const my_shard = a.cnt_stream + (b & (kLinShards - 1)) * kLinShardStride;
        auto signal = [&]() {                                 // the next image in order is out (ONE lane, behind every wave's drain + a barrier)
            if (t == 0) __hip_atomic_fetch_add(my_shard + p_sig.bs * kLinShards * kLinShardStride, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            p_sig.advance(per_batch);
        };
        if constexpr (GEN) {
            Pos q1 = p_load;
            q1.advance(per_batch);
            gen_share(p_load, q1, 2);                          // items 0 and 1: every wave draws
            p_load.advance(per_batch); p_load.advance(per_batch);
            lin_barrier();
            if (t == 0) *ticket = 0u;                          // (the loop's first barrier stands between this and the next ticket)
        } else if (loader) {
            prepare();
            issue_pieces();
            prepare();
            issue_pieces();
        }
        LinFeatMap<NB> fmap;                                  // this lane's operand addresses, but for the slot and the validity column
        fmap.init(a, tl, v_off, c_off, lane);
        [[maybe_unused]] unsigned long long s0 = 0, s1 = 0, s2 = 0, s3 = 0, s4 = 0, s5 = 0, s6 = 0, sacc_i = 0, sacc_l = 0, sacc_f = 0, sacc_m = 0, sacc_p = 0, sacc_b = 0;
        // ONE LOOP PER ROLE in the three-block kernels, the same barriers in both: the multiplying waves carry no piece cursors, no
        // LinTileSrc and no pointer tables through their loop, the loading waves no accumulators and no feature map, and neither
        // walks through the other's code as skipped branches (streamers alone 3.31 -> 3.20 us per step at the metric's shape:
        // profiles/lin_trim_roles.txt).  The four-block kernels keep one loop for both roles: their streamers are not the pace, and
        // the launch got SLOWER when they ran faster (profiles/lin_trim_bench.txt, M20).
        auto items_loop = [&](auto role) __attribute__((always_inline)) {
            constexpr int kRole = decltype(role)::value;          // 0 multiplying, 1 loading, 2 either (one loop for both)
            const bool is_loader = kRole == 2 ? loader : kRole == 1;
            for (int i = 0; i < items; ++i) {
                LIN_NOWQ(s0);
                lin_wait_vmcnt_upto((i + 1 < items ? npw : 0) + (i >= 1 ? sw : 0));       // tile i has landed, this wave's share of image i - 2 is out
                LIN_NOWQ(s1);
                lin_barrier();                                     // ... for every wave; and everybody is done with slot (i + 2) % 3 (the scratch of i - 1)
                LIN_NOWQ(s2);
                if (i >= 3) signal();                              // image i - 2 (image 0 left at the end of iteration 0)
                const int n = p_cur.n, tile = pos_tile(p_cur), slot_off = p_cur.slot * stride;
                char* slot = lin_smem + slot_off;
                const bool ragged = tile == a.ntiles - 1 && valid_last < a.T;
                if constexpr (!GEN) {
                    if (ragged) lin_fix_ragged(a, tl, tab[n], tab[kLinMaxPersist + n], tab[2 * kLinMaxPersist + n], tile, slot, t);
                }
                LIN_NOWQ(s3);
                f32x4 acc[NB * (NB + 1) / 2];
                if (!is_loader) {
                    int fb[NB];
                    fmap.at(slot_off, ragged ? vr_off - v_off : 0, fb);
                    lin_tile_products_at<NB, JT, kLinCW>(a, lin_smem, fb, fmap.fs, acc, lane, wave, [](int) {});
                }
                if constexpr (GEN) {
                    gen_share(p_load, p_load, 1);                  // item i + 2: the loading waves at once, the multiplying waves behind their products
                    p_load.advance(per_batch);
                } else if (is_loader && i > 0) {
                    // (iteration 0 issues the pieces of tile 2 only behind its early signal: the drain in front of that signal would
                    // otherwise wait for them to land)
                    prepare();
                    issue_pieces();
                }
                LIN_NOWQ(s5);
                float* const out = a.partial_base + ((long long)p_cur.bs * a.ntiles + tile) * NO;
                lin_barrier();                                     // every wave has read its last operand: the slot turns into scratch
                if constexpr (GEN) { if (t == 0) *ticket = 0u; }   // (nobody takes a ticket before the next iteration's first barrier)
                LIN_NOWQ(s6);
                lin_tile_combine<NB, true, kLinCW>(acc, slot, out, t, wave, lane);
                if (i == 0) {                                      // the launch's first image: out at once (pipeline fill), not two tiles later
                    lin_wait_vmcnt<0>();
                    lin_barrier();
                    signal();
                    if (sid == 0) { [[maybe_unused]] unsigned long long te = 0; LIN_NOWQ(te); LIN_PUT(53, te); }
                    if constexpr (!GEN) {
                        if (is_loader) {
                            prepare();
                            issue_pieces();
                        }
                    }
                }
                LIN_NOWQ(s4);
                if (i + 1 < items) { sacc_i += s1 - s0; sacc_l += s2 - s1; sacc_f += s3 - s2; sacc_m += s4 - s3; sacc_p += s5 - s3; sacc_b += s6 - s5; }
                if (sid == 7) { LIN_PUT(42, sacc_i); LIN_PUT(43, sacc_l); LIN_PUT(44, sacc_f); LIN_PUT(45, sacc_m); LIN_PUT(46, (unsigned long long)items); LIN_PUT(47, sacc_p); LIN_PUT(48, sacc_b); }
                p_cur.advance(per_batch);
            }
        };
        if constexpr (NB != 3) items_loop(std::integral_constant<int, 2>{});
        else if (loader) items_loop(std::integral_constant<int, 1>{});
        else items_loop(std::integral_constant<int, 0>{});
        lin_wait_vmcnt<0>();
        lin_barrier();
        if (items - 2 >= 1) signal();
        if (items - 1 >= 1) signal();
        { [[maybe_unused]] unsigned long long te = 0; LIN_NOWQ(te); LIN_PUTMAX(49, te); }
    }
}

typedef void (*LinPersistKernel)(const LinArgs, const LinPtrs);
typedef void (*LinPersistGenKernel)(const LinArgs, const BatchArgs);
// The four-block instantiations of the persistent form (linear_moments4.hip).  0: run-time shapes, 1: D = 20, L = 20.
LinPersistKernel lin_persist_four(int which);
LinPersistGenKernel lin_persist_four_gen(int which);

}  // namespace vaek
