// Shared internals of libuniver_hip.so (gfx950 only).  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <type_traits>
#include <utility>

#include "univer_hip.h"

// ---- launch reports: what the last accepted call of a kind chose, read back by the uocr_ctx_last_* getters.
// To add one: (1) an entry in this enum, (2) uocr_note(ctx, UOCR_REPORT_X, v0, v1, ...) at the end of the launcher, after
// its launches and never on an error path, (3) a getter next to the launcher that is one `return uocr_report_read(ctx,
// UOCR_REPORT_X, out0, out1, ...)` with the outs in the order of the noted values, (4) its declaration and comment in
// include/univer_hip.h, (5) its line in _PROTOS of hip/lib.py, (6) a Runtime.last_x in nn/gpu.py that returns
// self._report('uocr_ctx_last_x').  A new context reports all zeros.  (The two GEMM launchers of gemm_mfma.hip note just
// before their launch, not after it: a launch that fails there leaves the new report behind.  Not a pattern to copy.)
enum uocr_report_id {
    UOCR_REPORT_SPLIT,            // blocks and work items of the last launch with a run-time split
    UOCR_REPORT_GEMM,             // row tile, output-tile grid, slabs of the last MFMA GEMM
    UOCR_REPORT_GEMM_GROUP,       // problems / split problems of the last group flush
    UOCR_REPORT_PAIR,             // the form of the last Monochrome pair launch (kernel, g, mode, pf) and its geometry
                                  // (waves per block, grid x, grid y, rows per band)
    UOCR_REPORT_CONV,             // entry point and kernel family of the last accepted conv call
    UOCR_REPORT_LABEL,            // tile and launch count of the last labelling call
    UOCR_REPORT_LABEL_BATCH,      // tile, entries per launch and launch count of the last batched labelling call
    UOCR_REPORT_CHAR_LABEL,       // sizes and launch count of the last char-label call
    UOCR_REPORT_LINE_CROP,        // sizes and launch count of the last line-crop call
    UOCR_REPORT_ROTATE,           // sizes and launch count of the last rotation call
    UOCR_REPORT_ROTATION_SEARCH,  // rounds, paragraphs per launch and launch count of the last search
    UOCR_REPORT_PRED_TO_TEXT,     // sizes and launch count of the last pred-to-text call
    UOCR_REPORT_PACK_LINES,       // sizes and launch count of the last pack-lines or zero-gaps call
    UOCR_REPORT_PAGE_GEN,         // tile, pages per launch and launch count of the last page-layout or page-render call
    UOCR_REPORT_COUNT
};
constexpr int UOCR_REPORT_VALUES = 8;   // the most values of one report (pair); 64-bit for the item count of split

// Every field states its default here; uocr_ctx_create sets only what depends on its arguments, the environment or the device.
struct uocr_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool owns_stream = true;
    void* workspace = nullptr;
    size_t workspace_bytes = 0;
    const double* snap_src = nullptr;   // uocr_ctx_set_loss_snapshot: loss slots the fused optimizer kernels copy into ...
    int snap_count = 0;
    double* snap_ring = nullptr;        // ... row (counter++ % snap_ring_len) of this ring, or snap_src == null
    int snap_ring_len = 0;
    unsigned* snap_counter = nullptr;
    void* gemm_defer = nullptr;    // recorded weight-gradient GEMMs of an open deferred group (gemm_mfma.hip), or null
    void* finish_defer = nullptr;  // recorded finish kernels + their partial region (finish_group.hip), or null
    unsigned* sync = nullptr;      // arrival counters of the in-launch reductions, a word per user (uocr_sync_word): zero between launches
    int cu_count = 256;            // (the device's, once uocr_ctx_create could ask it)
    int opt_mfma = 1;        // 0 = never, 1 = auto (default), 2 = whenever eligible (tests)
    int opt_fast = 1;        // 0 = generic kernels only, 1 = shape-specialised fast paths (default)
    int opt_tiled = 1;       // 0 = no LDS-tiled conv kernels, 1 = use them where instantiated (default)
    int opt_split = 1024;    // MFMA GEMMs split their depth until there are about this many blocks (0 = never)
    int opt_split_min = 3;   // ... but only when that takes at least this many slabs (a 2-way split rarely pays its reduce)
    int opt_xcd = 1;         // 1 = MFMA GEMM blocks are renumbered so that neighbours share an XCD (L2)
    int opt_bm = 0;          // 0 = choose the MFMA GEMM row tile automatically, 64 / 128 = force it (experiments)
    int opt_h16 = 1;         // 1 = binary16-MFMA kernels for the small-channel convs in UOCR_F16 mode (default)
    int opt_t32 = 2;         // float32 vertical-Toeplitz MFMA kernels for the small-channel convs: bit 0 forward, bit 1 backward-data
                             // (2 was measured: only the 4-channel backward-data beats its vector kernel in the step; conv_t32.hip,
                             // conv_t32w.hip: bits 64 / 128 = the float32-MFMA weight gradients, 37.0 -> 36.1 k images/s with both)
    int opt_pair_band = 0;   // rows per band of the strip kernels (0 = about one block per CU)
    int opt_pair_pf = -1;    // row prefetch of the pair forward kernels (-1 auto / 0 / 1 / 2, see conv_pair_strip.hip)
                             // (auto: float32 one step ahead (49.5 us; 50.8 pinned in the loop, 51.8 three ahead), binary16 three (72.1;
                             // 73.8 / 75.5))
    int opt_h3 = 0;          // 1 = the float32 Line output conv forward on error-compensated binary16 MFMAs (conv_h3.hip; experiment)
    int opt_group_blocks = 0; // blocks of a deferred weight-gradient group (0 = four per CU)
    int opt_wgrad_bands = 0;  // row bands per tap / channel group of the direct weight-gradient kernels (0 = by accumulator count)
    int opt_pair_g = 4;      // groups of 16 columns per wave of the strip kernels: 4 (8 waves per block) or 2 (16 waves)
    int opt_act_dispatch = 1; // 1 = activation / mask kinds the nets use are compile-time tags of the kernel (default), 0 = the run-time switch
    int opt_max_blocks = 0;  // k > 0 lowers every run-time block budget to k (tests: several tiles per block at small shapes)
    long long report[UOCR_REPORT_COUNT][UOCR_REPORT_VALUES] = {};   // uocr_note writes, uocr_report_read reads
    char err[512] = {};
};

// bits of the "t32" option whose kernels this library contains (conv_t32.hip, conv_t32w.hip)
#ifdef UOCR_EXPERIMENTS
constexpr int UOCR_T32_BUILT = 255;
#else
constexpr int UOCR_T32_BUILT = 2;
#endif

#define UOCR_FAIL(ctx, code, ...)                                   \
    do {                                                            \
        if (ctx) snprintf((ctx)->err, sizeof((ctx)->err), __VA_ARGS__); \
        return (code);                                              \
    } while (0)

#define UOCR_HIP(ctx, call)                                                              \
    do {                                                                                 \
        hipError_t e_ = (call);                                                          \
        if (e_ != hipSuccess)                                                            \
            UOCR_FAIL(ctx, UOCR_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                      __FILE__, __LINE__);                                               \
    } while (0)

#define UOCR_LAUNCH_CHECK(ctx)                                                           \
    do {                                                                                 \
        hipError_t e_ = hipGetLastError();                                               \
        if (e_ != hipSuccess)                                                            \
            UOCR_FAIL(ctx, UOCR_ERR_HIP, "kernel launch failed: %s (%s:%d)", hipGetErrorString(e_), \
                      __FILE__, __LINE__);                                               \
    } while (0)

#define UOCR_REQUIRE(ctx, cond)                                                          \
    do {                                                                                 \
        if (!(cond)) UOCR_FAIL(ctx, UOCR_ERR_ARG, "bad argument: %s (%s:%d)", #cond, __FILE__, __LINE__); \
    } while (0)

#define UOCR_CHECK_CTX(ctx) \
    do {                    \
        if (!(ctx)) return UOCR_ERR_ARG; \
    } while (0)

// the one writer and the one reader of ctx->report (the recipe is above uocr_report_id)
template <typename... V>
static inline void uocr_note(uocr_ctx* ctx, uocr_report_id id, V... v) {
    static_assert(sizeof...(V) >= 1 && sizeof...(V) <= UOCR_REPORT_VALUES, "a report holds 1 to UOCR_REPORT_VALUES values");
    long long* slot = ctx->report[id];
    ((*slot++ = (long long)v), ...);
}
// a null out pointer is an error before anything is written; every value is cast to the type its pointer points to
template <typename... T>
static inline int uocr_report_read(uocr_ctx* ctx, uocr_report_id id, T*... out) {
    static_assert(sizeof...(T) >= 1 && sizeof...(T) <= UOCR_REPORT_VALUES, "a report holds 1 to UOCR_REPORT_VALUES values");
    UOCR_CHECK_CTX(ctx);
    if (!(out && ...)) UOCR_FAIL(ctx, UOCR_ERR_ARG, "bad argument: null out pointer of launch report %d", (int)id);
    const long long* slot = ctx->report[id];
    ((*out = (T)*slot++), ...);
    return UOCR_OK;
}

// dtype dispatch: BODY sees the type alias T
#define UOCR_DISPATCH(ctx, dtype, ...)                                   \
    do {                                                                 \
        if ((dtype) == UOCR_F32) { using T = float; __VA_ARGS__; }       \
        else if ((dtype) == UOCR_F64) { using T = double; __VA_ARGS__; } \
        else UOCR_FAIL(ctx, UOCR_ERR_DTYPE, "unknown dtype %d", (int)(dtype)); \
    } while (0)

// activation-tensor dispatch: BODY sees TS = the storage type in HBM and T = the type to compute in
// (UOCR_F16: binary16 storage, float32 arithmetic; the gradient-scale bits of dtype are ignored here)
#define UOCR_DISPATCH_ACT(ctx, dtype, ...)                                                        \
    do {                                                                                          \
        const int base_ = UOCR_DTYPE_BASE(dtype);                                                 \
        if (base_ == UOCR_F32) { using TS = float; using T = float; __VA_ARGS__; }                \
        else if (base_ == UOCR_F64) { using TS = double; using T = double; __VA_ARGS__; }         \
        else if (base_ == UOCR_F16) { using TS = _Float16; using T = float; __VA_ARGS__; }        \
        else UOCR_FAIL(ctx, UOCR_ERR_DTYPE, "unknown dtype %d", (int)(dtype));                    \
    } while (0)

// storage-type dispatch for kernels that convert every element on load / store themselves: BODY sees T
#define UOCR_DISPATCH_STORAGE(ctx, dtype, ...)                                                    \
    do {                                                                                          \
        const int base_ = UOCR_DTYPE_BASE(dtype);                                                 \
        if (base_ == UOCR_F32) { using T = float; __VA_ARGS__; }                                  \
        else if (base_ == UOCR_F64) { using T = double; __VA_ARGS__; }                            \
        else if (base_ == UOCR_F16) { using T = _Float16; __VA_ARGS__; }                          \
        else UOCR_FAIL(ctx, UOCR_ERR_DTYPE, "unknown dtype %d", (int)(dtype));                    \
    } while (0)

// 2^k of UOCR_F16_SCALED(k): the loss kernels multiply their gradient by it, the bwd_weight kernels divide
// dw / db by it (1 for the other dtypes)
static inline double uocr_grad_scale(int dtype) {
    return UOCR_DTYPE_BASE(dtype) == UOCR_F16 ? (double)(1u << (UOCR_DTYPE_GRAD_SCALE_LOG2(dtype) & 31)) : 1.0;
}
static inline double uocr_grad_unscale(int dtype) { return 1.0 / uocr_grad_scale(dtype); }

static inline int uocr_need_workspace(uocr_ctx* ctx, size_t bytes) {
    if (bytes > ctx->workspace_bytes)
        UOCR_FAIL(ctx, UOCR_ERR_WORKSPACE, "workspace too small: need %zu bytes, have %zu", bytes,
                  ctx->workspace_bytes);
    return UOCR_OK;
}

static inline unsigned uocr_blocks_for(size_t items, unsigned per_block, unsigned cap) {
    size_t b = (items + per_block - 1) / per_block;
    if (b < 1) b = 1;
    if (b > cap) b = cap;
    return (unsigned)b;
}

// a block budget of a launch that sizes its work at run time, lowered to the "max_blocks" option when that is set and
// smaller (never raised: some partial buffers are sized by the budget); the launch then reports its split
static inline long uocr_budget(const uocr_ctx* ctx, long budget) {
    return ctx->opt_max_blocks > 0 && ctx->opt_max_blocks < budget ? ctx->opt_max_blocks : budget;
}
static inline void uocr_note_split(uocr_ctx* ctx, long long blocks, long long items) {
    uocr_note(ctx, UOCR_REPORT_SPLIT, blocks, items);
}

// blocks of `kernel` (`threads` threads, no dynamic LDS) that one CU holds, asked once per `cache` (the caller's static
// int, 0 = not asked yet).  A failed query is an error, never "one block": a persistent kernel sized that way would
// quietly run several times slower.
template <typename K>
static inline int uocr_resident_blocks(uocr_ctx* ctx, K kernel, int threads, int* cache, int* out) {
    if (*cache == 0) {
        int nb = 0;
        UOCR_HIP(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, threads, 0));
        *cache = nb > 0 ? nb : 1;
    }
    *out = *cache;
    return UOCR_OK;
}
// grid of a persistent 256-thread kernel whose blocks walk t = blockIdx.x, += gridDim.x over ntiles tiles: one block per
// tile up to the budgeted cu_count * resident blocks * slots_per_resident; reports the split
template <typename K>
static inline int uocr_persistent_grid(uocr_ctx* ctx, K kernel, long ntiles, int slots_per_resident, int* cache,
                                       int* grid) {
    UOCR_REQUIRE(ctx, ntiles < (1l << 31));
    int resident = 0;
    const int rc = uocr_resident_blocks(ctx, kernel, 256, cache, &resident);
    if (rc != UOCR_OK) return rc;
    const long cap = uocr_budget(ctx, (long)ctx->cu_count * resident * slots_per_resident);
    *grid = (int)(ntiles < cap ? ntiles : cap);
    uocr_note_split(ctx, *grid, ntiles);
    return UOCR_OK;
}
// tiles of one column strip per block, the fewest with which tiles_x * ceil(tiles_y / per_block) * n blocks fit the budget
static inline int uocr_tiles_per_block(int tiles_x, int tiles_y, int n, long budget) {
    int per_block = 1;
    while (per_block < tiles_y && (size_t)tiles_x * ((tiles_y + per_block - 1) / per_block) * n > (size_t)budget) ++per_block;
    return per_block;
}

// what a pair launch chose (uocr_ctx_last_pair; kernel 1-5 as in univer_hip.h), noted once the launch was accepted
static inline void uocr_note_pair(uocr_ctx* ctx, int kernel, int g, int mode, int pf, int nw, int blocks_x, int bands,
                                  int band_h) {
    uocr_note(ctx, UOCR_REPORT_PAIR, kernel, g, mode, pf, nw, blocks_x, bands, band_h);
}

// which kernel family took a uocr_conv2d_* call (uocr_ctx_last_conv; entry 0 fwd / 1 bwd_data / 2 bwd_weight, kernel =
// UOCR_CONV_* of univer_hip.h), noted once the call was accepted: uocr_noted_conv passes a launcher's code through
static inline void uocr_note_conv(uocr_ctx* ctx, int entry, int kernel) {
    uocr_note(ctx, UOCR_REPORT_CONV, entry, kernel);
}
static inline int uocr_noted_conv(uocr_ctx* ctx, int entry, int kernel, int rc) {
    if (rc == UOCR_OK) uocr_note_conv(ctx, entry, kernel);
    return rc;
}

// grid cap for grid-stride HBM-bound kernels: 256 CUs x 8 blocks of 256 threads
constexpr unsigned UOCR_MAX_GRID = 2048;
constexpr int UOCR_WAVE = 64;

template <typename T>
__device__ __forceinline__ T wave_reduce_sum(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

template <typename T>
__device__ __forceinline__ T wave_reduce_max(T v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        T o = __shfl_down(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}

// block-wide sum of doubles for blocks of up to 1024 threads; result valid in thread 0 (NT: the block size where the caller
// knows it at compile time, 0 = ask blockDim)
template <int NT = 0>
__device__ __forceinline__ double block_reduce_sum(double v, double* smem /* >= 16 doubles */) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    v = wave_reduce_sum(v);
    __syncthreads();
    if (lane == 0) smem[wid] = v;
    __syncthreads();
    const int nw = NT ? (NT + 63) >> 6 : (blockDim.x + 63) >> 6;
    v = (threadIdx.x < (unsigned)nw) ? smem[threadIdx.x] : 0.0;
    if (wid == 0) v = wave_reduce_sum(v);
    return v;
}

// block-wide maximum of doubles (NaN never wins), same shape as block_reduce_sum; result valid in thread 0
template <int NT = 0>
__device__ __forceinline__ double block_reduce_max(double v, double* smem /* >= 16 doubles */) {
    v = wave_reduce_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) smem[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int nw = NT ? (NT + 63) >> 6 : (blockDim.x + 63) >> 6;
        for (int k = 1; k < nw; ++k) v = smem[k] > v ? smem[k] : v;
    }
    return v;
}

// ---- in-launch reductions: the last block to arrive folds what every block of the launch published
// Users: softmax_ce_kernel and sigmoid_ce_kernel (loss.hip: the loss, one sum), opt_fused_kernel (elementwise.hip: the four
// regulariser sums of the fused optimizer tail), label_stats (label.hip: sum and max of the image for the threshold).
// The protocol, stated once.  Blocks hand small float64 partials to each other INSIDE a launch.  gfx950 has one L2 per XCD
// and they are not coherent with each other, so every handed-off word is written by a relaxed agent-scope atomic store
// (write-through, sc1), drained (s_waitcnt vmcnt(0)) before the writer's arrival is counted by a relaxed agent-scope
// fetch-add, and read by relaxed agent-scope atomic loads (sc1: past this CU's L1 and this XCD's L2 copy); no fences.
// Nobody waits for another block.  Each user has its own counter word in ctx->sync (uocr_sync_word); a counter is zero
// between launches and is put back to zero by the block that drew the last ticket.
enum uocr_sync_word {
    UOCR_SYNC_SOFTMAX_CE = 1,   // (word 0 is not in use; the indices are the ones the launches have always counted in)
    UOCR_SYNC_SIGMOID_CE,
    UOCR_SYNC_OPT_TAIL,
    UOCR_SYNC_LABEL_STATS,
    UOCR_SYNC_WORDS             // words of ctx->sync
};
__device__ __forceinline__ void pub_store(double* p, double v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double pub_load(const double* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned sync_arrive(unsigned* c) {            // the payload stores of this thread's wave are drained first
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    return __hip_atomic_fetch_add(c, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void sync_clear(unsigned* c) {
    __hip_atomic_store(c, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// what one reduced quantity (a slot) is folded with: the order of the folds is fixed, so the bits are the same run to run
struct FoldSum {
    static __device__ __forceinline__ double identity() { return 0.0; }
    static __device__ __forceinline__ double fold(double acc, double v) { return acc + v; }
    template <int B>
    static __device__ __forceinline__ double block(double v, double* smem) { return block_reduce_sum<B>(v, smem); }
};
struct FoldMax {
    static __device__ __forceinline__ double identity() { return -INFINITY; }
    static __device__ __forceinline__ double fold(double acc, double v) { return v > acc ? v : acc; }
    template <int B>
    static __device__ __forceinline__ double block(double v, double* smem) { return block_reduce_max<B>(v, smem); }
};
// Every thread of every block of the launch calls this once (it contains barriers), with the block's own value of each slot
// in v[] of thread 0.  Returns false in all blocks but the one that drew the last ticket; there it returns true and leaves
// the launch-wide value of each slot in v[] of thread 0, for the caller to scale and store.  Thread t folds rows t, t + B,
// t + 2 B, ... of `partial` in that order (B = the block size of the launch), then the block tree of the slot's op.
// Two things are structure here, not a convention of the callers:
//  - thread 0 alone publishes all K words, drains them (sync_arrive) and takes the ticket: publisher and ticket-taker
//    are one lane of one wave, whatever K is;
//  - the K words of a thread's first TRIPS rows are all requested before the first one is waited for (an agent-scope load is
//    a trip to the memory side, and with a branch around each load hipcc waits for each: K x TRIPS trips in a row).  So a
//    row past the last block is read at a clamped address and replaced by the identity afterwards, no branch; rows past
//    TRIPS * B are walked K loads at a time.
template <int B, int TRIPS, class... Op, size_t... S /* 0 .. K-1: slot S is folded with the S-th Op */>
__device__ __forceinline__ bool last_block_fold_slots(std::index_sequence<S...>, unsigned* counter, double* partial,
                                                      double (&v)[sizeof...(Op)], double* smem) {
    constexpr int K = sizeof...(Op);
    static_assert(TRIPS >= 1 && K >= 1 && K * TRIPS <= 32, "a thread keeps K * TRIPS loads of two registers each in flight");
    if (threadIdx.x == 0) {
#pragma unroll
        for (int s = 0; s < K; ++s) pub_store(partial + (size_t)blockIdx.x * K + s, v[s]);
        smem[16] = sync_arrive(counter) == gridDim.x - 1 ? 1.0 : 0.0;
    }
    __syncthreads();
    if (smem[16] == 0.0) return false;                 // block-uniform
    const int count = (int)gridDim.x;
    double t[TRIPS][K];
#pragma unroll
    for (int k = 0; k < TRIPS; ++k)
#pragma unroll
        for (int s = 0; s < K; ++s) t[k][s] = pub_load(partial + (size_t)min((int)threadIdx.x + k * B, count - 1) * K + s);
    double acc[K] = {Op::identity()...};
#pragma unroll
    for (int k = 0; k < TRIPS; ++k) {
        const bool live = (int)threadIdx.x + k * B < count;
        ((acc[S] = Op::fold(acc[S], live ? t[k][S] : Op::identity())), ...);
    }
    for (int i = (int)threadIdx.x + TRIPS * B; i < count; i += B) {
        double row[K];
#pragma unroll
        for (int s = 0; s < K; ++s) row[s] = pub_load(partial + (size_t)i * K + s);
        ((acc[S] = Op::fold(acc[S], row[S])), ...);
    }
    ((v[S] = Op::template block<B>(acc[S], smem)), ...);
    if (threadIdx.x == 0) sync_clear(counter);
    return true;
}
template <int B, int TRIPS, class... Op>
__device__ __forceinline__ bool last_block_fold(unsigned* counter, double* partial /* [gridDim.x][K] */,
                                                double (&v)[sizeof...(Op)], double* smem /* >= 17 doubles */) {
    return last_block_fold_slots<B, TRIPS, Op...>(std::index_sequence_for<Op...>{}, counter, partial, v, smem);
}

// ---- activation-tensor element access ---------------------------------------------------------------------
// TA = float (UOCR_F32) or _Float16 (UOCR_F16: binary16 in HBM, float32 in registers).  1 / 2 / 4 consecutive
// elements per call as ONE memory instruction (4 / 8 / 16 bytes of float, 2 / 4 / 8 bytes of binary16).
using uocr_h2 = __attribute__((ext_vector_type(2))) _Float16;
using uocr_h4 = __attribute__((ext_vector_type(4))) _Float16;

__device__ __forceinline__ float ld1(const float* p) { return *p; }
__device__ __forceinline__ float ld1(const _Float16* p) { return (float)*p; }
__device__ __forceinline__ float2 ld2(const float* p) { return *reinterpret_cast<const float2*>(p); }
__device__ __forceinline__ float2 ld2(const _Float16* p) {
    const uocr_h2 v = *reinterpret_cast<const uocr_h2*>(p);
    return make_float2((float)v.x, (float)v.y);
}
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 ld4(const _Float16* p) {
    const uocr_h4 v = *reinterpret_cast<const uocr_h4*>(p);
    return make_float4((float)v.x, (float)v.y, (float)v.z, (float)v.w);
}
__device__ __forceinline__ void st1(float* p, float v) { *p = v; }
__device__ __forceinline__ void st1(_Float16* p, float v) { *p = (_Float16)v; }
__device__ __forceinline__ void st2(float* p, float2 v) { *reinterpret_cast<float2*>(p) = v; }
__device__ __forceinline__ void st2(_Float16* p, float2 v) {
    uocr_h2 h;
    h.x = (_Float16)v.x;
    h.y = (_Float16)v.y;
    *reinterpret_cast<uocr_h2*>(p) = h;
}
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ void st4(_Float16* p, float4 v) {
    uocr_h4 h;
    h.x = (_Float16)v.x;
    h.y = (_Float16)v.y;
    h.z = (_Float16)v.z;
    h.w = (_Float16)v.w;
    *reinterpret_cast<uocr_h4*>(p) = h;
}

// float32 / binary16 activation kernels: BODY sees TA (the float64 mode has its own generic kernels)
#define UOCR_DISPATCH_TA(ctx, dtype, ...)                                                          \
    do {                                                                                           \
        const int base_ = UOCR_DTYPE_BASE(dtype);                                                  \
        if (base_ == UOCR_F32) { using TA = float; __VA_ARGS__; }                                  \
        else if (base_ == UOCR_F16) { using TA = _Float16; __VA_ARGS__; }                          \
        else UOCR_FAIL(ctx, UOCR_ERR_DTYPE, "dtype %d: this kernel exists for float32 / float16 only", (int)(dtype)); \
    } while (0)

// alignment an activation pointer needs for the widest (4-element) access of the dtype
static inline bool uocr_aligned_act(const void* p, int dtype) {
    return (reinterpret_cast<uintptr_t>(p) & (UOCR_DTYPE_BASE(dtype) == UOCR_F16 ? 7u : 15u)) == 0;
}
static inline bool uocr_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// act(v) as the float32 epilogues compute it: the products of the reference's masks, 1 / (1 + expf(-v))
__device__ __forceinline__ float act_apply(float v, int act, float alpha) {
    switch (act) {
        case UOCR_ACT_RELU: return v * (v >= 0.f ? 1.f : 0.f);
        case UOCR_ACT_LEAKY: return v * ((v >= 0.f ? 1.f : 0.f) + alpha * (v < 0.f ? 1.f : 0.f));
        case UOCR_ACT_SIGMOID: return 1.f / (1.f + expf(-v));
        default: return v;
    }
}

// d act(x) / dx expressed through the activation OUTPUT y (leaky: alpha > 0 so sign(y) == sign(x))
template <typename T>
__device__ __forceinline__ T act_grad_from_output(T y, int act, T alpha) {
    if (act == UOCR_ACT_LEAKY) return y >= T(0) ? T(1) : alpha;
    if (act == UOCR_ACT_SIGMOID) return y * (T(1) - y);
    return T(1);
}

// ---- epilogue kinds at compile time
// A kernel that applies act(v) to its results or multiplies them by act'(y) takes the two kinds as the template tags
// ActKinds<ACT, MASK>.  UOCR_ACT_DYN in a place keeps the run-time switch on the kernel argument: the same template, one
// body, and what every pair the nets never use runs.  act_kind<KIND>(argument) is the kind a kernel works with: a
// constant unless the tag is dynamic, so the switches of act_apply / act_grad_from_output fold away.
constexpr int UOCR_ACT_DYN = -1;
template <int ACT, int MASK>
struct ActKinds {
    static constexpr int act = ACT, mask = MASK;
    static constexpr bool dynamic = ACT == UOCR_ACT_DYN;
};
// (a launcher keeps the tags only for the instantiations where they were measured to pay)
template <bool KEEP, class K>
using ActKindsIf = std::conditional_t<KEEP, K, ActKinds<UOCR_ACT_DYN, UOCR_ACT_DYN>>;
template <int KIND>
__host__ __device__ __forceinline__ int act_kind(int argument) {
    return KIND == UOCR_ACT_DYN ? argument : KIND;
}
// Calls f(ActKinds<..>{}) with the tags of (act, mask_act) where the four nets use that pair, with the dynamic tags for
// every other pair and when the "act_dispatch" option is 0.  SIDE 0: forward epilogues (no mask; none / LeakyReLU /
// Sigmoid), SIDE 1: masked backward-data (no activation; no mask / LeakyReLU').
template <int SIDE, class F>
static inline int uocr_act_tags(const uocr_ctx* ctx, int act, int mask_act, F&& f) {
    if (ctx->opt_act_dispatch) {
        if constexpr (SIDE == 0) {
            if (mask_act == UOCR_ACT_NONE && act == UOCR_ACT_NONE) return f(ActKinds<UOCR_ACT_NONE, UOCR_ACT_NONE>{});
            if (mask_act == UOCR_ACT_NONE && act == UOCR_ACT_LEAKY) return f(ActKinds<UOCR_ACT_LEAKY, UOCR_ACT_NONE>{});
            if (mask_act == UOCR_ACT_NONE && act == UOCR_ACT_SIGMOID) return f(ActKinds<UOCR_ACT_SIGMOID, UOCR_ACT_NONE>{});
        } else {
            if (act == UOCR_ACT_NONE && mask_act == UOCR_ACT_NONE) return f(ActKinds<UOCR_ACT_NONE, UOCR_ACT_NONE>{});
            if (act == UOCR_ACT_NONE && mask_act == UOCR_ACT_LEAKY) return f(ActKinds<UOCR_ACT_NONE, UOCR_ACT_LEAKY>{});
        }
    }
    return f(ActKinds<UOCR_ACT_DYN, UOCR_ACT_DYN>{});
}

// A tile staging loop `for (i = tid; i < COUNT; i += NT) lds[i] = in_image(i) ? load(i) : fill` compiles to ONE load, a wait
// and a store per trip: COUNT / NT global round trips in a row in front of every tile (ten for the dy tile of the upsample +
// conv backward-data kernels).  Here a thread issues up to BATCH loads (clamped addresses, no branch) before it waits for the
// first one; `addr(i, inside)` gives element i's clamped source pointer and whether it lies inside the image, `put(i, v,
// inside)` stores it (or the fill value).
template <int COUNT, int NT, int BATCH, typename V, typename Addr, typename Put>
__device__ __forceinline__ void stage_batched(int tid, Addr addr, Put put) {
    constexpr int K = (COUNT + NT - 1) / NT;
#pragma unroll
    for (int k0 = 0; k0 < K; k0 += BATCH) {
        V v[BATCH];
        bool in[BATCH];
#pragma unroll
        for (int k = 0; k < BATCH; ++k)
            if (k0 + k < K) v[k] = *addr(min(tid + NT * (k0 + k), COUNT - 1), in[k]);
#pragma unroll
        for (int k = 0; k < BATCH; ++k)
            if (k0 + k < K) {
                const int i = tid + NT * (k0 + k);
                if (i < COUNT) put(i, v[k], in[k]);
            }
    }
}

// Tile coordinates of a persistent block that walks t = blockIdx.x, += gridDim.x over tiles_x * tiles_y * images tiles:
// the three integer divisions (no hardware divide: ~20 dependent instructions each, in front of the tile's first load)
// are made once, for the first tile and for the stride; every further tile is three scalar adds with carries.
struct TileWalk {
    int strip, trow, img;
    int qx, qy, qz;
    __device__ __forceinline__ TileWalk(int first, int step, int tiles_x, int tiles_y) {
        strip = first % tiles_x;
        int r = first / tiles_x;
        trow = r % tiles_y;
        img = r / tiles_y;
        qx = step % tiles_x;
        r = step / tiles_x;
        qy = r % tiles_y;
        qz = r / tiles_y;
    }
    __device__ __forceinline__ void next(int tiles_x, int tiles_y) {
        strip += qx;
        int carry = strip >= tiles_x;
        strip -= carry ? tiles_x : 0;
        trow += qy + carry;
        carry = trow >= tiles_y;
        trow -= carry ? tiles_y : 0;
        img += qz + carry;
    }
};

// out = (accumulate ? out : 0) + scale * sum(partial[0..count)), one block, deterministic order
int uocr_finish_sum(uocr_ctx* ctx, const double* partial, int count, double scale, double* out, int accumulate);
