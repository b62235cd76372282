// Char labels: the device form of the reference's CharLabel stage (interpreter/interpreter.py:547-571 LabelChar._func1,
// driven by my_model/model.py:614-623).  Per line x (1, H, W, C) with channels bit_0 .. bit_{B-1} and then whatever else
// the `char` layer tag carries (letter_spacing, my_model/constants.py:22-25):
//   threshold  t = 0.5 * (mean + max) over all H * W * C elements; bit i of a pixel is set when x[y, x, i] > t
//   decode     code = sum bit_i 2^i; code < n_chars is that class, every other code is the ONE candidate "unknown"
//   vote       per column the most frequent candidate of its H pixels; on a tie the one that occurs first from the top
//   write      labels (W, n_chars): one-hot at the winner, all zeros where "unknown" won; ids (W): the class or -1
//
// All lines of a call travel together, CL_LINES per launch pair, their pointers and sizes in a by-value kernel argument
// (no device allocation, no copy, no host synchronisation: asynchronous and capturable).  Launches per CL_LINES lines:
//   1. char_label_stats  one block per CL_CHUNK elements of a line (a line is one flat contiguous range: 16-byte loads
//                        between a scalar head and tail, C = 9 gives no per-pixel alignment); float64 sum and max of
//                        the chunk go to the ctx workspace
//   2. char_label_vote   one block per CL_COLS columns of a line.  It adds its line's partials itself, in a fixed order
//                        (every block of a line gets the same bits; nobody waits for anybody inside a launch), reads
//                        its tile row by row -- a row of the tile is one contiguous span of cols * C elements -- and
//                        keeps one BIT per element in LDS (a wave's ballot is 64 consecutive elements), decodes to one
//                        byte per pixel, votes per column by a direct scan and writes its cols x n_chars block of the
//                        labels, zeros and ones together, as 16-byte stores
// The tensor crosses HBM twice.  No atomics: results are bit-identical run to run.
#include "entry_batch.h"

namespace {

constexpr int CL_NT = 256;          // threads per block of both kernels
constexpr int CL_LINES = 64;        // lines per launch pair (the descriptor is a kernel argument: 4 KB at most)
constexpr int CL_CHUNK = 8192;      // elements per block of char_label_stats
constexpr int CL_COLS = 32;         // columns per block of char_label_vote
constexpr int CL_SUB = CL_NT / CL_COLS;   // lanes that share a column's vote
constexpr int CL_MAX_H = 256, CL_MAX_C = 16;
constexpr int CL_BATCH = 8;         // loads a thread of char_label_vote has in flight
constexpr int CL_STAGE_WORDS = CL_MAX_H * CL_COLS * CL_MAX_C / 64;   // one bit per element of the largest tile

struct CLLine {
    const void* x;
    void* labels;
    int* ids;
    int h, w;
};
struct CLBatch {
    CLLine line[CL_LINES];
    int stat_first[CL_LINES + 1];   // first block of line i in the statistics grid = first partial of line i
    int tile_first[CL_LINES + 1];   // first block of line i in the vote grid
    int n, c, bits, n_chars;
};
static_assert(sizeof(CLBatch) <= 4096, "the descriptor travels as a kernel argument");

// block-wide max for CL_NT threads; valid in thread 0.  Contains barriers.
__device__ __forceinline__ double cl_block_max(double mx, double* smax /* >= CL_NT / 64 */) {
    mx = wave_reduce_max(mx);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) smax[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 1; k < CL_NT / 64; ++k) mx = smax[k] > mx ? smax[k] : mx;
    return mx;
}

// ---- 1. sum and max of every chunk ----------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(CL_NT) void char_label_stats(const CLBatch b, double* __restrict__ partial) {
    __shared__ double smem[17];
    __shared__ double smax[CL_NT / 64];
    using V = typename EBVec<T>::type;
    constexpr int VEC = EBVec<T>::N;
    const int tid = threadIdx.x;
    const int line = eb_entry_of(b.stat_first, b.n, blockIdx.x);
    const int chunk = blockIdx.x - b.stat_first[line];
    const size_t count = (size_t)b.line[line].h * b.line[line].w * b.c;
    const size_t first = (size_t)chunk * CL_CHUNK;
    const int n = (int)(count - first < (size_t)CL_CHUNK ? count - first : (size_t)CL_CHUNK);
    const T* p = (const T*)b.line[line].x + first;
    const auto [head, nvec, tail] = eb_split(p, n);
    double mx = -INFINITY, sum = 0.0;
    if (tid < head) {
        const double v = (double)p[tid];
        sum += v;
        mx = v > mx ? v : mx;
    }
    const V* pv = reinterpret_cast<const V*>(p + head);
#pragma unroll 4
    for (int i = tid; i < nvec; i += CL_NT) {
        const V v = pv[i];
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const double e = (double)v[j];
            sum += e;
            mx = e > mx ? e : mx;
        }
    }
    if (tid < tail) {
        const double v = (double)p[head + nvec * VEC + tid];
        sum += v;
        mx = v > mx ? v : mx;
    }
    sum = block_reduce_sum(sum, smem);
    mx = cl_block_max(mx, smax);
    if (tid == 0) {
        partial[2 * (size_t)blockIdx.x] = sum;
        partial[2 * (size_t)blockIdx.x + 1] = mx;
    }
}

// ---- 2. threshold, decode, vote, write --------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(CL_NT) void char_label_vote(const CLBatch b, const double* __restrict__ partial) {
    __shared__ double smem[17];
    __shared__ double smax[CL_NT / 64];
    __shared__ double s_thr;
    __shared__ unsigned long long stage[CL_STAGE_WORDS + 1];   // (+1: the decode reads two bytes per pixel)
    __shared__ unsigned char codes[CL_MAX_H * CL_COLS];
    __shared__ int win[CL_COLS];
    using V = typename EBVec<T>::type;
    constexpr int VEC = EBVec<T>::N;
    const int tid = threadIdx.x, lane = tid & 63;
    const int line = eb_entry_of(b.tile_first, b.n, blockIdx.x);
    const int tile = blockIdx.x - b.tile_first[line];
    const int h = b.line[line].h, w = b.line[line].w, c = b.c, bits = b.bits, n_chars = b.n_chars;
    const int x0 = tile * CL_COLS, ncols = w - x0 < CL_COLS ? w - x0 : CL_COLS;

    // the line's threshold from its partials: the same order in every block of the line and in every run
    {
        const int p0 = b.stat_first[line], np = b.stat_first[line + 1] - p0;
        double sum = 0.0, mx = -INFINITY;
        for (int i = tid; i < np; i += CL_NT) {
            sum += partial[2 * (size_t)(p0 + i)];
            const double m = partial[2 * (size_t)(p0 + i) + 1];
            mx = m > mx ? m : mx;
        }
        sum = block_reduce_sum(sum, smem);
        mx = cl_block_max(mx, smax);
        if (tid == 0) s_thr = 0.5 * (sum / (double)((size_t)h * w * c) + mx);
        __syncthreads();
    }
    const double thr = s_thr;

    // one bit per element of the tile, rows one after the other: element q = row * span + r
    const unsigned span = (unsigned)(ncols * c), total = (unsigned)h * span;
    const T* xt = (const T*)b.line[line].x + (size_t)x0 * c;
    const size_t pitch = (size_t)w * c;
    for (unsigned q0 = 0; q0 < total; q0 += CL_NT * CL_BATCH) {
        T v[CL_BATCH];
#pragma unroll
        for (int k = 0; k < CL_BATCH; ++k) {
            unsigned q = q0 + k * CL_NT + tid;
            q = q < total ? q : total - 1;                       // (a clamped address: no branch around the load)
            const unsigned row = q / span, r = q - row * span;
            v[k] = xt[row * pitch + r];
        }
#pragma unroll
        for (int k = 0; k < CL_BATCH; ++k) {
            const unsigned q = q0 + k * CL_NT + tid;
            const unsigned long long set = __ballot(q < total && (double)v[k] > thr);
            if (lane == 0 && q < total) stage[q >> 6] = set;     // (q is a multiple of 64 here)
        }
    }
    __syncthreads();

    // one byte per pixel: the class, or n_chars for every code that is none (no such code when n_chars = 2^bits)
    const unsigned char* sb = reinterpret_cast<const unsigned char*>(stage);
    for (int i = tid; i < h * CL_COLS; i += CL_NT) {
        const int row = i / CL_COLS, px = i % CL_COLS;
        if (px < ncols) {
            const unsigned off = (unsigned)row * span + (unsigned)(px * c);
            const unsigned two = (unsigned)sb[off >> 3] | ((unsigned)sb[(off >> 3) + 1] << 8);
            const int code = (int)((two >> (off & 7)) & ((1u << bits) - 1u));
            codes[i] = (unsigned char)(code < n_chars ? code : n_chars);
        }
    }
    __syncthreads();

    // the vote: CL_SUB lanes per column, lane j takes rows j, j + CL_SUB, ... upwards and keeps the strictly greater
    // count, so the first occurrence wins inside a lane; across lanes (count, then the smaller row)
    {
        const int px = tid / CL_SUB, j = tid % CL_SUB;
        int best_count = 0, best_row = INT32_MAX, best_code = 0;
        if (px < ncols)
            for (int y = j; y < h; y += CL_SUB) {
                const int mine = codes[y * CL_COLS + px];
                int same = 0;
                for (int y2 = 0; y2 < h; ++y2) same += codes[y2 * CL_COLS + px] == mine;
                if (same > best_count) best_count = same, best_row = y, best_code = mine;
            }
#pragma unroll
        for (int off = 1; off < CL_SUB; off <<= 1) {
            const int o_count = __shfl_xor(best_count, off, 64), o_row = __shfl_xor(best_row, off, 64);
            const int o_code = __shfl_xor(best_code, off, 64);
            if (o_count > best_count || (o_count == best_count && o_row < best_row))
                best_count = o_count, best_row = o_row, best_code = o_code;
        }
        if (j == 0 && px < ncols) {
            const int id = best_code < n_chars ? best_code : -1;
            win[px] = id;
            if (b.line[line].ids) b.line[line].ids[x0 + px] = id;
        }
    }
    __syncthreads();

    // the tile's rows of the labels are one contiguous range of ncols * n_chars elements
    T* out = (T*)b.line[line].labels + (size_t)x0 * n_chars;
    const int n = ncols * n_chars;
    const auto [head, nvec, tail] = eb_split(out, n);
    if (tid < head) out[tid] = (T)(win[tid / n_chars] == tid % n_chars ? 1.0f : 0.0f);
    V* ov = reinterpret_cast<V*>(out + head);
    for (int i = tid; i < nvec; i += CL_NT) {
        const int e = head + i * VEC;
        int px = e / n_chars, k = e - px * n_chars;
        V v;
#pragma unroll
        for (int jj = 0; jj < VEC; ++jj) {
            v[jj] = (T)(win[px] == k ? 1.0f : 0.0f);
            if (++k == n_chars) {
                k = 0;
                px = px + 1 < ncols ? px + 1 : px;               // (past the tile's last element: never stored)
            }
        }
        ov[i] = v;
    }
    if (tid < tail) {
        const int e = head + nvec * VEC + tid;
        out[e] = (T)(win[e / n_chars] == e % n_chars ? 1.0f : 0.0f);
    }
}

}  // namespace

extern "C" {

int uocr_char_label(uocr_ctx* ctx, int dtype, int n_lines, const void* const* x, const int* h, const int* w, int c,
                    int bits, int n_chars, void* const* labels, int* const* ids) {
    UOCR_CHECK_CTX(ctx);
    UOCR_REQUIRE(ctx, n_lines >= 0);
    if (n_lines == 0) return UOCR_OK;                              // nothing to do, whatever else was passed
    UOCR_REQUIRE(ctx, x && h && w && labels);
    const size_t elem = eb_storage_elem(ctx, dtype);
    if (!elem) return UOCR_ERR_DTYPE;
    UOCR_REQUIRE(ctx, bits >= 1 && bits <= 8);
    UOCR_REQUIRE(ctx, c >= bits && c <= CL_MAX_C);
    UOCR_REQUIRE(ctx, n_chars >= 1 && n_chars <= (1 << bits));
    const auto stat_blocks = [&](int i) { return ((long long)h[i] * w[i] * c + CL_CHUNK - 1) / CL_CHUNK; };
    const auto tile_blocks = [&](int i) { return (w[i] + CL_COLS - 1) / CL_COLS; };
    // everything is checked before the first launch: an error leaves every output as it was
    long long max_stat_blocks = 0;
    for (int first = 0; first < n_lines; first += CL_LINES) {
        const int count = eb_group_size(n_lines, first, CL_LINES);
        for (int i = first; i < first + count; ++i) {
            UOCR_REQUIRE(ctx, x[i] && labels[i] && (!ids || ids[i]));
            UOCR_REQUIRE(ctx, h[i] >= 1 && w[i] >= 1);
            UOCR_REQUIRE(ctx, (reinterpret_cast<uintptr_t>(x[i]) | reinterpret_cast<uintptr_t>(labels[i])) % elem == 0);
            UOCR_REQUIRE(ctx, !ids || reinterpret_cast<uintptr_t>(ids[i]) % sizeof(int) == 0);
            if (h[i] > CL_MAX_H)
                UOCR_FAIL(ctx, UOCR_ERR_UNSUPPORTED, "line %d is %d rows high: the vote kernel holds at most %d rows", i, h[i],
                          CL_MAX_H);
        }
        const long long group = eb_group_blocks(first, count, stat_blocks);
        if (group < 0 || eb_group_blocks(first, count, tile_blocks) < 0)
            UOCR_FAIL(ctx, UOCR_ERR_UNSUPPORTED, "lines %d..: too many blocks for one grid", first);
        max_stat_blocks = group > max_stat_blocks ? group : max_stat_blocks;
    }
    // workspace: (sum, max) per statistics block of one launch; the launch pairs of a call follow each other on the stream
    if (int rc = uocr_need_workspace(ctx, 2 * (size_t)max_stat_blocks * sizeof(double))) return rc;
    double* partial = (double*)ctx->workspace;
    int launches = 0;
    for (int first = 0; first < n_lines; first += CL_LINES) {
        CLBatch b;
        memset(&b, 0, sizeof(b));
        b.n = eb_group_size(n_lines, first, CL_LINES);
        eb_block_first(first, b.n, b.stat_first, stat_blocks);
        eb_block_first(first, b.n, b.tile_first, tile_blocks);
        b.c = c, b.bits = bits, b.n_chars = n_chars;
        for (int i = 0; i < b.n; ++i) {
            const int s = first + i;
            b.line[i].x = x[s], b.line[i].labels = labels[s], b.line[i].ids = ids ? ids[s] : nullptr;
            b.line[i].h = h[s], b.line[i].w = w[s];
        }
        UOCR_DISPATCH_STORAGE(ctx, dtype, {
            hipLaunchKernelGGL(char_label_stats<T>, dim3((unsigned)b.stat_first[b.n]), dim3(CL_NT), 0, ctx->stream, b,
                               partial);
            UOCR_LAUNCH_CHECK(ctx);
            hipLaunchKernelGGL(char_label_vote<T>, dim3((unsigned)b.tile_first[b.n]), dim3(CL_NT), 0, ctx->stream, b,
                               (const double*)partial);
            UOCR_LAUNCH_CHECK(ctx);
        });
        launches += 2;
    }
    uocr_note(ctx, UOCR_REPORT_CHAR_LABEL, CL_COLS, CL_CHUNK, CL_LINES, launches);
    return UOCR_OK;
}

int uocr_ctx_last_char_label(uocr_ctx* ctx, int* cols_per_block, int* stats_chunk, int* lines_per_launch, int* launches) {
    return uocr_report_read(ctx, UOCR_REPORT_CHAR_LABEL, cols_per_block, stats_chunk, lines_per_launch, launches);
}

}  // extern "C"
