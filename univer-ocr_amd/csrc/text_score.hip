// TextScore: how well the Char net read a line, as an edit distance between two readings.  Per line, pred is the Char
// net's raw output (W, n_chars) and label the one-hot labels of the same W columns (char_label.hip).  Both are read by
// ONE rule:
//   row id   -1 where the row holds a NaN or its maximum == 0.0 (-0.0 included); otherwise the SMALLEST column that
//            equals the row's maximum (a negative maximum is a maximum like any other) -- PredToText's conventions
//   reading  the ids of the runs of equal row ids; id 0 (the tab, the background class) and -1 emit nothing and end a run
// and the score of the line is the unit-cost Levenshtein distance between reading(label), the EXPECTED string, and
// reading(pred), the READ string, two ids matching when canon[x] == canon[y] -- the caller's table, the library knows no
// alphabet.  A reading is never longer than W.
//
// All lines of a call travel together, TS_LINES per launch pair, their pointers, sizes and the table in a by-value kernel
// argument (no device allocation, no copy, no host synchronisation: asynchronous and capturable).  Launches per TS_LINES
// lines:
//   1. text_score_read   the 2 x lines matrices are the entries; a block takes TS_ROWS consecutive rows of one matrix, a
//                        wave a row: 16-byte loads between a scalar head and tail, TS_UNROLL rows requested before the
//                        first is reduced; a wave reduction over (value, column) keeps the first maximum, a ballot the
//                        NaN flag.  One byte per row goes to the ctx workspace (TS_NONE: -1).  The only kernel that moves
//                        real bytes: both matrices cross HBM once.
//   2. text_score_dp     a wave per line, TS_WAVES lines per block, no barrier and no LDS.  Both row-id strings are
//                        collapsed 64 rows at a time (a ballot of "id > 0 and id != the row before", the last id of a
//                        chunk carried into the next, positions by popcount prefixes) into the workspace, next to
//                        their canon entries, and, where the caller gave buffers, into them.  The distance runs as a skewed wavefront: lane j owns K
//                        consecutive columns of the expected string with the previous row of its K cells in registers and
//                        handles row t - j of the read string at step t.  From lane j - 1 it needs that lane's last cell of
//                        the same row (made one step earlier) and of the row before (what it received the step before):
//                        ONE __shfl_up per step, the read character packed into the same word and moving down the lanes
//                        with it.  Lane 0 is fed from register chunks of 64 characters and 64 boundary cells, reloaded
//                        every 64 steps and requested a chunk ahead.  K is 1, 2 or 4 (the smallest that covers the expected string); a longer string
//                        runs as panels of TS_PANEL columns, the right boundary column of a panel parked in the workspace
//                        (two buffers in turn) as lane 0's left input of the next.
// Comparisons and integer arithmetic only (binary16 is widened to float32, which is exact): no floating-point result
// exists.  No atomics: bit-identical run to run.
#include "entry_batch.h"

namespace {

constexpr int TS_NT = 256;               // threads per block of both kernels
constexpr int TS_WAVES = TS_NT / 64;     // rows in flight per read block; lines per dp block
constexpr int TS_ROWS = 64;              // rows of a matrix per read block
constexpr int TS_UNROLL = 4;             // rows a wave requests before it reduces the first
constexpr int TS_LINES = 64;             // lines per launch pair (the descriptor is a kernel argument: 4 KB at most)
constexpr int TS_MAX_CHARS = 255;        // ids are bytes and TS_NONE is taken
constexpr int TS_NONE = 255;             // the row id -1 as a byte
constexpr int TS_KMAX = 4;               // columns of the expected string per lane, at most
constexpr int TS_PANEL = 64 * TS_KMAX;   // columns per panel
constexpr int TS_MAX_WIDTH = 1 << 16;    // rows of a line (a cell, at most 2 * width, travels in 24 bits)
constexpr int TS_NO_CHAR = 256;          // what lanes past the end of the expected string hold: matches nothing

struct TSLine {
    const void* pred;
    const void* label;
    unsigned char* read_ids;             // or null
    unsigned char* expected_ids;         // or null
    int w;
    unsigned scratch;                    // of this line in the workspace, bytes from the scratch base (a multiple of 4):
                                         // two boundary columns of w + 1 ints, then w bytes each: the read ids, the
                                         // expected ids and both again as their canon entries
};
struct TSBatch {
    TSLine line[TS_LINES];
    int block_first[2 * TS_LINES + 1];   // first read block of matrix 2 * line + (0: pred, 1: label)
    unsigned char canon[TS_MAX_CHARS + 1];
    int n, n_chars;
};
static_assert(sizeof(TSBatch) <= 4096, "the descriptor travels as a kernel argument");

__host__ __device__ inline size_t ts_scratch_bytes(int w) { return (size_t)8 * (w + 1) + 4 * (size_t)w; }

// ---- 1. the id of every row -------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(TS_NT) void text_score_read(const TSBatch b, unsigned char* __restrict__ rows) {
    using CT = std::conditional_t<std::is_same_v<T, double>, double, float>;   // binary16 -> float32 is exact
    using V = typename EBVec<T>::type;
    constexpr int VEC = EBVec<T>::N;
    constexpr int TRIPS = (TS_MAX_CHARS / VEC + 63) / 64;             // vector loads of a lane per row, at most
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int entry = eb_entry_of(b.block_first, 2 * b.n, blockIdx.x);
    const int row0 = (blockIdx.x - b.block_first[entry]) * TS_ROWS;
    const TSLine& line = b.line[entry >> 1];
    const T* base = (const T*)((entry & 1) ? line.label : line.pred);
    const int n_chars = b.n_chars;
    const int nrows = line.w - row0 < TS_ROWS ? line.w - row0 : TS_ROWS;
    for (int r0 = wave * TS_UNROLL; r0 < nrows; r0 += TS_WAVES * TS_UNROLL) {
        T hv[TS_UNROLL], tv[TS_UNROLL];
        V vv[TS_UNROLL][TRIPS];
        EBSplit split[TS_UNROLL];
#pragma unroll
        for (int q = 0; q < TS_UNROLL; ++q) {                         // every load of TS_UNROLL rows (past the end: the last row again)
            const int r = r0 + q < nrows ? r0 + q : nrows - 1;
            const T* p = base + (size_t)(row0 + r) * n_chars;
            split[q] = eb_split(p, n_chars);
            const V* pv = reinterpret_cast<const V*>(p + split[q].head);
            hv[q] = lane < split[q].head ? p[lane] : T(0);
#pragma unroll
            for (int trip = 0; trip < TRIPS; ++trip) {
                const int i = lane + 64 * trip;
                vv[q][trip] = i < split[q].nvec ? pv[i] : V{};
            }
            const int at = split[q].head + split[q].nvec * VEC + lane;
            tv[q] = lane < split[q].tail ? p[at] : T(0);
        }
#pragma unroll
        for (int q = 0; q < TS_UNROLL; ++q) {
            CT mx = -INFINITY;
            int col = INT32_MAX;                                       // (a lane without an element never wins a tie)
            bool nan = false;
            const auto take = [&](int c, CT v) {                       // a lane meets its columns in ascending order
                nan |= v != v;
                const bool better = v > mx || (v == mx && c < col);
                mx = better ? v : mx;
                col = better ? c : col;
            };
            if (lane < split[q].head) take(lane, (CT)hv[q]);
#pragma unroll
            for (int trip = 0; trip < TRIPS; ++trip) {
                const int i = lane + 64 * trip;
                if (i < split[q].nvec) {
#pragma unroll
                    for (int j = 0; j < VEC; ++j) take(split[q].head + i * VEC + j, (CT)vv[q][trip][j]);
                }
            }
            if (lane < split[q].tail) take(split[q].head + split[q].nvec * VEC + lane, (CT)tv[q]);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {                   // the first maximum of the row ends in lane 0
                const CT omx = __shfl_down(mx, off, 64);
                const int ocol = __shfl_down(col, off, 64);
                const bool better = omx > mx || (omx == mx && ocol < col);
                mx = better ? omx : mx;
                col = better ? ocol : col;
            }
            const bool dead = __ballot(nan) != 0ull;
            if (lane == 0 && r0 + q < nrows)                           // (-0.0 == 0.0: such a row reads as nothing)
                rows[(size_t)blockIdx.x * TS_ROWS + r0 + q] = (unsigned char)(dead || mx == (CT)0 ? TS_NONE : col);
        }
    }
}

// ---- 2. the two readings and their distance ---------------------------------------------------------------------------
// the reading of the w row ids at `rows`: to `out` (and to `also` unless null), its canon entries to `out_canon`; returns
// its length (wave-uniform)
__device__ __forceinline__ int ts_collapse(const unsigned char* __restrict__ rows, int w, const unsigned char* __restrict__ canon,
                                           unsigned char* out, unsigned char* out_canon, unsigned char* also, int lane) {
    int carry = TS_NONE, length = 0;                                   // (no id equals TS_NONE: row 0 starts a run)
    for (int r0 = 0; r0 < w; r0 += 64) {
        const int r = r0 + lane;
        const int id = r < w ? (int)rows[r] : TS_NONE;
        int before = __shfl_up(id, 1, 64);
        before = lane == 0 ? carry : before;
        carry = __shfl(id, 63, 64);
        const bool emit = id != TS_NONE && id != 0 && id != before;
        const unsigned long long mask = __ballot(emit);
        if (emit) {
            const int at = length + __popcll(mask & ((1ull << lane) - 1ull));
            out[at] = (unsigned char)id;
            out_canon[at] = canon[id];
            if (also) also[at] = (unsigned char)id;
        }
        length += __popcll(mask);
    }
    return length;
}

// One panel: columns (c0, c0 + 64 K] of the expected string `e` (m canon entries) against all n of the read string `r`.
// `left`: the column c0 of the table, cell i at left[i] for i = 1 .. n (cell 0 is c0), or null for c0 = 0 (cell i of it
// is i); `right`: where column c0 + 64 K goes in the same form, or null when no panel follows.  Returns the cell (n, m)
// where this panel holds it (in every lane), else -1.
template <int K>
__device__ __forceinline__ int ts_panel(const unsigned char* __restrict__ e, int m, const unsigned char* __restrict__ r, int n,
                                        int c0, const int* __restrict__ left, int* __restrict__ right, int lane) {
    int ech[K], above[K];                                              // the lane's characters; row i - 1 of its cells
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int c = c0 + lane * K + k;                               // 0-based position in e of column c + 1
        ech[k] = c < m ? (int)e[c] : TS_NO_CHAR;
        above[k] = c + 1;
    }
    int corner = c0 + lane * K;                                        // cell (i - 1, the column left of the lane's first)
    unsigned out = 0;                                                  // (last cell << 8 | read character) of the lane's last row
    int chunk_char = 0, chunk_left = 0;                                // of row 64 q + 1 + lane, for lane 0's input ...
    int next_char = lane < n ? (int)r[lane] : 0;                       // ... and of the chunk after it, requested 64 steps ahead
    int next_left = left ? (lane < n ? left[lane + 1] : 0) : lane + 1;
    const int last_lane = m - c0 > 64 * K ? 63 : (m - c0 - 1) / K;     // the last lane that owns a column of e
    const int steps = n + last_lane;
    for (int t = 1; t <= steps; ++t) {
        if (((t - 1) & 63) == 0) {
            const int i = t + 64 + lane;
            chunk_char = next_char, chunk_left = next_left;
            next_char = i <= n ? (int)r[i - 1] : 0;
            next_left = left ? (i <= n ? left[i] : 0) : i;
        }
        unsigned in = __shfl_up(out, 1, 64);
        const int src = (t - 1) & 63;
        const unsigned fed = ((unsigned)__builtin_amdgcn_readlane(chunk_left, src) << 8) |
                             (unsigned)__builtin_amdgcn_readlane(chunk_char, src);
        in = lane == 0 ? fed : in;
        const int i = t - lane;
        if (i >= 1 && i <= n) {
            const int ch = (int)(in & 255u);
            int beside = (int)(in >> 8), diagonal = corner;
            corner = beside;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int up = above[k];
                int v = up < beside ? up : beside;
                v += 1;
                const int match = diagonal + (ch != ech[k] ? 1 : 0);
                v = match < v ? match : v;
                diagonal = up;
                beside = above[k] = v;
            }
            out = ((unsigned)beside << 8) | (unsigned)ch;
            if (right && lane == 63) right[i] = beside;
        }
    }
    if (m - c0 > 64 * K) return -1;
    int mine = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) mine = (m - c0 - 1) % K == k ? above[k] : mine;
    return __shfl(mine, last_lane, 64);
}

__global__ __launch_bounds__(TS_NT) void text_score_dp(const TSBatch b, const unsigned char* __restrict__ rows,
                                                       unsigned char* __restrict__ scratch, int* __restrict__ scores) {
    const int lane = threadIdx.x & 63;
    const int index = blockIdx.x * TS_WAVES + (threadIdx.x >> 6);
    if (index >= b.n) return;                                          // (wave-uniform; there is no barrier below)
    const TSLine& line = b.line[index];
    const int w = line.w;
    int* boundary = (int*)(scratch + line.scratch);
    unsigned char* ids = (unsigned char*)(boundary + 2 * (w + 1));
    const unsigned char *rd = ids + 2 * w, *ex = ids + 3 * w;         // the canon entries of the two readings
    const int n = ts_collapse(rows + (size_t)b.block_first[2 * index] * TS_ROWS, w, b.canon, ids, ids + 2 * w, line.read_ids, lane);
    const int m = ts_collapse(rows + (size_t)b.block_first[2 * index + 1] * TS_ROWS, w, b.canon, ids + w, ids + 3 * w,
                              line.expected_ids, lane);
    __threadfence();                                                   // the ids are read back by other lanes of this wave
    int distance = m == 0 ? n : m;                                     // (one string empty: the length of the other)
    if (m > 0 && n > 0) {
        if (m <= 64) distance = ts_panel<1>(ex, m, rd, n, 0, nullptr, nullptr, lane);
        else if (m <= 128) distance = ts_panel<2>(ex, m, rd, n, 0, nullptr, nullptr, lane);
        else {
            int turn = 0;
            for (int c0 = 0; c0 < m; c0 += TS_PANEL, turn ^= 1) {
                int* right = m - c0 > TS_PANEL ? boundary + turn * (w + 1) : nullptr;
                const int* left = c0 ? boundary + (turn ^ 1) * (w + 1) : nullptr;
                distance = ts_panel<TS_KMAX>(ex, m, rd, n, c0, left, right, lane);
                __threadfence();                                       // lane 63 wrote what lane 0 reads next
            }
        }
    }
    if (lane < 4) scores[4 * index + lane] = lane == 0 ? distance : lane == 1 ? m : lane == 2 ? n : 0;
}

}  // namespace

extern "C" {

int uocr_text_score(uocr_ctx* ctx, int dtype, int n_lines, const void* const* pred, const void* const* label, const int* w,
                    int n_chars, const int* canon, unsigned char* const* read_ids, unsigned char* const* expected_ids,
                    int* scores) {
    UOCR_CHECK_CTX(ctx);
    UOCR_REQUIRE(ctx, n_lines >= 0);
    if (n_lines == 0) return UOCR_OK;                              // nothing to do, whatever else was passed
    UOCR_REQUIRE(ctx, pred && label && w && canon && scores);
    UOCR_REQUIRE(ctx, reinterpret_cast<uintptr_t>(scores) % sizeof(int) == 0);
    const size_t elem = eb_storage_elem(ctx, dtype);
    if (!elem) return UOCR_ERR_DTYPE;
    UOCR_REQUIRE(ctx, n_chars >= 1 && n_chars <= TS_MAX_CHARS);
    for (int k = 0; k < n_chars; ++k) UOCR_REQUIRE(ctx, canon[k] >= 0 && canon[k] < n_chars);
    const auto blocks = [&](int i) { return ((long long)w[i >> 1] + TS_ROWS - 1) / TS_ROWS; };   // of matrix i of the call
    // everything is checked before the first launch: an error leaves every output as it was
    long long max_blocks = 0;
    size_t max_scratch = 0;
    for (int first = 0; first < n_lines; first += TS_LINES) {
        const int group = eb_group_size(n_lines, first, TS_LINES);
        size_t scratch = 0;
        for (int i = first; i < first + group; ++i) {
            UOCR_REQUIRE(ctx, w[i] >= 1 && w[i] <= TS_MAX_WIDTH);
            UOCR_REQUIRE(ctx, pred[i] && label[i]);
            UOCR_REQUIRE(ctx, reinterpret_cast<uintptr_t>(pred[i]) % elem == 0);
            UOCR_REQUIRE(ctx, reinterpret_cast<uintptr_t>(label[i]) % elem == 0);
            scratch += ts_scratch_bytes(w[i]);
        }
        const long long total = eb_group_blocks(2 * first, 2 * group, blocks);
        if (total < 0) UOCR_FAIL(ctx, UOCR_ERR_UNSUPPORTED, "lines %d..: too many blocks for one grid", first);
        max_blocks = total > max_blocks ? total : max_blocks;
        max_scratch = scratch > max_scratch ? scratch : max_scratch;
    }
    // workspace: the row ids of one launch pair (a multiple of 64 bytes), then every line's scratch; the pairs of a call
    // follow each other on the stream
    const size_t row_bytes = (size_t)max_blocks * TS_ROWS;
    if (int rc = uocr_need_workspace(ctx, row_bytes + max_scratch)) return rc;
    unsigned char* rows = (unsigned char*)ctx->workspace;
    unsigned char* scratch = rows + row_bytes;
    for (int first = 0; first < n_lines; first += TS_LINES) {
        TSBatch b;
        memset(&b, 0, sizeof(b));
        b.n = eb_group_size(n_lines, first, TS_LINES);
        eb_block_first(2 * first, 2 * b.n, b.block_first, blocks);
        b.n_chars = n_chars;
        for (int k = 0; k < n_chars; ++k) b.canon[k] = (unsigned char)canon[k];
        size_t at = 0;
        for (int i = 0; i < b.n; ++i) {
            const int s = first + i;
            b.line[i].pred = pred[s], b.line[i].label = label[s], b.line[i].w = w[s];
            b.line[i].read_ids = read_ids ? read_ids[s] : nullptr;
            b.line[i].expected_ids = expected_ids ? expected_ids[s] : nullptr;
            b.line[i].scratch = (unsigned)at;
            at += ts_scratch_bytes(w[s]);
        }
        UOCR_DISPATCH_STORAGE(ctx, dtype, {
            hipLaunchKernelGGL(text_score_read<T>, dim3((unsigned)b.block_first[2 * b.n]), dim3(TS_NT), 0, ctx->stream, b, rows);
            UOCR_LAUNCH_CHECK(ctx);
        });
        hipLaunchKernelGGL(text_score_dp, dim3((unsigned)((b.n + TS_WAVES - 1) / TS_WAVES)), dim3(TS_NT), 0, ctx->stream, b,
                           (const unsigned char*)rows, scratch, scores + 4 * (size_t)first);
        UOCR_LAUNCH_CHECK(ctx);
    }
    return UOCR_OK;
}

int uocr_text_score_limits(int* rows_per_block, int* lines_per_launch, int* columns_per_panel, int* max_width) {
    if (!rows_per_block || !lines_per_launch || !columns_per_panel || !max_width) return UOCR_ERR_ARG;
    *rows_per_block = TS_ROWS, *lines_per_launch = TS_LINES, *columns_per_panel = TS_PANEL, *max_width = TS_MAX_WIDTH;
    return UOCR_OK;
}

}  // extern "C"
