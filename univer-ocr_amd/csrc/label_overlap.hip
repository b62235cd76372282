// LabelOverlap: the overlap counts of two label planes, and what a score of a mask net needs from them.  Entry i is a pair
// of int32 planes a[i] (the EXPECTED labels) and b[i] (the PREDICTED labels) of (h[i], w[i]) as uocr_label_batch writes
// them: 0 is the background, components are 1, 2, ...  With
//   bucket(l, cap) = l where 0 <= l <= cap (compared as unsigned: a negative label is large), else cap + 1, the OVERFLOW
// the call writes per entry
//   overlap [cap_a + 2][cap_b + 2]   overlap[r][s] = pixels p with bucket(a[p]) = r and bucket(b[p]) = s
//   rows    [cap_a + 2][4]           {area, best, inter, other} of row r: area = the sum of the row, best = the s in
//                                    1 .. cap_b with the largest overlap[r][s] > 0 (the smallest s on a tie, 0: none),
//                                    inter = overlap[r][best], other = the sum of column best (both 0 where best is 0)
//   cols    [cap_b + 2][4]           the same of the transposed table
//   summary [8] (int64)              tp, fp, fn, tn (foreground = any bucket but 0), expected / predicted = the rows /
//                                    columns 1 .. cap with area > 0, matched = the rows 1 .. cap_a with best > 0 and
//                                    2 inter > area + other - inter (IoU above 1/2), overflow = pixels with a bucket in
//                                    the overflow
// One memset of the tables per call, then two launches per LO_ENTRIES entries, the entries as by-value kernel arguments
// (entry_batch.h); no allocation, copy or host synchronisation, no workspace: asynchronous and capturable.
//   1. label_overlap_count   a histogram does not care for image rows: a block takes LO_PIXELS consecutive pixels of an
//                            entry, a wave LO_WAVE_PIXELS of them, in linear order.  16-byte loads of both planes between
//                            a scalar head and tail (the split is plane a's; plane b is read at the same pixels, 4-byte
//                            aligned, which global memory takes), LO_UNROLL tiles of 256 pixels requested before the first
//                            is consumed.  Label planes are long runs of equal pairs, so no lane adds per pixel: a lane
//                            folds its four pixels, lanes whose four are one pair fold across the wave (run heads from a
//                            compare with the lane before, lengths from a ballot and a find-first), and a tile that is one
//                            pair altogether goes to a (pair, count) carried in registers, flushed when the pair changes
//                            and at the end.  The counts go to a block-private table in LDS where the table has at most
//                            LO_LDS_CELLS cells -- the block then adds its non-zero cells to the global table, one
//                            no-return integer atomic each -- and straight to the global table otherwise.
//   2. label_overlap_reduce  a block per entry.  A wave per row of the table and a wave per column: the sum, and the first
//                            largest cell by a wave reduction over (count, index); results parked in LDS.  After a barrier
//                            every row takes the area of its best column, every column of its best row, both go out, and
//                            the block writes the summary from the finished rows and columns.
// Integer atomics only: the results are bit-identical run to run.
#include "entry_batch.h"

namespace {

constexpr int LO_NT = 256;                          // threads per block of both kernels
constexpr int LO_WAVES = LO_NT / 64;
constexpr int LO_TILE = 64 * 4;                     // pixels of a wave per 16-byte load
constexpr int LO_UNROLL = 4;                        // tiles a wave requests of each plane before it consumes the first
constexpr int LO_WAVE_PIXELS = 2 * LO_UNROLL * LO_TILE;
constexpr int LO_PIXELS = LO_WAVES * LO_WAVE_PIXELS;   // pixels per block: 8192
constexpr int LO_LDS_CELLS = 66 * 68;               // cells of a block-private table: caps 64 and 64 (66 x 66) fit
constexpr int LO_ENTRIES = 128;                     // entries per launch pair (the descriptor is a kernel argument)
constexpr int LO_MAX_CAP = 255;                     // rows and columns of a table the reduce block parks in LDS

struct LOEntry {
    const int* a;
    const int* b;
    int pixels;
};
struct LOBatch {
    LOEntry entry[LO_ENTRIES];
    int block_first[LO_ENTRIES + 1];
    int n, cap_a, cap_b;
};
static_assert(sizeof(LOBatch) <= 4096, "the descriptor travels as a kernel argument");

using lo_int4 = int __attribute__((ext_vector_type(4)));

// ---- 1. the counts ------------------------------------------------------------------------------------------------------
template <bool LDS>
__device__ __forceinline__ void lo_add(int* __restrict__ table, unsigned cell, int count) {
    if constexpr (LDS) atomicAdd(table + cell, count);                                    // (ds_add_u32)
    else (void)__hip_atomic_fetch_add(table + cell, count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // no-return
}

__device__ __forceinline__ unsigned lo_cell(int la, int lb, unsigned cap_a, unsigned cap_b) {
    const unsigned r = (unsigned)la <= cap_a ? (unsigned)la : cap_a + 1;
    const unsigned s = (unsigned)lb <= cap_b ? (unsigned)lb : cap_b + 1;
    return r * (cap_b + 2) + s;
}

// the pair a wave carries from tile to tile
struct LOCarry {
    unsigned cell;
    int count;                                      // 0: nothing carried
};

// one tile: lane l holds the cells k[0..3] of four consecutive pixels (live) or nothing
template <bool LDS>
__device__ __forceinline__ void lo_tile(int* __restrict__ table, const unsigned (&k)[4], bool live, LOCarry& carry, int lane) {
    const bool uniform = live && k[0] == k[1] && k[1] == k[2] && k[2] == k[3];
    const unsigned long long u = __ballot(uniform);                           // the lanes that hold one pair
    const unsigned before = __shfl_up(k[0], 1, 64);
    const bool head = uniform && (lane == 0 || !((u >> (lane - 1)) & 1ull) || before != k[0]);
    const unsigned long long heads = __ballot(head);
    if (u == ~0ull && heads == 1ull) {                                        // the whole tile is one pair (wave-uniform)
        const unsigned cell = __builtin_amdgcn_readfirstlane(k[0]);
        if (carry.count && carry.cell != cell) {
            if (lane == 0) lo_add<LDS>(table, carry.cell, carry.count);
            carry.count = 0;
        }
        carry.cell = cell, carry.count += LO_TILE;
        return;
    }
    if (head) {                                                               // a run of such lanes: up to the next head or
        const unsigned long long stops = heads | ~u;                          // the next lane of another kind
        const unsigned long long after = lane == 63 ? 0ull : stops & (~0ull << (lane + 1));
        const int end = after ? __builtin_ctzll(after) : 64;
        lo_add<LDS>(table, k[0], 4 * (end - lane));
    } else if (live && !uniform) {                                            // the runs inside the lane
        int count = 1;
#pragma unroll
        for (int j = 1; j < 4; ++j) {
            if (k[j] == k[j - 1]) ++count;
            else {
                lo_add<LDS>(table, k[j - 1], count);
                count = 1;
            }
        }
        lo_add<LDS>(table, k[3], count);
    }
}

template <bool LDS>
__global__ __launch_bounds__(LO_NT) void label_overlap_count(const LOBatch b, int first_entry, int* __restrict__ overlap) {
    __shared__ int lds[LDS ? LO_LDS_CELLS : 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int entry = eb_entry_of(b.block_first, b.n, blockIdx.x);
    const LOEntry& e = b.entry[entry];
    const unsigned cap_a = (unsigned)b.cap_a, cap_b = (unsigned)b.cap_b;
    const int cells = (b.cap_a + 2) * (b.cap_b + 2);
    int* global = overlap + (size_t)(first_entry + entry) * cells;
    int* table = LDS ? lds : global;
    if constexpr (LDS) {
        for (int c = threadIdx.x; c < cells; c += LO_NT) lds[c] = 0;
        __syncthreads();
    }
    // the wave's pixels [start, start + n) of the entry
    const long long start = (long long)(blockIdx.x - b.block_first[entry]) * LO_PIXELS + (long long)wave * LO_WAVE_PIXELS;
    const long long left = (long long)e.pixels - start;
    const int n = left < 0 ? 0 : left < LO_WAVE_PIXELS ? (int)left : LO_WAVE_PIXELS;
    if (n > 0) {                                                              // (wave-uniform)
        const int* pa = e.a + start;
        const int* pb = e.b + start;
        const EBSplit split = eb_split(pa, n);
        // head and tail: at most three pixels each, a pixel per lane
        {
            const int at = lane < split.head ? lane : lane >= 4 && lane - 4 < split.tail ? split.head + 4 * split.nvec + lane - 4 : -1;
            if (at >= 0) lo_add<LDS>(table, lo_cell(pa[at], pb[at], cap_a, cap_b), 1);
        }
        const lo_int4* va = reinterpret_cast<const lo_int4*>(pa + split.head);
        const int* sb = pb + split.head;
        LOCarry carry{0u, 0};
        for (int t0 = 0; t0 * 64 < split.nvec; t0 += LO_UNROLL) {
            lo_int4 xa[LO_UNROLL], xb[LO_UNROLL];
#pragma unroll
            for (int q = 0; q < LO_UNROLL; ++q) {                             // every load of LO_UNROLL tiles
                const int i = (t0 + q) * 64 + lane;
                xa[q] = lo_int4{}, xb[q] = lo_int4{};
                if (i < split.nvec) {
                    xa[q] = va[i];
                    __builtin_memcpy(&xb[q], sb + 4 * (size_t)i, 16);         // 16 bytes at a 4-byte alignment
                }
            }
#pragma unroll
            for (int q = 0; q < LO_UNROLL; ++q) {
                if ((t0 + q) * 64 >= split.nvec) break;                       // (wave-uniform)
                const bool live = (t0 + q) * 64 + lane < split.nvec;
                unsigned k[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) k[j] = lo_cell(xa[q][j], xb[q][j], cap_a, cap_b);
                lo_tile<LDS>(table, k, live, carry, lane);
            }
        }
        if (carry.count && lane == 0) lo_add<LDS>(table, carry.cell, carry.count);
    }
    if constexpr (LDS) {
        __syncthreads();
        for (int c = threadIdx.x; c < cells; c += LO_NT) {
            const int v = lds[c];
            if (v) lo_add<false>(global, (unsigned)c, v);
        }
    }
}

// ---- 2. rows, columns, summary ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LO_NT) void label_overlap_reduce(int cap_a, int cap_b, int first_entry,
                                                             const int* __restrict__ overlap, int* __restrict__ rows,
                                                             int* __restrict__ cols, long long* __restrict__ summary) {
    __shared__ int line[2 * (LO_MAX_CAP + 2)][4];                             // the rows, then the columns
    __shared__ long long part[LO_WAVES][3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int entry = first_entry + blockIdx.x;
    const int R = cap_a + 2, S = cap_b + 2;
    const int* table = overlap + (size_t)entry * R * S;
    for (int task = wave; task < R + S; task += LO_WAVES) {                   // a wave per row, then per column
        const bool is_row = task < R;
        const int index = is_row ? task : task - R;
        const int length = is_row ? S : R, cap = is_row ? cap_b : cap_a;
        const int* p = is_row ? table + (size_t)index * S : table + index;
        const int step = is_row ? 1 : S;
        int area = 0, most = 0, at = 0;                                       // (most == 0: no candidate yet)
        for (int i = lane; i < length; i += 64) {                             // a lane meets its cells in ascending order
            const int v = p[(size_t)i * step];
            area += v;
            const bool better = i >= 1 && i <= cap && v > most;
            most = better ? v : most;
            at = better ? i : at;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {                              // the first largest ends in lane 0
            area += __shfl_down(area, off, 64);
            const int omost = __shfl_down(most, off, 64), oat = __shfl_down(at, off, 64);
            const bool better = omost > most || (omost == most && omost > 0 && oat < at);
            most = better ? omost : most;
            at = better ? oat : at;
        }
        if (lane == 0) line[task][0] = area, line[task][1] = at, line[task][2] = most, line[task][3] = 0;
    }
    __syncthreads();
    for (int task = threadIdx.x; task < R + S; task += LO_NT) {               // the area of the best line of the other kind
        const bool is_row = task < R;
        const int best = line[task][1];
        const int other = best ? line[is_row ? R + best : best][0] : 0;
        line[task][3] = other;
        int* out = is_row ? rows + ((size_t)entry * R + task) * 4 : cols + ((size_t)entry * S + task - R) * 4;
        out[0] = line[task][0], out[1] = best, out[2] = line[task][2], out[3] = other;
    }
    __syncthreads();
    long long expected = 0, predicted = 0, matched = 0;
    for (int r = 1 + (int)threadIdx.x; r <= cap_a; r += LO_NT) {
        const long long area = line[r][0], inter = line[r][2], other = line[r][3];
        expected += area > 0;
        matched += line[r][1] > 0 && 2 * inter > area + other - inter;
    }
    for (int s = 1 + (int)threadIdx.x; s <= cap_b; s += LO_NT) predicted += line[R + s][0] > 0;
    expected = wave_reduce_sum(expected), predicted = wave_reduce_sum(predicted), matched = wave_reduce_sum(matched);
    if (lane == 0) part[wave][0] = expected, part[wave][1] = predicted, part[wave][2] = matched;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < LO_WAVES; ++k) expected += part[k][0], predicted += part[k][1], matched += part[k][2];
        long long total = 0;
        for (int r = 0; r < R; ++r) total += line[r][0];                      // every pixel of the entry
        const long long tn = table[0];
        const long long fp = line[0][0] - tn, fn = line[R][0] - tn;           // row 0 and column 0 without their corner
        const long long overflow = (long long)line[R - 1][0] + line[R + S - 1][0] - table[(size_t)R * S - 1];
        long long* out = summary + (size_t)entry * 8;
        out[0] = total - tn - fp - fn, out[1] = fp, out[2] = fn, out[3] = tn;
        out[4] = expected, out[5] = predicted, out[6] = matched, out[7] = overflow;
    }
}

}  // namespace

extern "C" {

int uocr_label_overlap(uocr_ctx* ctx, int n_entries, const int* const* a, const int* const* b, const int* h, const int* w,
                       int cap_a, int cap_b, int* overlap, int* rows, int* cols, long long* summary) {
    UOCR_CHECK_CTX(ctx);
    UOCR_REQUIRE(ctx, n_entries >= 0);
    if (n_entries == 0) return UOCR_OK;                            // nothing to do, whatever else was passed
    UOCR_REQUIRE(ctx, a && b && h && w && overlap && rows && cols && summary);
    UOCR_REQUIRE(ctx, cap_a >= 0 && cap_b >= 0);
    UOCR_REQUIRE(ctx, reinterpret_cast<uintptr_t>(overlap) % sizeof(int) == 0);
    UOCR_REQUIRE(ctx, reinterpret_cast<uintptr_t>(rows) % sizeof(int) == 0);
    UOCR_REQUIRE(ctx, reinterpret_cast<uintptr_t>(cols) % sizeof(int) == 0);
    UOCR_REQUIRE(ctx, reinterpret_cast<uintptr_t>(summary) % sizeof(long long) == 0);
    if (cap_a > LO_MAX_CAP || cap_b > LO_MAX_CAP)
        UOCR_FAIL(ctx, UOCR_ERR_UNSUPPORTED, "caps %d and %d: the largest is %d", cap_a, cap_b, LO_MAX_CAP);
    const auto blocks = [&](int i) { return ((long long)h[i] * w[i] + LO_PIXELS - 1) / LO_PIXELS; };
    // everything is checked before the memset: an error leaves every output as it was
    for (int first = 0; first < n_entries; first += LO_ENTRIES) {
        const int group = eb_group_size(n_entries, first, LO_ENTRIES);
        for (int i = first; i < first + group; ++i) {
            UOCR_REQUIRE(ctx, h[i] >= 1 && w[i] >= 1);
            UOCR_REQUIRE(ctx, a[i] && b[i]);
            UOCR_REQUIRE(ctx, reinterpret_cast<uintptr_t>(a[i]) % sizeof(int) == 0);
            UOCR_REQUIRE(ctx, reinterpret_cast<uintptr_t>(b[i]) % sizeof(int) == 0);
            if ((long long)h[i] * w[i] > INT32_MAX)
                UOCR_FAIL(ctx, UOCR_ERR_UNSUPPORTED, "entry %d: %d x %d pixels do not fit an int", i, h[i], w[i]);
        }
        if (eb_group_blocks(first, group, blocks) < 0)
            UOCR_FAIL(ctx, UOCR_ERR_UNSUPPORTED, "entries %d..: too many blocks for one grid", first);
    }
    const size_t cells = (size_t)(cap_a + 2) * (cap_b + 2);
    UOCR_HIP(ctx, hipMemsetAsync(overlap, 0, (size_t)n_entries * cells * sizeof(int), ctx->stream));
    for (int first = 0; first < n_entries; first += LO_ENTRIES) {
        LOBatch d;
        memset(&d, 0, sizeof(d));
        d.n = eb_group_size(n_entries, first, LO_ENTRIES);
        d.cap_a = cap_a, d.cap_b = cap_b;
        eb_block_first(first, d.n, d.block_first, blocks);
        for (int i = 0; i < d.n; ++i) d.entry[i] = LOEntry{a[first + i], b[first + i], h[first + i] * w[first + i]};
        const dim3 grid((unsigned)d.block_first[d.n]);
        if (cells <= (size_t)LO_LDS_CELLS)
            hipLaunchKernelGGL(label_overlap_count<true>, grid, dim3(LO_NT), 0, ctx->stream, d, first, overlap);
        else
            hipLaunchKernelGGL(label_overlap_count<false>, grid, dim3(LO_NT), 0, ctx->stream, d, first, overlap);
        UOCR_LAUNCH_CHECK(ctx);
        hipLaunchKernelGGL(label_overlap_reduce, dim3((unsigned)d.n), dim3(LO_NT), 0, ctx->stream, cap_a, cap_b, first,
                           (const int*)overlap, rows, cols, summary);
        UOCR_LAUNCH_CHECK(ctx);
    }
    return UOCR_OK;
}

int uocr_label_overlap_limits(int* pixels_per_block, int* lds_cells, int* entries_per_launch, int* max_cap) {
    if (!pixels_per_block || !lds_cells || !entries_per_launch || !max_cap) return UOCR_ERR_ARG;
    *pixels_per_block = LO_PIXELS, *lds_cells = LO_LDS_CELLS, *entries_per_launch = LO_ENTRIES, *max_cap = LO_MAX_CAP;
    return UOCR_OK;
}

}  // extern "C"
