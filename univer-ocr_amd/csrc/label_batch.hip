// Connected components of a LIST of images in one call: the labelling every paragraph of a page starts its line finding
// with (interpreter/interpreter.py:437-438 the two thresholded line masks, :16-21 ndimage.label, :36-39 center_of_mass,
// :494-502 the boxes), for all paragraphs at once.  Entry i is ONE CHANNEL of an interleaved (1, h, w, c) tensor, read in
// place: pixel (y, x) is the element at (y * w + x) * c + channel.  Sizes differ from entry to entry.
//
// The chain is that of label.hip, and the body of every step is the same code (label_common.h); what differs is how a
// block finds its image.  The entries of a call travel in by-value kernel arguments, LB_ENTRIES per group, next to the
// prefix sums of their block counts in each of the four grids (entry_batch.h); linear indices and roots are
// entry-LOCAL int32, every entry has an offset into one root plane in the ctx workspace, and its label plane is
// labels[i] or, where the caller wants no labels, lies in the workspace too.  Launches of one group, all on the
// context's stream, whatever the number of entries:
//   1. lb_stats     one block per LB_STAT pixels of an entry: float64 sum and max of its channel go to the workspace
//                   (not for UOCR_THRESH_VALUE)
//   2. lb_local     one block per tile.  It adds its entry's partials itself, in a fixed order (every block of an entry
//                   gets the same bits; nobody waits for anybody inside a launch), then the tile-local union-find
//   3. lb_merge     unions across tile borders (only when an entry of the group has more than one tile)
//   4. lb_flatten   root of every pixel + roots per chunk of LCHUNK pixels
//   5. lb_scan      one block per ENTRY: exclusive scan of its chunk counts, count[i]
//   6. lb_rank      number of every root, its table entry initialised
//   7. lb_relabel   final labels and the table
// and ONE memset of the whole table per call.  The only exchange between blocks inside a launch is the one label.hip
// has: relaxed agent-scope atomicMin on links that only decrease (3) and integer atomics into the table (7).  Every
// other hand-off is a kernel boundary: no arrival counter, no grid barrier, nothing spins.
#include "label_common.h"

namespace {

constexpr int LB_ENTRIES = 32;             // entries per group (the descriptor is a kernel argument: 4 KB at most)
constexpr int LB_STAT = 4096;              // pixels per block of lb_stats

struct LBEntry {
    const void* x;
    int* plane;                            // labels[i], or the entry's plane in the workspace
    long long root_off;                    // first int of the entry in the root plane
    int h, w, c, channel;
};
struct LBBatch {
    LBEntry e[LB_ENTRIES];
    int stat_first[LB_ENTRIES + 1];        // first block of entry i in the statistics grid = its first partial
    int tile_first[LB_ENTRIES + 1];        // ... in the grids of lb_local and lb_merge
    int chunk_first[LB_ENTRIES + 1];       // ... of lb_flatten and lb_rank = its first chunk count
    int strip_first[LB_ENTRIES + 1];       // ... of lb_relabel
    int n, mode, max_components;
    double thr_value;
};
static_assert(sizeof(LBBatch) <= 4096, "the descriptor travels as a kernel argument");

// block-wide max for LNT threads; valid in thread 0.  Contains barriers.
__device__ __forceinline__ double lb_block_max(double mx, double* smax /* >= LNT / 64 */) {
    mx = wave_reduce_max(mx);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) smax[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 1; k < LNT / 64; ++k) mx = smax[k] > mx ? smax[k] : mx;
    return mx;
}

// ---- 1. sum and max of every LB_STAT pixels of an entry's channel ----------------------------------------------------
template <typename T>
__global__ __launch_bounds__(LNT) void lb_stats(const LBBatch b, double* __restrict__ partial) {
    __shared__ double smem[17];
    __shared__ double smax[LNT / 64];
    const int entry = eb_entry_of(b.stat_first, b.n, blockIdx.x);
    const LBEntry& d = b.e[entry];
    const int hw = d.h * d.w, first = (blockIdx.x - b.stat_first[entry]) * LB_STAT;
    const T* x = (const T*)d.x + d.channel;
    double sum = 0.0, mx = -INFINITY;
#pragma unroll 4
    for (int j = 0; j < LB_STAT / LNT; ++j) {                  // (first + LB_STAT stays below 2^31: hw <= INT32_MAX - LCHUNK - LB_STAT)
        const int i = first + j * LNT + threadIdx.x;
        if (i < hw) {
            const double v = (double)x[(size_t)i * d.c];
            sum += v;
            mx = v > mx ? v : mx;
        }
    }
    sum = block_reduce_sum(sum, smem);
    mx = lb_block_max(mx, smax);
    if (threadIdx.x == 0) {
        partial[2 * (size_t)blockIdx.x] = sum;
        partial[2 * (size_t)blockIdx.x + 1] = mx;
    }
}

// ---- 2. threshold of the entry, tile-local union-find ------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(LNT) void lb_local(const LBBatch b, const double* __restrict__ partial) {
    __shared__ int L[LTH * LTW];
    __shared__ double smem[17];
    __shared__ double smax[LNT / 64];
    __shared__ double s_thr;
    const int entry = eb_entry_of(b.tile_first, b.n, blockIdx.x);
    const LBEntry& d = b.e[entry];
    const int h = d.h, w = d.w, c = d.c;
    double thr = b.thr_value;
    if (b.mode != UOCR_THRESH_VALUE) {
        // the entry's threshold from its partials: the same order in every block of the entry and in every run
        const int p0 = b.stat_first[entry], np = b.stat_first[entry + 1] - p0;
        double sum = 0.0, mx = -INFINITY;
        for (int i = threadIdx.x; i < np; i += LNT) {
            sum += partial[2 * (size_t)(p0 + i)];
            const double m = partial[2 * (size_t)(p0 + i) + 1];
            mx = m > mx ? m : mx;
        }
        sum = block_reduce_sum(sum, smem);
        mx = lb_block_max(mx, smax);
        if (threadIdx.x == 0) {
            const double mean = sum / ((double)h * (double)w);
            s_thr = b.mode == UOCR_THRESH_MEAN ? mean : 0.5 * (mean + mx);
        }
        __syncthreads();
        thr = s_thr;
    }
    const int tiles_x = (w + LTW - 1) / LTW, tile = blockIdx.x - b.tile_first[entry];
    const T* x = (const T*)d.x + d.channel;
    label_local_tile([&](int gy, int gx) { return (double)x[((size_t)gy * w + gx) * c] > thr; }, h, w, tile % tiles_x,
                     tile / tiles_x, L, d.plane);
}

// ---- 3. unions across tile borders ----------------------------------------------------------------------------------
__global__ __launch_bounds__(LNT) void lb_merge(const LBBatch b) {
    const int entry = eb_entry_of(b.tile_first, b.n, blockIdx.x);
    const LBEntry& d = b.e[entry];
    const int tiles_x = (d.w + LTW - 1) / LTW, tile = blockIdx.x - b.tile_first[entry];
    label_merge_tile(d.h, d.w, tile % tiles_x, tile / tiles_x, d.plane);
}

// ---- 4. flatten + roots per chunk ----------------------------------------------------------------------------------
__global__ __launch_bounds__(LNT) void lb_flatten(const LBBatch b, int* __restrict__ root, int* __restrict__ chunk_count) {
    __shared__ int smem[LNT / 64 + 1];
    const int entry = eb_entry_of(b.chunk_first, b.n, blockIdx.x);
    const LBEntry& d = b.e[entry];
    const int total = label_flatten_chunk(d.h * d.w, blockIdx.x - b.chunk_first[entry], d.plane, root + d.root_off, smem);
    if (threadIdx.x == 0) chunk_count[blockIdx.x] = total;
}

// ---- 5. scan of the chunk counts, one block per entry ------------------------------------------------------------------
__global__ __launch_bounds__(LNT) void lb_scan(const LBBatch b, int* __restrict__ chunk_count, int* __restrict__ count) {
    __shared__ int smem[LNT / 64 + 1];
    const int entry = blockIdx.x, c0 = b.chunk_first[entry];
    const int total = label_scan_image(b.chunk_first[entry + 1] - c0, chunk_count + c0, smem);
    if (threadIdx.x == 0) count[entry] = total;
}

// ---- 6. rank of every root ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LNT) void lb_rank(const LBBatch b, const int* __restrict__ root,
                                               const int* __restrict__ chunk_offset, long long* __restrict__ table) {
    __shared__ int smem[LNT / 64 + 1];
    const int entry = eb_entry_of(b.chunk_first, b.n, blockIdx.x);
    const LBEntry& d = b.e[entry];
    label_rank_chunk(d.h * d.w, blockIdx.x - b.chunk_first[entry], chunk_offset[blockIdx.x], root + d.root_off, d.plane,
                     table + (size_t)entry * b.max_components * 8, b.max_components, smem);
}

// ---- 7. final labels + table: one wave per strip of 64 columns x LROWS rows ---------------------------------------------
__global__ __launch_bounds__(LNT) void lb_relabel(const LBBatch b, const int* __restrict__ root, long long* __restrict__ table) {
    const int entry = eb_entry_of(b.strip_first, b.n, blockIdx.x);
    const LBEntry& d = b.e[entry];
    const int strips_x = (d.w + 63) / 64, strips_y = (d.h + LROWS - 1) / LROWS;
    const int wave = (blockIdx.x - b.strip_first[entry]) * (LNT / 64) + (threadIdx.x >> 6);
    if (wave >= strips_x * strips_y) return;                        // (an entry's strips are rounded up to whole blocks)
    label_relabel_strip(d.h, d.w, wave % strips_x, wave / strips_x, root + d.root_off, d.plane,
                        table + (size_t)entry * b.max_components * 8, b.max_components);
}

inline size_t lb_round16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

}  // namespace

extern "C" {

int uocr_label_batch(uocr_ctx* ctx, int dtype, int n_entries, const void* const* x, const int* h, const int* w, const int* c,
                     const int* channel, int thresh_mode, double thresh_value, int* const* labels, long long* table,
                     int max_components, int* count) {
    UOCR_CHECK_CTX(ctx);
    UOCR_REQUIRE(ctx, n_entries >= 0);
    if (n_entries == 0) return UOCR_OK;                            // nothing to do, whatever else was passed
    UOCR_REQUIRE(ctx, x && h && w && c && channel && table && count);
    UOCR_REQUIRE(ctx, max_components >= 0);
    UOCR_REQUIRE(ctx, thresh_mode == UOCR_THRESH_MEAN || thresh_mode == UOCR_THRESH_MEAN_MAX ||
                          thresh_mode == UOCR_THRESH_VALUE);
    const size_t elem = eb_storage_elem(ctx, dtype);
    if (!elem) return UOCR_ERR_DTYPE;
    UOCR_REQUIRE(ctx, reinterpret_cast<uintptr_t>(table) % sizeof(long long) == 0);
    UOCR_REQUIRE(ctx, reinterpret_cast<uintptr_t>(count) % sizeof(int) == 0);
    const auto pixels = [&](int i) { return (long long)h[i] * w[i]; };
    const auto stat_blocks = [&](int i) { return (pixels(i) + LB_STAT - 1) / LB_STAT; };
    const auto tile_blocks = [&](int i) { return (long long)((w[i] + LTW - 1) / LTW) * ((h[i] + LTH - 1) / LTH); };
    const auto chunk_blocks = [&](int i) { return (pixels(i) + LCHUNK - 1) / LCHUNK; };
    const auto strip_blocks = [&](int i) {
        return ((long long)((w[i] + 63) / 64) * ((h[i] + LROWS - 1) / LROWS) + LNT / 64 - 1) / (LNT / 64);
    };
    // workspace of a group: root plane | planes of the entries without labels | chunk counts | statistics partials
    struct Need { size_t off_plane, off_counts, off_partial, bytes; };
    const auto need_of = [&](int first, int n) {
        size_t all = 0, own = 0, chunks = 0, stats = 0;
        for (int i = first; i < first + n; ++i) {
            all += (size_t)pixels(i);
            if (!labels || !labels[i]) own += (size_t)pixels(i);
            chunks += (size_t)chunk_blocks(i), stats += (size_t)stat_blocks(i);
        }
        Need need;
        need.off_plane = lb_round16(all * sizeof(int));
        need.off_counts = need.off_plane + lb_round16(own * sizeof(int));
        need.off_partial = need.off_counts + lb_round16(chunks * sizeof(int));
        need.bytes = need.off_partial + 2 * stats * sizeof(double);
        return need;
    };
    // everything is checked before the first launch: an error leaves every output as it was
    size_t workspace = 0;
    for (int first = 0; first < n_entries; first += LB_ENTRIES) {
        const int n = eb_group_size(n_entries, first, LB_ENTRIES);
        for (int i = first; i < first + n; ++i) {
            UOCR_REQUIRE(ctx, x[i] != nullptr);
            UOCR_REQUIRE(ctx, h[i] >= 1 && w[i] >= 1 && c[i] >= 1);
            UOCR_REQUIRE(ctx, channel[i] >= 0 && channel[i] < c[i]);
            UOCR_REQUIRE(ctx, reinterpret_cast<uintptr_t>(x[i]) % elem == 0);
            UOCR_REQUIRE(ctx, !labels || reinterpret_cast<uintptr_t>(labels[i]) % sizeof(int) == 0);
            if (pixels(i) > (long long)INT32_MAX - LCHUNK - LB_STAT)
                UOCR_FAIL(ctx, UOCR_ERR_UNSUPPORTED, "entry %d of %d x %d pixels: linear indices must fit int32", i, h[i], w[i]);
        }
        if (eb_group_blocks(first, n, stat_blocks) < 0 || eb_group_blocks(first, n, tile_blocks) < 0 ||
            eb_group_blocks(first, n, chunk_blocks) < 0 || eb_group_blocks(first, n, strip_blocks) < 0)
            UOCR_FAIL(ctx, UOCR_ERR_UNSUPPORTED, "entries %d..: too many blocks for one grid", first);
        const size_t bytes = need_of(first, n).bytes;
        workspace = bytes > workspace ? bytes : workspace;
    }
    if (int rc = uocr_need_workspace(ctx, workspace)) return rc;
    if (max_components > 0)   // rows past an entry's count read zero
        UOCR_HIP(ctx, hipMemsetAsync(table, 0, (size_t)n_entries * max_components * 8 * sizeof(long long), ctx->stream));
    char* ws = (char*)ctx->workspace;
    int launches = 0;
    for (int first = 0; first < n_entries; first += LB_ENTRIES) {   // the groups of a call follow each other on the stream
        LBBatch b;
        memset(&b, 0, sizeof(b));
        b.n = eb_group_size(n_entries, first, LB_ENTRIES);
        b.mode = thresh_mode, b.max_components = max_components, b.thr_value = thresh_value;
        eb_block_first(first, b.n, b.stat_first, stat_blocks);
        eb_block_first(first, b.n, b.tile_first, tile_blocks);
        eb_block_first(first, b.n, b.chunk_first, chunk_blocks);
        eb_block_first(first, b.n, b.strip_first, strip_blocks);
        const Need need = need_of(first, b.n);
        int* root = (int*)ws;
        int* own_plane = (int*)(ws + need.off_plane);
        int* chunk_count = (int*)(ws + need.off_counts);
        double* partial = (double*)(ws + need.off_partial);
        long long root_off = 0, own_off = 0;
        bool merge = false;
        for (int i = 0; i < b.n; ++i) {
            const int s = first + i;
            LBEntry& d = b.e[i];
            d.x = x[s], d.h = h[s], d.w = w[s], d.c = c[s], d.channel = channel[s];
            d.root_off = root_off;
            root_off += pixels(s);
            if (labels && labels[s]) {
                d.plane = labels[s];
            } else {
                d.plane = own_plane + own_off;
                own_off += pixels(s);
            }
            merge = merge || tile_blocks(s) > 1;
        }
        long long* group_table = table + (size_t)first * max_components * 8;
        UOCR_DISPATCH_STORAGE(ctx, dtype, {
            if (thresh_mode != UOCR_THRESH_VALUE) {
                hipLaunchKernelGGL(lb_stats<T>, dim3((unsigned)b.stat_first[b.n]), dim3(LNT), 0, ctx->stream, b, partial);
                UOCR_LAUNCH_CHECK(ctx);
                ++launches;
            }
            hipLaunchKernelGGL(lb_local<T>, dim3((unsigned)b.tile_first[b.n]), dim3(LNT), 0, ctx->stream, b,
                               (const double*)partial);
            UOCR_LAUNCH_CHECK(ctx);
            ++launches;
        });
        if (merge) {
            hipLaunchKernelGGL(lb_merge, dim3((unsigned)b.tile_first[b.n]), dim3(LNT), 0, ctx->stream, b);
            UOCR_LAUNCH_CHECK(ctx);
            ++launches;
        }
        hipLaunchKernelGGL(lb_flatten, dim3((unsigned)b.chunk_first[b.n]), dim3(LNT), 0, ctx->stream, b, root, chunk_count);
        UOCR_LAUNCH_CHECK(ctx);
        hipLaunchKernelGGL(lb_scan, dim3((unsigned)b.n), dim3(LNT), 0, ctx->stream, b, chunk_count, count + first);
        UOCR_LAUNCH_CHECK(ctx);
        hipLaunchKernelGGL(lb_rank, dim3((unsigned)b.chunk_first[b.n]), dim3(LNT), 0, ctx->stream, b, (const int*)root,
                           (const int*)chunk_count, group_table);
        UOCR_LAUNCH_CHECK(ctx);
        hipLaunchKernelGGL(lb_relabel, dim3((unsigned)b.strip_first[b.n]), dim3(LNT), 0, ctx->stream, b, (const int*)root,
                           group_table);
        UOCR_LAUNCH_CHECK(ctx);
        launches += 4;
    }
    uocr_note(ctx, UOCR_REPORT_LABEL_BATCH, LTH, LTW, LB_ENTRIES, launches);
    return UOCR_OK;
}

int uocr_ctx_last_label_batch(uocr_ctx* ctx, int* tile_h, int* tile_w, int* entries_per_launch, int* launches) {
    return uocr_report_read(ctx, UOCR_REPORT_LABEL_BATCH, tile_h, tile_w, entries_per_launch, launches);
}

}  // extern "C"
