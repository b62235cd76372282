// Lines of a page side by side in one strip, and the columns between them set back to zero: what lets the Char net take
// all lines of a page in ONE forward pass (my_model/model.py: PackedLinesComponent; the reference runs one pass per line,
// nn/model_system.py:150-154).  Both calls work on a strip (1, h, strip_w, c) whose columns are cut into SEGMENTS
// [x0[i], x0[i] + w[i]), ascending and disjoint, with GAPS before, between and after them.
//   pack       segment i of the strip = line i: (1, h, w[i], c), every gap = +0.0; every element of the strip is written
//   zero gaps  every gap = +0.0, written and not multiplied (a NaN there becomes 0); no element of a segment is touched
// Neither does arithmetic: a copied element keeps its bits in every dtype.  An ENTRY is a column range [lo, lo + span) of
// the strip, its h rows each one contiguous run of the strip: for pack, line i with the gap behind it (line 0 also with
// the gap in front), for zero gaps one gap -- so the work of zero gaps is proportional to the gaps, not to the tensor.
// A block takes PL_CHUNK elements of an entry at most: whole rows while a row is shorter than that, one piece of one row
// otherwise; a row (or piece) is written with 16-byte stores between a scalar head and tail, because a row of the strip
// starts wherever x0 and c put it.  Short rows go one to a wave, long ones to the whole block.  All entries of a call
// travel together, PL_ENTRIES per launch, in a by-value kernel argument (no device allocation, no copy, no host
// synchronisation: asynchronous and capturable).  No atomics, no workspace.
#include "entry_batch.h"

namespace {

constexpr int PL_NT = 256;          // threads per block
constexpr int PL_ENTRIES = 128;     // entries per launch (the descriptor is a kernel argument: 4 KB at most)
constexpr int PL_CHUNK = 4096;      // elements of an entry per block, at most

struct PLEntry {
    const void* src;                // pack: element (0, 0, 0) of the line, rows of copy_n elements; zero gaps: unused
    int lo, span;                   // the entry's elements [lo, lo + span) of every strip row
    int copy_lo, copy_n;            // of these, [copy_lo, copy_lo + copy_n) are the line's row; the others are zero
};
struct PLBatch {
    PLEntry entry[PL_ENTRIES];
    int block_first[PL_ENTRIES + 1];   // first block of entry i in the grid
    void* strip;
    int h, pitch;                   // rows of the strip, elements per strip row
    int n;
};
static_assert(sizeof(PLBatch) <= 4096, "the descriptor travels as a kernel argument");

// rows of an entry one block takes, and pieces a row is cut into (one of the two is 1)
__host__ __device__ __forceinline__ int pl_pieces(int span) { return (span + PL_CHUNK - 1) / PL_CHUNK; }
__host__ __device__ __forceinline__ int pl_rows(int span) { return span >= PL_CHUNK ? 1 : PL_CHUNK / span; }
inline long long pl_blocks(int h, int span) {
    return span < 1 ? 0 : (long long)((h + pl_rows(span) - 1) / pl_rows(span)) * pl_pieces(span);
}

// COUNT consecutive elements of row `row` from element q of the entry on: all loads are issued before the first is used
template <typename T, bool COPY, int COUNT>
__device__ __forceinline__ void pl_fetch(const PLEntry& e, int row, int q, T* v) {
    if constexpr (COPY) {
        const T* src = (const T*)e.src + (size_t)row * e.copy_n;
        bool in[COUNT];
#pragma unroll
        for (int k = 0; k < COUNT; ++k) {
            const unsigned at = (unsigned)(q + k - e.copy_lo);
            in[k] = at < (unsigned)e.copy_n;
            v[k] = src[in[k] ? at : 0u];                           // (a clamped address: no branch around the load)
        }
#pragma unroll
        for (int k = 0; k < COUNT; ++k) v[k] = in[k] ? v[k] : (T)0.0f;
    } else {
#pragma unroll
        for (int k = 0; k < COUNT; ++k) v[k] = (T)0.0f;
    }
}

template <typename T, bool COPY>
__global__ __launch_bounds__(PL_NT) void pack_rows(const PLBatch b) {
    using V = typename EBVec<T>::type;
    constexpr int VEC = EBVec<T>::N;
    const int i = eb_entry_of(b.block_first, b.n, blockIdx.x);
    const PLEntry& e = b.entry[i];
    const int local = blockIdx.x - b.block_first[i];
    const int pieces = pl_pieces(e.span), rows = pl_rows(e.span);
    const int piece = local % pieces;
    const int row_first = (local / pieces) * rows;
    const int row_end = row_first + rows < b.h ? row_first + rows : b.h;
    const int first = piece * PL_CHUNK;
    const int n = e.span - first < PL_CHUNK ? e.span - first : PL_CHUNK;
    // a wave per row where the block holds at least four rows, the whole block per row otherwise (block-uniform)
    const int team = row_end - row_first >= PL_NT / 64 ? 64 : PL_NT;
    const int lane = threadIdx.x % team;
    for (int row = row_first + threadIdx.x / team; row < row_end; row += PL_NT / team) {
        T* out = (T*)b.strip + (size_t)row * b.pitch + e.lo + first;
        const auto [head, nvec, tail] = eb_split(out, n);
        if (lane < head) {
            T v;
            pl_fetch<T, COPY, 1>(e, row, first + lane, &v);
            out[lane] = v;
        }
        V* ov = reinterpret_cast<V*>(out + head);
        for (int k = lane; k < nvec; k += team) {
            T v[VEC];
            pl_fetch<T, COPY, VEC>(e, row, first + head + k * VEC, v);
            V packed;
#pragma unroll
            for (int j = 0; j < VEC; ++j) packed[j] = v[j];
            ov[k] = packed;
        }
        if (lane < tail) {
            const int at = head + nvec * VEC + lane;
            T v;
            pl_fetch<T, COPY, 1>(e, row, first + at, &v);
            out[at] = v;
        }
    }
}

// what both calls ask of a strip and its segments; nothing has been launched when this fails
int pl_check(uocr_ctx* ctx, int dtype, int n_lines, const int* x0, const int* w, const void* strip, int h, int strip_w, int c,
             size_t* elem) {
    UOCR_REQUIRE(ctx, x0 && w && strip);
    *elem = eb_storage_elem(ctx, dtype);
    if (!*elem) return UOCR_ERR_DTYPE;
    UOCR_REQUIRE(ctx, h >= 1 && strip_w >= 1 && c >= 1);
    UOCR_REQUIRE(ctx, reinterpret_cast<uintptr_t>(strip) % *elem == 0);
    long long end = 0;                                             // where the segment before this one ends
    for (int i = 0; i < n_lines; ++i) {
        UOCR_REQUIRE(ctx, w[i] >= 1);
        UOCR_REQUIRE(ctx, x0[i] >= end);                           // ascending, not overlapping, not before column 0
        end = (long long)x0[i] + w[i];
        UOCR_REQUIRE(ctx, end <= strip_w);
    }
    if ((long long)strip_w * c > INT32_MAX)
        UOCR_FAIL(ctx, UOCR_ERR_UNSUPPORTED, "a strip row of %d x %d elements is too long", strip_w, c);
    return UOCR_OK;
}

// the entries [lo, hi) (columns; an empty one has no blocks) of a call in groups of PL_ENTRIES: checked, then launched
template <bool COPY, typename Entry>
int pl_launch(uocr_ctx* ctx, int dtype, int n_entries, void* strip, int h, int strip_w, int c, Entry entry) {
    const auto blocks = [&](int i) { return pl_blocks(h, entry(i).span); };
    for (int first = 0; first < n_entries; first += PL_ENTRIES)
        if (eb_group_blocks(first, eb_group_size(n_entries, first, PL_ENTRIES), blocks) < 0)
            UOCR_FAIL(ctx, UOCR_ERR_UNSUPPORTED, "entries %d..: too many blocks for one grid", first);
    int launches = 0;
    for (int first = 0; first < n_entries; first += PL_ENTRIES) {
        PLBatch b;
        memset(&b, 0, sizeof(b));
        b.n = eb_group_size(n_entries, first, PL_ENTRIES);
        b.strip = strip, b.h = h, b.pitch = strip_w * c;
        eb_block_first(first, b.n, b.block_first, blocks);
        for (int i = 0; i < b.n; ++i) b.entry[i] = entry(first + i);
        if (b.block_first[b.n] == 0) continue;                     // (gaps without columns)
        UOCR_DISPATCH_STORAGE(ctx, dtype, {
            hipLaunchKernelGGL((pack_rows<T, COPY>), dim3((unsigned)b.block_first[b.n]), dim3(PL_NT), 0, ctx->stream, b);
            UOCR_LAUNCH_CHECK(ctx);
        });
        launches += 1;
    }
    uocr_note(ctx, UOCR_REPORT_PACK_LINES, PL_CHUNK, PL_ENTRIES, launches);
    return UOCR_OK;
}

}  // namespace

extern "C" {

int uocr_pack_lines(uocr_ctx* ctx, int dtype, int n_lines, const void* const* src, const int* w, int h, int c, const int* x0,
                    void* strip, int strip_w) {
    UOCR_CHECK_CTX(ctx);
    UOCR_REQUIRE(ctx, n_lines >= 0);
    if (n_lines == 0) return UOCR_OK;                              // nothing to do, whatever else was passed
    UOCR_REQUIRE(ctx, src);
    size_t elem = 0;
    const int rc = pl_check(ctx, dtype, n_lines, x0, w, strip, h, strip_w, c, &elem);
    if (rc != UOCR_OK) return rc;
    for (int i = 0; i < n_lines; ++i) UOCR_REQUIRE(ctx, src[i] && reinterpret_cast<uintptr_t>(src[i]) % elem == 0);
    // entry i: line i and the gap behind it; entry 0 also takes the gap in front of line 0
    return pl_launch<true>(ctx, dtype, n_lines, strip, h, strip_w, c, [&](int i) {
        const int lo = i == 0 ? 0 : x0[i], hi = i + 1 < n_lines ? x0[i + 1] : strip_w;
        return PLEntry{src[i], lo * c, (hi - lo) * c, (x0[i] - lo) * c, w[i] * c};
    });
}

int uocr_zero_gaps(uocr_ctx* ctx, int dtype, void* x, int h, int strip_w, int c, int n_lines, const int* x0, const int* w) {
    UOCR_CHECK_CTX(ctx);
    UOCR_REQUIRE(ctx, n_lines >= 0);
    if (n_lines == 0) return UOCR_OK;                              // nothing to do, whatever else was passed
    size_t elem = 0;
    const int rc = pl_check(ctx, dtype, n_lines, x0, w, x, h, strip_w, c, &elem);
    if (rc != UOCR_OK) return rc;
    // entry i: the gap in front of line i; entry n_lines: the gap behind the last line
    return pl_launch<false>(ctx, dtype, n_lines + 1, x, h, strip_w, c, [&](int i) {
        const int lo = i == 0 ? 0 : x0[i - 1] + w[i - 1], hi = i < n_lines ? x0[i] : strip_w;
        return PLEntry{nullptr, lo * c, (hi - lo) * c, 0, 0};
    });
}

int uocr_ctx_last_pack_lines(uocr_ctx* ctx, int* elements_per_block, int* entries_per_launch, int* launches) {
    return uocr_report_read(ctx, UOCR_REPORT_PACK_LINES, elements_per_block, entries_per_launch, launches);
}

}  // extern "C"
