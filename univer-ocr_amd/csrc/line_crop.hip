// Line crops: the device form of the gather half of the reference's LineCrop stage (interpreter/interpreter.py:504-523
// CropRotateAndZoomLines._func2, driven by my_model/model.py:595-612).  Per (array, line) pair -- an ENTRY:
//   crop    the box [y0, y0 + box_h) x [x0, x0 + box_w) of a (1, src_h, src_w, c) array, nothing masked (:506)
//   rotate  by quarter_turns * 90 degrees: ndimage.rotate(.., axes=(2, 1), order=1, reshape=True) (:192) of 90 / 180 /
//           270 degrees equals np.rot90(.., quarter_turns, axes=(1, 2)) bit for bit -- a permutation, no arithmetic
//   zoom    ndimage.zoom(.., order=0) (:514) to zoom_h x zoom_w: a gather.  Per axis z = (n_in - 1) / (n_out - 1) in
//           float64 (n_out = 1 reads index 0); output index j reads floor(j * z + 0.5), product and sum each rounded on
//           their own; where j * z comes out above n_in - 1 (only ever at the last index) scipy's constant mode writes 0
//   pad     zero columns from zoom_w up to out_w (:516-521)
// All four are ONE index map from an output element to a source element or zero, so results are equal to the
// reference's in every dtype.  The output of an entry is one flat contiguous range of zoom_h * out_w * c elements; a
// block writes LC_CHUNK consecutive elements of it -- gathered values, artefact zeros and padding alike -- with 16-byte
// stores between a scalar head and tail (c = 9 gives no per-pixel alignment).  Reads are a direct gather: consecutive
// outputs of an upright line read ascending addresses of one source row, those of a quarter-turned line walk down a
// source column.  All entries of a call travel together, LC_ENTRIES per launch, their pointers, sizes and zoom ratios in
// a by-value kernel argument (no device allocation, no copy, no host synchronisation: asynchronous and capturable).
// No atomics, no workspace.
// hipcc-flags: -ffp-contract=off
#include "entry_batch.h"

namespace {

constexpr int LC_NT = 256;          // threads per block
constexpr int LC_ENTRIES = 48;      // entries per launch (the descriptor is a kernel argument: 4 KB at most)
constexpr int LC_CHUNK = 4096;      // output elements per block

struct LCEntry {
    const void* src;                // element (y0, x0, 0) of the source array: the box's first element
    void* out;
    double zy, zx;                  // (n_in - 1) / (n_out - 1) of the rotated box's rows and columns; 0 when n_out <= 1
    int pitch, c;                   // source row pitch in pixels, channels
    int box_h, box_w, turns;
    int rot_h, rot_w;               // the rotated box: (box_w, box_h) for an odd number of turns
    int zoom_h, zoom_w, out_w;
};
struct LCBatch {
    LCEntry entry[LC_ENTRIES];
    int block_first[LC_ENTRIES + 1];   // first block of entry i in the grid
    int n;
};
static_assert(sizeof(LCBatch) <= 4096, "the descriptor travels as a kernel argument");

// ndimage.zoom at order 0: the input index output index j reads, or -1 where scipy writes its constant 0
__device__ __forceinline__ int lc_zoom_index(int j, double z, int n_in) {
    const double t = __dmul_rn((double)j, z);
    if (t > (double)(n_in - 1)) return -1;
    return (int)__dadd_rn(t, 0.5);              // (t >= 0: the conversion is the floor; at most n_in - 1)
}

// element (row, col, ch) of the entry's output as an offset from the box's first element, or -1 for a zero
__device__ __forceinline__ long long lc_source(const LCEntry& e, int sy, int col, int ch) {
    if (sy < 0 || col >= e.zoom_w) return -1;
    const int sx = lc_zoom_index(col, e.zx, e.rot_w);
    if (sx < 0) return -1;
    // np.rot90(a, k, axes=(1, 2)): k = 1 r[i, j] = a[j, w - 1 - i]; k = 2 r[i, j] = a[h - 1 - i, w - 1 - j]; k = 3 r[i, j] = a[h - 1 - j, i]
    int y, x;
    switch (e.turns) {
        case 0: y = sy, x = sx; break;
        case 1: y = sx, x = e.box_w - 1 - sy; break;
        case 2: y = e.box_h - 1 - sy, x = e.box_w - 1 - sx; break;
        default: y = e.box_h - 1 - sx, x = sy; break;
    }
    return ((long long)y * e.pitch + x) * e.c + ch;
}

// COUNT consecutive output elements from flat index q of the entry on: all loads are issued before the first is used
template <typename T, int COUNT>
__device__ __forceinline__ void lc_gather(const LCEntry& e, size_t q, T* v) {
    const size_t span = (size_t)e.out_w * e.c;
    int row = (int)(q / span);
    const unsigned r = (unsigned)(q - (size_t)row * span);
    int col = (int)(r / (unsigned)e.c), ch = (int)(r - (unsigned)col * (unsigned)e.c);
    int sy = lc_zoom_index(row, e.zy, e.rot_h);
    long long off[COUNT];
#pragma unroll
    for (int k = 0; k < COUNT; ++k) {
        off[k] = lc_source(e, sy, col, ch);
        if (++ch == e.c) {
            ch = 0;
            if (++col == e.out_w) {
                col = 0;
                sy = lc_zoom_index(++row, e.zy, e.rot_h);        // (past the entry's last element: never stored)
            }
        }
    }
    const T* src = (const T*)e.src;
#pragma unroll
    for (int k = 0; k < COUNT; ++k) v[k] = src[off[k] < 0 ? 0 : off[k]];   // (a clamped address: no branch around the load)
#pragma unroll
    for (int k = 0; k < COUNT; ++k) v[k] = off[k] < 0 ? (T)0.0f : v[k];
}

template <typename T>
__global__ __launch_bounds__(LC_NT) void line_crop_gather(const LCBatch b) {
    using V = typename EBVec<T>::type;
    constexpr int VEC = EBVec<T>::N;
    const int tid = threadIdx.x;
    const int i = eb_entry_of(b.block_first, b.n, blockIdx.x);
    const LCEntry& e = b.entry[i];
    const size_t count = (size_t)e.zoom_h * e.out_w * e.c;
    const size_t first = (size_t)(blockIdx.x - b.block_first[i]) * LC_CHUNK;
    const int n = (int)(count - first < (size_t)LC_CHUNK ? count - first : (size_t)LC_CHUNK);
    T* out = (T*)e.out + first;
    const auto [head, nvec, tail] = eb_split(out, n);
    if (tid < head) {
        T v;
        lc_gather<T, 1>(e, first + tid, &v);
        out[tid] = v;
    }
    V* ov = reinterpret_cast<V*>(out + head);
    for (int k = tid; k < nvec; k += LC_NT) {
        T v[VEC];
        lc_gather<T, VEC>(e, first + head + (size_t)k * VEC, v);
        V packed;
#pragma unroll
        for (int j = 0; j < VEC; ++j) packed[j] = v[j];
        ov[k] = packed;
    }
    if (tid < tail) {
        const int at = head + nvec * VEC + tid;
        T v;
        lc_gather<T, 1>(e, first + at, &v);
        out[at] = v;
    }
}

}  // namespace

extern "C" {

int uocr_line_crop(uocr_ctx* ctx, int dtype, int n_entries, const void* const* src, const int* src_h, const int* src_w,
                   const int* c, const int* y0, const int* x0, const int* box_h, const int* box_w, const int* quarter_turns,
                   const int* zoom_h, const int* zoom_w, void* const* out, const int* out_w) {
    UOCR_CHECK_CTX(ctx);
    UOCR_REQUIRE(ctx, n_entries >= 0);
    if (n_entries == 0) return UOCR_OK;                            // nothing to do, whatever else was passed
    UOCR_REQUIRE(ctx, src && src_h && src_w && c && y0 && x0 && box_h && box_w && quarter_turns && zoom_h && zoom_w && out && out_w);
    const size_t elem = eb_storage_elem(ctx, dtype);
    if (!elem) return UOCR_ERR_DTYPE;
    const auto blocks = [&](int i) { return ((long long)zoom_h[i] * out_w[i] * c[i] + LC_CHUNK - 1) / LC_CHUNK; };
    // everything is checked before the first launch: an error leaves every output as it was
    for (int first = 0; first < n_entries; first += LC_ENTRIES) {
        const int count = eb_group_size(n_entries, first, LC_ENTRIES);
        for (int i = first; i < first + count; ++i) {
            UOCR_REQUIRE(ctx, src[i] && (out[i] || out_w[i] == 0));   // (an output without elements has no address)
            UOCR_REQUIRE(ctx, (reinterpret_cast<uintptr_t>(src[i]) | reinterpret_cast<uintptr_t>(out[i])) % elem == 0);
            UOCR_REQUIRE(ctx, c[i] >= 1 && src_h[i] >= 1 && src_w[i] >= 1);
            UOCR_REQUIRE(ctx, y0[i] >= 0 && x0[i] >= 0 && box_h[i] >= 1 && box_w[i] >= 1);
            UOCR_REQUIRE(ctx, (long long)y0[i] + box_h[i] <= src_h[i] && (long long)x0[i] + box_w[i] <= src_w[i]);
            UOCR_REQUIRE(ctx, quarter_turns[i] >= 0 && quarter_turns[i] <= 3);
            UOCR_REQUIRE(ctx, zoom_h[i] >= 1 && zoom_w[i] >= 0 && out_w[i] >= zoom_w[i]);
            const long long span = (long long)out_w[i] * c[i];
            if (span > INT32_MAX || span * zoom_h[i] / LC_CHUNK > INT32_MAX)
                UOCR_FAIL(ctx, UOCR_ERR_UNSUPPORTED, "entry %d: %d x %d x %d is too large an output", i, zoom_h[i], out_w[i], c[i]);
        }
        if (eb_group_blocks(first, count, blocks) < 0)
            UOCR_FAIL(ctx, UOCR_ERR_UNSUPPORTED, "entries %d..: too many blocks for one grid", first);
    }
    int launches = 0;
    for (int first = 0; first < n_entries; first += LC_ENTRIES) {
        LCBatch b;
        memset(&b, 0, sizeof(b));
        b.n = eb_group_size(n_entries, first, LC_ENTRIES);
        eb_block_first(first, b.n, b.block_first, blocks);
        for (int i = 0; i < b.n; ++i) {
            const int s = first + i;
            LCEntry& e = b.entry[i];
            e.src = (const char*)src[s] + (((size_t)y0[s] * src_w[s] + x0[s]) * c[s]) * elem;
            e.out = out[s];
            e.pitch = src_w[s], e.c = c[s];
            e.box_h = box_h[s], e.box_w = box_w[s], e.turns = quarter_turns[s];
            e.rot_h = e.turns & 1 ? e.box_w : e.box_h, e.rot_w = e.turns & 1 ? e.box_h : e.box_w;
            e.zoom_h = zoom_h[s], e.zoom_w = zoom_w[s], e.out_w = out_w[s];
            // scipy's zoom ratios, one float64 division each (ndimage.zoom: ratio 1 where the output has one element,
            // which reads index 0 just as ratio 0 does)
            e.zy = e.zoom_h > 1 ? (double)(e.rot_h - 1) / (double)(e.zoom_h - 1) : 0.0;
            e.zx = e.zoom_w > 1 ? (double)(e.rot_w - 1) / (double)(e.zoom_w - 1) : 0.0;
        }
        if (b.block_first[b.n] == 0) continue;                     // (outputs without elements)
        UOCR_DISPATCH_STORAGE(ctx, dtype, {
            hipLaunchKernelGGL(line_crop_gather<T>, dim3((unsigned)b.block_first[b.n]), dim3(LC_NT), 0, ctx->stream, b);
            UOCR_LAUNCH_CHECK(ctx);
        });
        launches += 1;
    }
    uocr_note(ctx, UOCR_REPORT_LINE_CROP, LC_CHUNK, 16, LC_ENTRIES, launches);
    return UOCR_OK;
}

int uocr_ctx_last_line_crop(uocr_ctx* ctx, int* elements_per_block, int* store_bytes, int* entries_per_launch, int* launches) {
    return uocr_report_read(ctx, UOCR_REPORT_LINE_CROP, elements_per_block, store_bytes, entries_per_launch, launches);
}

}  // extern "C"
