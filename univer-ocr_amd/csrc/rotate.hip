// Paragraph rotation: the device form of the rotation search and the rotated crops of the reference's ParagraphCrop stage
// (interpreter/interpreter.py:188-231 rotate_array / FindObjectHeightInRotated._func, :319-347
// CropAndRotateSingleParagraph._func).  Both kernels evaluate ndimage.rotate(.., axes=(2, 1), reshape=True,
// mode='constant', cval=0) per OUTPUT pixel; the matrix, the offset and the shape of the rotated plane come from the host,
// which computes them as scipy does in Python (nn/ops.py: rotation_geometry) -- the device never evaluates a cosine:
//   coordinate  cy = offset[0] + oy * M[0][0] + ox * M[0][1], cx = offset[1] + oy * M[1][0] + ox * M[1][1] in float64,
//               every product and every sum rounded on its own, in this order (no fused multiply-add)
//   bounds      cy outside [0, ih - 1] or cx outside [0, iw - 1] (both inclusive): the pixel is 0 at either order
//   order 0     reads (floor(cy + 0.5), floor(cx + 0.5))
//   order 1     bilinear over floor(c) and floor(c) + 1, weights 1 - t and 1 - (1 - t) with t = c - floor(c), no
//               prefilter; the four terms (value * wy) * wx are added row-major; the neighbour at index n is reachable only
//               at c == n - 1, where its weight is 0, and is not read
// rotated_extent   a PROBE asks for the half-open extent (find_objects, :230 / :341) of the set pixels of the order-0
//                  rotation of labels[box] == id.  No rotated array is written: a block takes RT_BAND output rows of one
//                  probe, a wave 64 consecutive pixels of a row at a time; it ballots, keeps its row and column range in
//                  registers, and one lane folds them into the probe's four ints with vector atomic max (the lower ends
//                  are stored as size - index, so that one zero fill initialises all four).  A second, tiny kernel turns
//                  the four into y0, y1, x0, x1.  The gathers are scattered, but a box of labels sits in L2: the kernel is
//                  bound by launch and synchronisation latency, not by bandwidth.
// rotate_crop      an ENTRY is one (array, paragraph) pair: the order-1 rotation of (image * (labels == id))[box], cut to
//                  a region of the rotated plane and centred in make_divisible_by's zero frame, one thread per output
//                  pixel looping over the channels (NHWC stores of neighbouring threads are contiguous).  Coordinates,
//                  weights and the sum are float64 for every dtype; the result is rounded once.
// rotation_search   the whole ternary search of interpreter.py:321-336 without the host: the tree of (low, high)
//                  intervals does not depend on the data, so the host tabulates cos a, sin a, cos b, sin b of every node
//                  once (nn/ops.py: search_table) and the device walks the tree.  A round is two launches: search_probe
//                  is rotated_extent for the two probes of every paragraph, with the paragraph's current NODE read from
//                  the workspace, the geometry of the rotated plane evaluated by every block for itself (rs_geometry:
//                  nn/ops.py: search_geometry bit for bit, identical in all blocks of a probe) and only the row range
//                  kept; search_decide turns the ranges into the round's two heights, moves every paragraph to a child
//                  node and clears the ranges.  The host cannot know a probe's rows and sizes the grid by their bound;
//                  blocks past the plane return.  All rounds are enqueued back to back: plain stream order, nothing spins.
// All probes / entries of a call travel together, RT_ENTRIES per launch, in a by-value kernel argument (no device
// allocation, no host synchronisation: asynchronous and capturable).  Integer atomics only: bit-identical run to run.
// hipcc-flags: -ffp-contract=off
#include "entry_batch.h"

namespace {

constexpr int RT_NT = 256;          // threads per block: 4 waves; rotate_crop: output pixels per block
constexpr int RT_BAND = 8;          // rotated_extent: output rows per block
constexpr int RT_ENTRIES = 28;      // probes / entries per launch (the descriptor is a kernel argument: 4 KB at most)

struct RTProbe {
    const int* lab;                 // label of the box's first pixel
    double m[4], off[2];
    int pitch, id, ch, cw;          // row pitch of the labels, label id, the box: the input plane of the rotation
    int out_h, out_w;               // the rotated plane
};
struct RTBatch {
    RTProbe probe[RT_ENTRIES];
    int block_first[RT_ENTRIES + 1];   // first block of probe i in the grid
    int n;
    int* extent;                    // four ints per probe of this launch
};
struct RCEntry {
    const void* src;                // element (y0, x0, 0) of the image: the box's first element
    const int* lab;
    void* out;
    double m[4], off[2];
    int pitch, c, id, ch, cw;
    int ry0, rx0, rh, rw;           // the region of the rotated plane
    int py, px, out_h, out_w;       // where the region sits in the output, the output
};
struct RCBatch {
    RCEntry entry[RT_ENTRIES];
    int block_first[RT_ENTRIES + 1];
    int n;
};
constexpr int RS_PARAGRAPHS = RT_ENTRIES / 2;   // rotation_search: paragraphs per launch, two probes each
constexpr int RS_MAX_ROUNDS = 16;
constexpr int RS_STATE = 5;                     // workspace ints per paragraph: node, then (top - first row, last row + 1) of a and b
constexpr int RS_TOP = 1 << 30;                 // lower ends are stored as RS_TOP - index: zero = nothing set
struct RSParagraph {
    const int* lab;                 // label of the box's first pixel
    int id, ch, cw;
};
struct RSBatch {
    RSParagraph par[RS_PARAGRAPHS];
    int block_first[2 * RS_PARAGRAPHS + 1];   // first block of probe i = 2 * paragraph + (0: a, 1: b)
    int n;                          // paragraphs of this launch
    int pitch, round, stride;       // row pitch of the labels; the round; ints per paragraph in the result
    const double* table;            // four doubles per node: cos a, sin a, cos b, sin b
    int* state;                     // RS_STATE ints per paragraph of this launch
    int* result;                    // per paragraph of this launch: leaf, then height_a, height_b of every round
};
static_assert(sizeof(RTBatch) <= 4096 && sizeof(RCBatch) <= 4096 && sizeof(RSBatch) <= 4096,
              "the descriptor travels as a kernel argument");

// (offset + oy * m0) + ox * m1, each operation rounded on its own
__device__ __forceinline__ double rt_coord(double off, double m0, double m1, int oy, int ox) {
    return __dadd_rn(__dadd_rn(off, __dmul_rn((double)oy, m0)), __dmul_rn((double)ox, m1));
}

// scipy's constant mode: inside means 0 <= c <= n - 1 (false for a NaN)
__device__ __forceinline__ bool rt_inside(double c, int n) { return c >= 0.0 && c <= (double)(n - 1); }

__global__ __launch_bounds__(RT_NT) void rotated_extent(const RTBatch b) {
    const int i = eb_entry_of(b.block_first, b.n, blockIdx.x);
    const RTProbe& p = b.probe[i];
    const int row0 = (blockIdx.x - b.block_first[i]) * RT_BAND;
    const int rows = p.out_h - row0 < RT_BAND ? p.out_h - row0 : RT_BAND;
    const int segs = (p.out_w + 63) / 64;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int y_lo = INT32_MAX, y_hi = -1, x_lo = INT32_MAX, x_hi = -1;      // (wave-uniform)
    for (int item = wave; item < rows * segs; item += RT_NT / 64) {
        const int oy = row0 + item / segs, seg0 = (item % segs) * 64, ox = seg0 + lane;
        bool set = false;
        if (ox < p.out_w) {
            const double cy = rt_coord(p.off[0], p.m[0], p.m[1], oy, ox), cx = rt_coord(p.off[1], p.m[2], p.m[3], oy, ox);
            if (rt_inside(cy, p.ch) && rt_inside(cx, p.cw)) {
                int sy = (int)__dadd_rn(cy, 0.5), sx = (int)__dadd_rn(cx, 0.5);   // (>= 0: the conversion is the floor)
                sy = sy < p.ch ? sy : p.ch - 1, sx = sx < p.cw ? sx : p.cw - 1;   // (never taken: n - 1 + 0.5 floors to n - 1)
                set = p.lab[(size_t)sy * p.pitch + sx] == p.id;
            }
        }
        const unsigned long long mask = __ballot(set);
        if (mask) {
            const int first = seg0 + __ffsll((long long)mask) - 1, last = seg0 + 63 - __clzll((long long)mask);
            y_lo = oy < y_lo ? oy : y_lo, y_hi = oy > y_hi ? oy : y_hi;
            x_lo = first < x_lo ? first : x_lo, x_hi = last > x_hi ? last : x_hi;
        }
    }
    if (lane == 0 && y_hi >= 0) {
        int* e = b.extent + 4 * i;                                     // zero = nothing set; lower ends as size - index
        atomicMax(e + 0, p.out_h - y_lo);
        atomicMax(e + 1, y_hi + 1);
        atomicMax(e + 2, p.out_w - x_lo);
        atomicMax(e + 3, x_hi + 1);
    }
}

__global__ void rotated_extent_finish(const RTBatch b) {
    const int i = threadIdx.x;
    if (i >= b.n) return;
    int* e = b.extent + 4 * i;
    if (e[1] > 0) e[0] = b.probe[i].out_h - e[0], e[2] = b.probe[i].out_w - e[2];    // (else all four are 0 already)
}

// nn/ops.py: search_geometry, operation by operation: the shape of the rotated plane of an ih x iw box and the offset
struct RSGeometry { double off[2]; int out_h, out_w; };
__device__ __forceinline__ double rs_ptp(double p1, double p2) {       // max - min over (0, p1, p2, p2 + p1)
    const double p3 = __dadd_rn(p2, p1);
    return __dadd_rn(fmax(fmax(0.0, p1), fmax(p2, p3)), -fmin(fmin(0.0, p1), fmin(p2, p3)));
}
__device__ __forceinline__ RSGeometry rs_geometry(int ch, int cw, double c, double s) {
    const double ih = (double)ch, iw = (double)cw, ns = -s;
    RSGeometry g;
    g.out_h = (int)__dadd_rn(rs_ptp(__dmul_rn(s, iw), __dmul_rn(c, ih)), 0.5);
    g.out_w = (int)__dadd_rn(rs_ptp(__dmul_rn(c, iw), __dmul_rn(ns, ih)), 0.5);
    const double hy = (double)(g.out_h - 1) / 2.0, hx = (double)(g.out_w - 1) / 2.0;
    g.off[0] = __dadd_rn((double)(ch - 1) / 2.0, -__dadd_rn(__dmul_rn(c, hy), __dmul_rn(s, hx)));
    g.off[1] = __dadd_rn((double)(cw - 1) / 2.0, -__dadd_rn(__dmul_rn(ns, hy), __dmul_rn(c, hx)));
    return g;
}

__global__ __launch_bounds__(RT_NT) void search_probe(const RSBatch b) {
    const int i = eb_entry_of(b.block_first, 2 * b.n, blockIdx.x);
    const RSParagraph& p = b.par[i >> 1];
    int* state = b.state + RS_STATE * (i >> 1);
    const double* t = b.table + 4 * (size_t)state[0] + 2 * (i & 1);   // (the node: below 2^round - 1 rows of the table)
    const double c = t[0], s = t[1];
    const RSGeometry g = rs_geometry(p.ch, p.cw, c, s);
    const int row0 = (blockIdx.x - b.block_first[i]) * RT_BAND;
    if (row0 >= g.out_h) return;                                       // (the grid holds the bound of out_h)
    const int rows = g.out_h - row0 < RT_BAND ? g.out_h - row0 : RT_BAND;
    const int segs = (g.out_w + 63) / 64;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int y_lo = INT32_MAX, y_hi = -1;                                   // (wave-uniform)
    for (int item = wave; item < rows * segs; item += RT_NT / 64) {
        const int oy = row0 + item / segs, ox = (item % segs) * 64 + lane;
        bool set = false;                                              // (the pixel test of rotated_extent, which stays as it is)
        if (ox < g.out_w) {
            const double cy = rt_coord(g.off[0], c, s, oy, ox), cx = rt_coord(g.off[1], -s, c, oy, ox);
            if (rt_inside(cy, p.ch) && rt_inside(cx, p.cw)) {
                int sy = (int)__dadd_rn(cy, 0.5), sx = (int)__dadd_rn(cx, 0.5);   // (>= 0: the conversion is the floor)
                sy = sy < p.ch ? sy : p.ch - 1, sx = sx < p.cw ? sx : p.cw - 1;   // (never taken: n - 1 + 0.5 floors to n - 1)
                set = p.lab[(size_t)sy * b.pitch + sx] == p.id;
            }
        }
        if (__ballot(set)) y_lo = oy < y_lo ? oy : y_lo, y_hi = oy > y_hi ? oy : y_hi;
    }
    if (lane == 0 && y_hi >= 0) {
        int* e = state + 1 + 2 * (i & 1);
        atomicMax(e + 0, RS_TOP - y_lo);
        atomicMax(e + 1, y_hi + 1);
    }
}

__global__ void search_decide(const RSBatch b) {
    const int i = threadIdx.x;
    if (i >= b.n) return;
    int* state = b.state + RS_STATE * i;
    int* result = b.result + (size_t)b.stride * i;
    const int height_a = state[2] > 0 ? state[2] - (RS_TOP - state[1]) : 0;
    const int height_b = state[4] > 0 ? state[4] - (RS_TOP - state[3]) : 0;
    result[1 + 2 * b.round] = height_a, result[2 + 2 * b.round] = height_b;
    state[0] = result[0] = 2 * state[0] + (height_a < height_b ? 1 : 2);   // (after the last round: the leaf)
    state[1] = state[2] = state[3] = state[4] = 0;
}

template <typename T>
__global__ __launch_bounds__(RT_NT) void rotate_crop(const RCBatch b) {
    const int i = eb_entry_of(b.block_first, b.n, blockIdx.x);
    const RCEntry& e = b.entry[i];
    const size_t o = (size_t)(blockIdx.x - b.block_first[i]) * RT_NT + threadIdx.x;
    if (o >= (size_t)e.out_h * e.out_w) return;
    const int oy = (int)(o / e.out_w), ox = (int)(o % e.out_w);
    const int c = e.c;
    T* out = (T*)e.out + o * c;
    const int ry = oy - e.py, rx = ox - e.px;
    bool inside = ry >= 0 && ry < e.rh && rx >= 0 && rx < e.rw;
    double cy = 0.0, cx = 0.0;
    if (inside) {
        cy = rt_coord(e.off[0], e.m[0], e.m[1], e.ry0 + ry, e.rx0 + rx);
        cx = rt_coord(e.off[1], e.m[2], e.m[3], e.ry0 + ry, e.rx0 + rx);
        inside = rt_inside(cy, e.ch) && rt_inside(cx, e.cw);
    }
    if (!inside) {
        for (int k = 0; k < c; ++k) out[k] = T(0.0f);
        return;
    }
    const double fy = floor(cy), fx = floor(cx);
    const int iy = (int)fy, ix = (int)fx;
    double wy[2], wx[2];
    wy[0] = 1.0 - (cy - fy), wy[1] = 1.0 - wy[0];
    wx[0] = 1.0 - (cx - fx), wx[1] = 1.0 - wx[0];
    // the four neighbours, row-major: read only inside the box and where the label is the paragraph's
    bool take[4];
    size_t at[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int y = iy + (j >> 1), x = ix + (j & 1);
        take[j] = y < e.ch && x < e.cw;
        at[j] = take[j] ? (size_t)y * e.pitch + x : 0;
        take[j] = take[j] && e.lab[at[j]] == e.id;
    }
    const T* src = (const T*)e.src;
    for (int k = 0; k < c; ++k) {
        double t = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (take[j]) t += ((double)src[at[j] * c + k] * wy[j >> 1]) * wx[j & 1];
        out[k] = (T)t;
    }
}

// matrix and offset of entry i are numbers (inf * 0 and NaN * 0 are NaN)
inline bool rt_finite(const double* matrix, const double* offset, int i) {
    const double *m = matrix + 4 * i, *o = offset + 2 * i;
    return m[0] * 0.0 + m[1] * 0.0 + m[2] * 0.0 + m[3] * 0.0 + o[0] * 0.0 + o[1] * 0.0 == 0.0;
}

// the box (y0, x0, height, width) is not empty and lies inside h x w
inline bool rt_box_inside(const int* bx, int h, int w) {
    return bx[0] >= 0 && bx[1] >= 0 && bx[2] >= 1 && bx[3] >= 1 && bx[2] <= h - bx[0] && bx[3] <= w - bx[1];
}

}  // namespace

extern "C" {

int uocr_rotated_extent(uocr_ctx* ctx, const int* labels, int n, int h, int w, int image_index, int n_probes,
                        const int* label_id, const int* box, const double* matrix, const double* offset,
                        const int* out_shape, int* extent) {
    UOCR_CHECK_CTX(ctx);
    UOCR_REQUIRE(ctx, n_probes >= 0);
    if (n_probes == 0) return UOCR_OK;                             // nothing to do, whatever else was passed
    UOCR_REQUIRE(ctx, labels && label_id && box && matrix && offset && out_shape && extent);
    UOCR_REQUIRE(ctx, n >= 1 && h >= 1 && w >= 1 && image_index >= 0 && image_index < n);
    UOCR_REQUIRE(ctx, reinterpret_cast<uintptr_t>(extent) % sizeof(int) == 0);
    if ((long long)h * w > INT32_MAX) UOCR_FAIL(ctx, UOCR_ERR_UNSUPPORTED, "image of %d x %d pixels: linear indices must fit int32", h, w);
    // everything is checked before the first launch: an error leaves the extents as they were
    const auto blocks = [&](int i) { return (out_shape[2 * i] + RT_BAND - 1) / RT_BAND; };
    for (int first = 0; first < n_probes; first += RT_ENTRIES) {
        const int count = eb_group_size(n_probes, first, RT_ENTRIES);
        for (int i = first; i < first + count; ++i) {
            UOCR_REQUIRE(ctx, label_id[i] >= 1);
            UOCR_REQUIRE(ctx, rt_box_inside(box + 4 * i, h, w));
            UOCR_REQUIRE(ctx, out_shape[2 * i] >= 1 && out_shape[2 * i + 1] >= 1);
            UOCR_REQUIRE(ctx, rt_finite(matrix, offset, i));
        }
        if (eb_group_blocks(first, count, blocks) < 0)
            UOCR_FAIL(ctx, UOCR_ERR_UNSUPPORTED, "probes %d..: too many blocks for one grid", first);
    }
    UOCR_HIP(ctx, hipMemsetAsync(extent, 0, (size_t)n_probes * 4 * sizeof(int), ctx->stream));
    const int* lab = labels + (size_t)image_index * h * w;
    int launches = 0;
    for (int first = 0; first < n_probes; first += RT_ENTRIES) {
        RTBatch b;
        memset(&b, 0, sizeof(b));
        b.n = eb_group_size(n_probes, first, RT_ENTRIES);
        eb_block_first(first, b.n, b.block_first, blocks);
        b.extent = extent + 4 * (size_t)first;
        for (int i = 0; i < b.n; ++i) {
            const int s = first + i;
            RTProbe& p = b.probe[i];
            p.lab = lab + (size_t)box[4 * s] * w + box[4 * s + 1];
            memcpy(p.m, matrix + 4 * s, sizeof(p.m));
            memcpy(p.off, offset + 2 * s, sizeof(p.off));
            p.pitch = w, p.id = label_id[s], p.ch = box[4 * s + 2], p.cw = box[4 * s + 3];
            p.out_h = out_shape[2 * s], p.out_w = out_shape[2 * s + 1];
        }
        hipLaunchKernelGGL(rotated_extent, dim3((unsigned)b.block_first[b.n]), dim3(RT_NT), 0, ctx->stream, b);
        UOCR_LAUNCH_CHECK(ctx);
        hipLaunchKernelGGL(rotated_extent_finish, dim3(1), dim3(64), 0, ctx->stream, b);
        UOCR_LAUNCH_CHECK(ctx);
        launches += 2;
    }
    uocr_note(ctx, UOCR_REPORT_ROTATE, RT_BAND, RT_NT, RT_ENTRIES, launches);
    return UOCR_OK;
}

int uocr_rotate_crop(uocr_ctx* ctx, int dtype, int n_entries, const void* const* image, const int* const* labels,
                     const int* dims, const int* image_index, const int* label_id, const int* box, const double* matrix,
                     const double* offset, const int* plane, const int* region, void* const* out, const int* out_shape) {
    UOCR_CHECK_CTX(ctx);
    UOCR_REQUIRE(ctx, n_entries >= 0);
    if (n_entries == 0) return UOCR_OK;                            // nothing to do, whatever else was passed
    UOCR_REQUIRE(ctx, image && labels && dims && image_index && label_id && box && matrix && offset && plane && region && out && out_shape);
    const size_t elem = eb_storage_elem(ctx, dtype);
    if (!elem) return UOCR_ERR_DTYPE;
    const auto blocks = [&](int i) { return ((long long)out_shape[2 * i] * out_shape[2 * i + 1] + RT_NT - 1) / RT_NT; };
    // everything is checked before the first launch: an error leaves every output as it was
    for (int first = 0; first < n_entries; first += RT_ENTRIES) {
        const int count = eb_group_size(n_entries, first, RT_ENTRIES);
        for (int i = first; i < first + count; ++i) {
            const int *d = dims + 4 * i, *bx = box + 4 * i, *pl = plane + 2 * i, *rg = region + 4 * i, *os = out_shape + 2 * i;
            UOCR_REQUIRE(ctx, image[i] && labels[i] && out[i]);
            UOCR_REQUIRE(ctx, (reinterpret_cast<uintptr_t>(image[i]) | reinterpret_cast<uintptr_t>(out[i])) % elem == 0);
            UOCR_REQUIRE(ctx, reinterpret_cast<uintptr_t>(labels[i]) % sizeof(int) == 0);
            UOCR_REQUIRE(ctx, d[0] >= 1 && d[1] >= 1 && d[2] >= 1 && d[3] >= 1);
            UOCR_REQUIRE(ctx, image_index[i] >= 0 && image_index[i] < d[0] && label_id[i] >= 1);
            UOCR_REQUIRE(ctx, rt_box_inside(bx, d[1], d[2]));
            UOCR_REQUIRE(ctx, pl[0] >= 1 && pl[1] >= 1);
            UOCR_REQUIRE(ctx, rt_box_inside(rg, pl[0], pl[1]));
            UOCR_REQUIRE(ctx, os[0] >= rg[2] && os[1] >= rg[3]);
            UOCR_REQUIRE(ctx, rt_finite(matrix, offset, i));
            if ((long long)d[1] * d[2] > INT32_MAX)
                UOCR_FAIL(ctx, UOCR_ERR_UNSUPPORTED, "entry %d: image of %d x %d pixels: linear indices must fit int32", i, d[1], d[2]);
        }
        if (eb_group_blocks(first, count, blocks) < 0)
            UOCR_FAIL(ctx, UOCR_ERR_UNSUPPORTED, "entries %d..: too many blocks for one grid", first);
    }
    int launches = 0;
    for (int first = 0; first < n_entries; first += RT_ENTRIES) {
        RCBatch b;
        memset(&b, 0, sizeof(b));
        b.n = eb_group_size(n_entries, first, RT_ENTRIES);
        eb_block_first(first, b.n, b.block_first, blocks);
        for (int i = 0; i < b.n; ++i) {
            const int s = first + i;
            const int *d = dims + 4 * s, *bx = box + 4 * s, *rg = region + 4 * s, *os = out_shape + 2 * s;
            RCEntry& e = b.entry[i];
            const size_t pixel = ((size_t)image_index[s] * d[1] + bx[0]) * d[2] + bx[1];
            e.src = (const char*)image[s] + pixel * d[3] * elem;
            e.lab = labels[s] + pixel;
            e.out = out[s];
            memcpy(e.m, matrix + 4 * s, sizeof(e.m));
            memcpy(e.off, offset + 2 * s, sizeof(e.off));
            e.pitch = d[2], e.c = d[3], e.id = label_id[s], e.ch = bx[2], e.cw = bx[3];
            e.ry0 = rg[0], e.rx0 = rg[1], e.rh = rg[2], e.rw = rg[3];
            e.out_h = os[0], e.out_w = os[1];
            e.py = (e.out_h - e.rh) / 2, e.px = (e.out_w - e.rw) / 2;
        }
        UOCR_DISPATCH_STORAGE(ctx, dtype, {
            hipLaunchKernelGGL(rotate_crop<T>, dim3((unsigned)b.block_first[b.n]), dim3(RT_NT), 0, ctx->stream, b);
            UOCR_LAUNCH_CHECK(ctx);
        });
        launches += 1;
    }
    uocr_note(ctx, UOCR_REPORT_ROTATE, RT_BAND, RT_NT, RT_ENTRIES, launches);
    return UOCR_OK;
}

int uocr_rotation_search_workspace(int n_paragraphs, size_t* bytes) {
    if (n_paragraphs < 0 || !bytes) return UOCR_ERR_ARG;
    *bytes = (size_t)n_paragraphs * RS_STATE * sizeof(int);
    return UOCR_OK;
}

int uocr_rotation_search(uocr_ctx* ctx, const int* labels, int n, int h, int w, int image_index, int n_paragraphs,
                         const int* label_id, const int* box, int rounds, const double* table, int* result, int* workspace) {
    UOCR_CHECK_CTX(ctx);
    UOCR_REQUIRE(ctx, n_paragraphs >= 0);
    if (n_paragraphs == 0) return UOCR_OK;                         // nothing to do, whatever else was passed
    UOCR_REQUIRE(ctx, labels && label_id && box && table && result && workspace);
    UOCR_REQUIRE(ctx, n >= 1 && h >= 1 && w >= 1 && image_index >= 0 && image_index < n);
    UOCR_REQUIRE(ctx, rounds >= 1 && rounds <= RS_MAX_ROUNDS);
    UOCR_REQUIRE(ctx, (reinterpret_cast<uintptr_t>(result) | reinterpret_cast<uintptr_t>(workspace)) % sizeof(int) == 0);
    UOCR_REQUIRE(ctx, reinterpret_cast<uintptr_t>(table) % sizeof(double) == 0);
    if ((long long)h * w > INT32_MAX) UOCR_FAIL(ctx, UOCR_ERR_UNSUPPORTED, "image of %d x %d pixels: linear indices must fit int32", h, w);
    // everything is checked before the first launch: an error leaves the result as it was.  A probe's rows are known to
    // the device alone; out_h = int(ptp + 0.5) with ptp <= |c| h + |s| w <= hypot(h, w) is at most int(hypot) + 1
    const auto blocks = [&](int i) {
        const int* bx = box + 4 * (i >> 1);
        return ((int)hypot((double)bx[2], (double)bx[3]) + 2 + RT_BAND - 1) / RT_BAND;
    };
    for (int first = 0; first < n_paragraphs; first += RS_PARAGRAPHS) {
        const int count = eb_group_size(n_paragraphs, first, RS_PARAGRAPHS);
        for (int i = first; i < first + count; ++i) {
            UOCR_REQUIRE(ctx, label_id[i] >= 1);
            UOCR_REQUIRE(ctx, rt_box_inside(box + 4 * i, h, w));
        }
        if (eb_group_blocks(2 * first, 2 * count, blocks) < 0)
            UOCR_FAIL(ctx, UOCR_ERR_UNSUPPORTED, "paragraphs %d..: too many blocks for one grid", first);
    }
    UOCR_HIP(ctx, hipMemsetAsync(workspace, 0, (size_t)n_paragraphs * RS_STATE * sizeof(int), ctx->stream));   // node 0, nothing set
    const int* lab = labels + (size_t)image_index * h * w;
    int launches = 0;
    for (int first = 0; first < n_paragraphs; first += RS_PARAGRAPHS) {
        RSBatch b;
        memset(&b, 0, sizeof(b));
        b.n = eb_group_size(n_paragraphs, first, RS_PARAGRAPHS);
        eb_block_first(2 * first, 2 * b.n, b.block_first, blocks);
        b.pitch = w, b.stride = 1 + 2 * rounds, b.table = table;
        b.state = workspace + (size_t)RS_STATE * first;
        b.result = result + (size_t)b.stride * first;
        for (int i = 0; i < b.n; ++i) {
            const int s = first + i;
            RSParagraph& p = b.par[i];
            p.lab = lab + (size_t)box[4 * s] * w + box[4 * s + 1];
            p.id = label_id[s], p.ch = box[4 * s + 2], p.cw = box[4 * s + 3];
        }
        for (b.round = 0; b.round < rounds; ++b.round) {
            hipLaunchKernelGGL(search_probe, dim3((unsigned)b.block_first[2 * b.n]), dim3(RT_NT), 0, ctx->stream, b);
            UOCR_LAUNCH_CHECK(ctx);
            hipLaunchKernelGGL(search_decide, dim3(1), dim3(64), 0, ctx->stream, b);
            UOCR_LAUNCH_CHECK(ctx);
            launches += 2;
        }
    }
    uocr_note(ctx, UOCR_REPORT_ROTATION_SEARCH, rounds, RS_PARAGRAPHS, launches);
    return UOCR_OK;
}

int uocr_ctx_last_rotation_search(uocr_ctx* ctx, int* rounds, int* paragraphs_per_launch, int* launches) {
    return uocr_report_read(ctx, UOCR_REPORT_ROTATION_SEARCH, rounds, paragraphs_per_launch, launches);
}

int uocr_ctx_last_rotate(uocr_ctx* ctx, int* rows_per_band, int* pixels_per_block, int* entries_per_launch, int* launches) {
    return uocr_report_read(ctx, UOCR_REPORT_ROTATE, rows_per_band, pixels_per_block, entries_per_launch, launches);
}

}  // extern "C"
