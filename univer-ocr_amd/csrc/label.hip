// Connected-component labelling, component table and masked crop: the device form of the reference's ParagraphCrop
// stage (interpreter/interpreter.py:16-21 label_layer, :303 ndimage.find_objects, :304-308 the masked crop) and of the
// labelling every later stage starts with (:437-438, :549).
//
// Foreground is x > t; connectivity is scipy's default structure (the four edge neighbours in the H-W plane).  EVERY
// IMAGE OF THE BATCH IS LABELLED ON ITS OWN: for N = 1 that is exactly what the reference computes; its 4-D
// ndimage.label call would also join equal pixels of neighbouring images, but its data path only ever has N = 1
// (my_model/datasets.py:18,39).  The components of an image are numbered 1..count in the order of their first pixel in
// row-major order, which is scipy's numbering: the representative of a component is its minimum linear index and its
// number is the rank of that root among the roots of its image.
//
// Launches of one uocr_label_components call, all on the context's stream (no grid barrier, nobody waits for another
// block; every exchange between blocks inside a launch is an integer atomic on a word that only ever decreases):
//   1. label_stats     float64 sum and max of x, the last block to arrive stores the threshold (not for THRESH_VALUE)
//   2. label_local     union-find of one LTH x LTW tile in LDS (a pixel starts at the head of its row run, unions only
//                      with the row above and once per pair of runs); writes the tile root's image-linear index, -1 =
//                      background
//   3. label_merge     unions across tile borders, one per pair of border runs: lock-free atomicMin retries on the plane
//   4. label_flatten   root of every pixel into the second plane (workspace) + roots per chunk of LCHUNK pixels
//   5. label_scan      one block per image: exclusive scan of the chunk counts, count[n]
//   6. label_rank      number of every root (written at the root's own pixel), its table entry initialised
//   7. label_relabel   final labels; box / area / coordinate sums: runs of equal label inside a wave are combined (a
//                      segmented reduction along the row), full-width runs of consecutive rows too, one atomic per
//                      field and flush -- never one per pixel
#include "label_common.h"

// float64 forms of the activation accessors of uocr_common.h (8 / 16 bytes per access)
__device__ __forceinline__ double ld1(const double* p) { return *p; }
__device__ __forceinline__ double2 ld2(const double* p) { return *reinterpret_cast<const double2*>(p); }
__device__ __forceinline__ void st1(double* p, double v) { *p = v; }
__device__ __forceinline__ void st2(double* p, double2 v) { *reinterpret_cast<double2*>(p) = v; }

namespace {

// (tile, chunk and strip sizes, the union-find and the body of steps 2-7 for one image: label_common.h, shared with
// label_batch.hip)

// ---- 1. threshold statistics ------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(LNT) void label_stats(const T* __restrict__ x, size_t count, int mode, unsigned* counter,
                                                   double* partial /* [grid][2] */, double* thr) {
    __shared__ double smem[17];
    double v[2] = {0.0, -INFINITY};                            // sum, max
    for (size_t i = (size_t)blockIdx.x * LNT + threadIdx.x; i < count; i += (size_t)gridDim.x * LNT) {
        const double xi = (double)x[i];
        v[0] += xi;
        v[1] = xi > v[1] ? xi : v[1];
    }
    v[0] = block_reduce_sum(v[0], smem);
    v[1] = block_reduce_max(v[1], smem);
    // (the last block to arrive folds the blocks' sums and maxima in a fixed order: the same bits run to run)
    if (!last_block_fold<LNT, 4, FoldSum, FoldMax>(counter, partial, v, smem)) return;
    if (threadIdx.x == 0) {
        const double mean = v[0] / (double)count;
        *thr = mode == UOCR_THRESH_MEAN ? mean : 0.5 * (mean + v[1]);
    }
}

// ---- 2. tile-local union-find -------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(LNT) void label_local(const T* __restrict__ x, int h, int w, int tiles_x, int tiles_y,
                                                   const double* thr_dev, double thr_value, int* __restrict__ plane) {
    __shared__ int L[LTH * LTW];
    const double thr = thr_dev ? *thr_dev : thr_value;
    const int tile = blockIdx.x;
    const int tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y, img = tile / (tiles_x * tiles_y);
    const size_t base = (size_t)img * h * w;
    label_local_tile([&](int gy, int gx) { return (double)x[base + (size_t)gy * w + gx] > thr; }, h, w, tx, ty, L,
                     plane + base);
}

// ---- 3. unions across tile borders ----------------------------------------------------------------------------------
__global__ __launch_bounds__(LNT) void label_merge(int h, int w, int tiles_x, int tiles_y, int* plane) {
    const int tile = blockIdx.x;
    const int tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y, img = tile / (tiles_x * tiles_y);
    label_merge_tile(h, w, tx, ty, plane + (size_t)img * h * w);
}

// ---- 4. flatten + roots per chunk ----------------------------------------------------------------------------------
__global__ __launch_bounds__(LNT) void label_flatten(int hw, int chunks, int* __restrict__ plane, int* __restrict__ root,
                                                     int* __restrict__ chunk_count) {
    __shared__ int smem[LNT / 64 + 1];
    const int img = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
    const int total = label_flatten_chunk(hw, chunk, plane + (size_t)img * hw, root + (size_t)img * hw, smem);
    if (threadIdx.x == 0) chunk_count[blockIdx.x] = total;
}

// ---- 5. scan of the chunk counts, one block per image ----------------------------------------------------------------
__global__ __launch_bounds__(LNT) void label_scan(int chunks, int* __restrict__ chunk_count, int* __restrict__ count) {
    __shared__ int smem[LNT / 64 + 1];
    const int total = label_scan_image(chunks, chunk_count + (size_t)blockIdx.x * chunks, smem);
    if (threadIdx.x == 0) count[blockIdx.x] = total;
}

// ---- 6. rank of every root ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LNT) void label_rank(int hw, int chunks, const int* __restrict__ root,
                                                  const int* __restrict__ chunk_offset, int* __restrict__ plane,
                                                  long long* __restrict__ table, int max_components) {
    __shared__ int smem[LNT / 64 + 1];
    const int img = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
    label_rank_chunk(hw, chunk, chunk_offset[blockIdx.x], root + (size_t)img * hw, plane + (size_t)img * hw,
                     table + (size_t)img * max_components * 8, max_components, smem);
}

// ---- 7. final labels + table: one wave per strip of 64 columns x LROWS rows ---------------------------------------------
__global__ __launch_bounds__(LNT) void label_relabel(int h, int w, int strips_x, int strips_y,
                                                     const int* __restrict__ root, int* __restrict__ plane,
                                                     long long* __restrict__ table, int max_components, int n) {
    const long long wave = (long long)blockIdx.x * (LNT / 64) + (threadIdx.x >> 6);
    const int sx_ = (int)(wave % strips_x), sy_ = (int)((wave / strips_x) % strips_y);
    const long long img = wave / ((long long)strips_x * strips_y);
    if (img >= n) return;                                           // (the grid is rounded up to whole blocks)
    const size_t hw = (size_t)h * w;
    label_relabel_strip(h, w, sx_, sy_, root + img * hw, plane + img * hw, table + (size_t)img * max_components * 8,
                        max_components);
}

// ---- masked crop ----------------------------------------------------------------------------------------------------------
// one thread per output pixel; C = 1 / 2 / 4 channels move as one 4- / 8- / 16-byte access of float (2 / 4 / 8 of
// binary16; float64 as 8 / 16 / 2 x 16), C = 0 is the generic loop over `c` channels
template <typename T, int C>
__global__ __launch_bounds__(LNT) void masked_crop(const T* __restrict__ image, const int* __restrict__ labels, int w, int c,
                                                   int label_id, int y0, int x0, int ch, int cw, int py, int px,
                                                   T* __restrict__ out, int out_h, int out_w) {
    const size_t o = (size_t)blockIdx.x * LNT + threadIdx.x;
    if (o >= (size_t)out_h * out_w) return;
    const int oy = (int)(o / out_w), ox = (int)(o % out_w);
    const int sy = oy - py, sx = ox - px;
    bool take = sy >= 0 && sy < ch && sx >= 0 && sx < cw;
    size_t src = 0;
    if (take) {
        src = (size_t)(y0 + sy) * w + (x0 + sx);
        take = labels[src] == label_id;
    }
    if constexpr (C == 0) {
        for (int i = 0; i < c; ++i) out[o * c + i] = take ? image[src * c + i] : T(0);
    } else if constexpr (C == 1) {
        decltype(ld1(image)) v = 0;
        if (take) v = ld1(image + src);
        st1(out + o, v);
    } else if constexpr (C == 2) {
        decltype(ld2(image)) v = {0, 0};
        if (take) v = ld2(image + src * 2);
        st2(out + o * 2, v);
    } else if constexpr (sizeof(T) == 8) {
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            double2 v = {0, 0};
            if (take) v = ld2(image + src * 4 + 2 * half);
            st2(out + o * 4 + 2 * half, v);
        }
    } else {
        decltype(ld4(image)) v = {0, 0, 0, 0};
        if (take) v = ld4(image + src * 4);
        st4(out + o * 4, v);
    }
}

}  // namespace

#define UOCR_CROP(C)                                                                                                   \
    hipLaunchKernelGGL((masked_crop<T, C>), dim3((unsigned)blocks), dim3(LNT), 0, ctx->stream, img, lab, w, c, label_id, \
                       y0, x0, ch, cw, py, px, (T*)out, out_h, out_w)

extern "C" {

int uocr_label_components(uocr_ctx* ctx, int dtype, const void* x, int n, int h, int w, int thresh_mode,
                          double thresh_value, int* labels, long long* table, int max_components, int* count) {
    UOCR_CHECK_CTX(ctx);
    UOCR_REQUIRE(ctx, x && labels && table && count);
    UOCR_REQUIRE(ctx, n >= 0 && h >= 0 && w >= 0 && max_components >= 0);
    UOCR_REQUIRE(ctx, thresh_mode == UOCR_THRESH_MEAN || thresh_mode == UOCR_THRESH_MEAN_MAX ||
                          thresh_mode == UOCR_THRESH_VALUE);
    if (!eb_storage_elem(ctx, dtype)) return UOCR_ERR_DTYPE;
    if ((long long)h * w > (long long)INT32_MAX - LCHUNK)
        UOCR_FAIL(ctx, UOCR_ERR_UNSUPPORTED, "image of %d x %d pixels: linear indices must fit int32", h, w);
    if (n == 0 || h == 0 || w == 0) return UOCR_OK;
    const int hw = h * w;
    const size_t pixels = (size_t)n * hw;
    const int tiles_x = (w + LTW - 1) / LTW, tiles_y = (h + LTH - 1) / LTH;
    const int chunks = (hw + LCHUNK - 1) / LCHUNK;
    const int strips_x = (w + 63) / 64, strips_y = (h + LROWS - 1) / LROWS;
    const long long tiles = (long long)n * tiles_x * tiles_y, nchunks = (long long)n * chunks;
    const long long relabel_blocks = ((long long)n * strips_x * strips_y + LNT / 64 - 1) / (LNT / 64);
    if (tiles > INT32_MAX || nchunks > INT32_MAX || relabel_blocks > INT32_MAX)
        UOCR_FAIL(ctx, UOCR_ERR_UNSUPPORTED, "batch of %d images of %d x %d: too many blocks for one grid", n, h, w);
    const unsigned stat_blocks = uocr_blocks_for(pixels, 4 * LNT, UOCR_MAX_GRID);
    // workspace: root plane | chunk counts | statistics partials (sum, max per block) | threshold
    const size_t off_counts = (pixels * sizeof(int) + 15) & ~(size_t)15;
    const size_t off_partial = (off_counts + (size_t)nchunks * sizeof(int) + 15) & ~(size_t)15;
    const size_t off_thr = off_partial + 2 * (size_t)stat_blocks * sizeof(double);
    if (int rc = uocr_need_workspace(ctx, off_thr + sizeof(double))) return rc;
    char* ws = (char*)ctx->workspace;
    int* root = (int*)ws;
    int* chunk_count = (int*)(ws + off_counts);
    double* partial = (double*)(ws + off_partial);
    double* thr = (double*)(ws + off_thr);
    int launches = 0;
    UOCR_DISPATCH_STORAGE(ctx, dtype, {
        if (thresh_mode != UOCR_THRESH_VALUE) {
            hipLaunchKernelGGL(label_stats<T>, dim3(stat_blocks), dim3(LNT), 0, ctx->stream, (const T*)x, pixels, thresh_mode,
                               ctx->sync + UOCR_SYNC_LABEL_STATS, partial, thr);
            UOCR_LAUNCH_CHECK(ctx);
            ++launches;
        }
        hipLaunchKernelGGL(label_local<T>, dim3((unsigned)tiles), dim3(LNT), 0, ctx->stream, (const T*)x, h, w, tiles_x,
                           tiles_y, thresh_mode == UOCR_THRESH_VALUE ? (const double*)nullptr : (const double*)thr,
                           thresh_value, labels);
        UOCR_LAUNCH_CHECK(ctx);
        ++launches;
    });
    if (tiles_x > 1 || tiles_y > 1) {
        hipLaunchKernelGGL(label_merge, dim3((unsigned)tiles), dim3(LNT), 0, ctx->stream, h, w, tiles_x, tiles_y, labels);
        UOCR_LAUNCH_CHECK(ctx);
        ++launches;
    }
    hipLaunchKernelGGL(label_flatten, dim3((unsigned)nchunks), dim3(LNT), 0, ctx->stream, hw, chunks, labels, root,
                       chunk_count);
    UOCR_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(label_scan, dim3(n), dim3(LNT), 0, ctx->stream, chunks, chunk_count, count);
    UOCR_LAUNCH_CHECK(ctx);
    if (max_components > 0)   // entries past an image's count read zero
        UOCR_HIP(ctx, hipMemsetAsync(table, 0, (size_t)n * max_components * 8 * sizeof(long long), ctx->stream));
    hipLaunchKernelGGL(label_rank, dim3((unsigned)nchunks), dim3(LNT), 0, ctx->stream, hw, chunks, (const int*)root,
                       (const int*)chunk_count, labels, table, max_components);
    UOCR_LAUNCH_CHECK(ctx);
    hipLaunchKernelGGL(label_relabel, dim3((unsigned)relabel_blocks), dim3(LNT), 0, ctx->stream, h, w, strips_x, strips_y,
                       (const int*)root, labels, table, max_components, n);
    UOCR_LAUNCH_CHECK(ctx);
    launches += 4;
    uocr_note(ctx, UOCR_REPORT_LABEL, LTH, LTW, launches);
    return UOCR_OK;
}

int uocr_masked_crop(uocr_ctx* ctx, int dtype, const void* image, const int* labels, int n, int h, int w, int c,
                     int image_index, int label_id, int y0, int x0, int ch, int cw, void* out, int out_h, int out_w) {
    UOCR_CHECK_CTX(ctx);
    UOCR_REQUIRE(ctx, image && labels && out);
    UOCR_REQUIRE(ctx, n >= 0 && h >= 0 && w >= 0 && c >= 0 && ch >= 0 && cw >= 0 && out_h >= 0 && out_w >= 0);
    UOCR_REQUIRE(ctx, image_index >= 0 && image_index < n && label_id >= 1);
    UOCR_REQUIRE(ctx, y0 >= 0 && x0 >= 0 && ch <= h - y0 && cw <= w - x0);
    UOCR_REQUIRE(ctx, out_h >= ch && out_w >= cw);
    if (!eb_storage_elem(ctx, dtype)) return UOCR_ERR_DTYPE;
    const size_t out_pixels = (size_t)out_h * out_w;
    if (out_pixels == 0 || c == 0) return UOCR_OK;
    const size_t blocks = (out_pixels + LNT - 1) / LNT;
    if (blocks > INT32_MAX) UOCR_FAIL(ctx, UOCR_ERR_UNSUPPORTED, "crop of %d x %d pixels: too many blocks", out_h, out_w);
    const int py = (out_h - ch) / 2, px = (out_w - cw) / 2;
    const size_t hw = (size_t)h * w;
    const int* lab = labels + (size_t)image_index * hw;
    UOCR_DISPATCH_STORAGE(ctx, dtype, {
        const T* img = (const T*)image + (size_t)image_index * hw * c;
        const size_t pixel_bytes = sizeof(T) * (size_t)c;
        const size_t align = pixel_bytes > 16 ? 16 : pixel_bytes;
        const bool vec = (c == 1 || c == 2 || c == 4) &&
                         ((reinterpret_cast<uintptr_t>(img) | reinterpret_cast<uintptr_t>(out)) & (align - 1)) == 0;
        if (vec && c == 1) UOCR_CROP(1);
        else if (vec && c == 2) UOCR_CROP(2);
        else if (vec && c == 4) UOCR_CROP(4);
        else UOCR_CROP(0);
        UOCR_LAUNCH_CHECK(ctx);
    });
    return UOCR_OK;
}

int uocr_ctx_last_label(uocr_ctx* ctx, int* tile_h, int* tile_w, int* launches) {
    return uocr_report_read(ctx, UOCR_REPORT_LABEL, tile_h, tile_w, launches);
}

}  // extern "C"
