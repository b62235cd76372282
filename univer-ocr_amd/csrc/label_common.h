// What the two labelling calls share: uocr_label_components (label.hip: a batch of equal images) and uocr_label_batch
// (label_batch.hip: a list of images of different sizes, each one channel of an interleaved tensor).  The union-find,
// the block scan, the run accumulator of the table and the body of every step of the chain as a function of ONE image:
// its size, its tile / chunk / strip and its planes.  The kernels only differ in how a block finds its image.  Linear
// indices and roots are image-local int32.  No floating-point arithmetic in here.
#pragma once
#include "entry_batch.h"

constexpr int LTH = 16, LTW = 64;          // tile of the local and merge steps
constexpr int LNT = 256;                   // threads per block of every labelling kernel
constexpr int LCHUNK = 1024;               // pixels per block of the flatten and rank steps
constexpr int LROWS = 16;                  // rows per wave of the relabel step

__device__ __forceinline__ int g_load(int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int g_min(int* p, int v) {
    return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int l_load(int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ int l_min(int* p, int v) {
    return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// Union-find whose links always point to a smaller index of the same component.  A link is only ever lowered
// (atomicMin), so a reader that sees an older value still walks inside the component and every loop ends; whoever
// replaces a link a -> old by a -> b goes on to unite old and b, so no connection is lost.  GLOBAL = the image plane in
// HBM (relaxed agent-scope atomics: the L2s are per XCD), else a tile in LDS.
template <bool GLOBAL>
__device__ __forceinline__ int uf_load(int* L, int i) { return GLOBAL ? g_load(L + i) : l_load(L + i); }
template <bool GLOBAL>
__device__ __forceinline__ int uf_min(int* L, int i, int v) { return GLOBAL ? g_min(L + i, v) : l_min(L + i, v); }

template <bool GLOBAL>
__device__ __forceinline__ int uf_find(int* L, int x) {
    int at = x, p;
    while ((p = uf_load<GLOBAL>(L, x)) != x) x = p;
    if (GLOBAL)                                                // shorten the chain for whoever walks it next (still only lowering)
        while (at > x) {                                       // (links go strictly downwards: this ends at or below x)
            p = uf_load<true>(L, at);
            if (p > x) uf_min<true>(L, at, x);
            at = p;
        }
    return x;
}

template <bool GLOBAL>
__device__ __forceinline__ void uf_unite(int* L, int a, int b) {
    for (;;) {
        a = uf_find<GLOBAL>(L, a);
        b = uf_find<GLOBAL>(L, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = uf_min<GLOBAL>(L, a, b);
        if (old == a) return;                                  // a was a root and now hangs below b
        a = old;                                               // a had a parent already: that one and b remain to be united
    }
}

// ---- tile-local union-find: tile (tx, ty) of an h x w image whose pixel (gy, gx) is foreground where is_fg(gy, gx) (only
// asked inside the image); L = LTH * LTW ints of LDS; writes the tile root's image-linear index, -1 = background
template <typename F>
__device__ __forceinline__ void label_local_tile(F is_fg, int h, int w, int tx, int ty, int* L, int* __restrict__ plane) {
    const int lx = threadIdx.x & (LTW - 1), gx = tx * LTW + lx;
    constexpr int RSTEP = LNT / LTW, PER = LTH / RSTEP;
    static_assert(LTW == 64, "a wave is one row of the tile: its ballot is the row's foreground");
    bool fg[PER];
    int run[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int ly = (threadIdx.x / LTW) + k * RSTEP, gy = ty * LTH + ly;
        fg[k] = gy < h && gx < w && is_fg(gy, gx);
        // every pixel starts at the first pixel of its horizontal run: no union along a row is needed
        const unsigned long long gaps_below = ~__ballot(fg[k]) & ((1ull << lx) - 1ull);
        run[k] = gaps_below ? 64 - __clzll((long long)gaps_below) : 0;
        L[ly * LTW + lx] = fg[k] ? ly * LTW + run[k] : -1;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int ly = (threadIdx.x / LTW) + k * RSTEP, i = ly * LTW + lx;
        // with the row above: not where the left neighbour and the one above it are foreground too -- those two are in
        // this pixel's and the upper pixel's runs, and the union is made further left (at the run's start at the latest)
        if (fg[k] && ly > 0 && l_load(L + i - LTW) >= 0 && (lx == run[k] || l_load(L + i - LTW - 1) < 0))
            uf_unite<false>(L, i, i - LTW);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int ly = (threadIdx.x / LTW) + k * RSTEP, gy = ty * LTH + ly;
        if (gy < h && gx < w) {
            int out = -1;
            if (fg[k]) {
                const int r = uf_find<false>(L, ly * LTW + lx);
                out = (ty * LTH + r / LTW) * w + tx * LTW + (r % LTW);
            }
            plane[(size_t)gy * w + gx] = out;
        }
    }
}

// ---- unions across the top and left border of tile (tx, ty) of the h x w plane L
__device__ __forceinline__ void label_merge_tile(int h, int w, int tx, int ty, int* L) {
    for (int e = threadIdx.x; e < LTW + LTH; e += LNT) {
        int gy, gx, other;
        if (e < LTW) {                       // top row of the tile against the row above
            gy = ty * LTH, gx = tx * LTW + e;
            if (ty == 0 || gx >= w) continue;
            other = (gy - 1) * w + gx;
        } else {                             // left column against the column to its left
            gy = ty * LTH + (e - LTW), gx = tx * LTW;
            if (tx == 0 || gy >= h) continue;
            other = gy * w + gx - 1;
        }
        const int i = gy * w + gx;
        if (g_load(L + i) < 0 || g_load(L + other) < 0) continue;
        // the previous pixel along the border and its partner, when both are foreground, are joined to this pair inside
        // their tiles already and make the union themselves (or the pair before them does)
        const int back = e < LTW ? 1 : w;
        if (e != 0 && e != LTW && g_load(L + i - back) >= 0 && g_load(L + other - back) >= 0) continue;
        uf_unite<true>(L, i, other);
    }
}

// exclusive scan of one int per thread over the block (LNT threads); *total = the block's sum.  Contains barriers.
__device__ __forceinline__ int block_exscan(int v, int* total, int* smem /* >= LNT / 64 + 1 */) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(inc, off, 64);
        if (lane >= off) inc += o;
    }
    __syncthreads();
    if (lane == 63) smem[wid] = inc;
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < LNT / 64; ++k) {
        before += k < wid ? smem[k] : 0;
        all += smem[k];
    }
    *total = all;
    return before + inc - v;
}

// ---- flatten: the root of every pixel of chunk `chunk` of the plane L (hw pixels) into R; returns the chunk's roots
__device__ __forceinline__ int label_flatten_chunk(int hw, int chunk, const int* __restrict__ L, int* __restrict__ R,
                                                   int* smem /* >= LNT / 64 + 1 */) {
    int mine = 0;
#pragma unroll
    for (int j = 0; j < LCHUNK / LNT; ++j) {
        const int i = chunk * LCHUNK + j * LNT + threadIdx.x;
        if (i < hw) {
            int r = L[i];                      // (no block writes the plane in this launch)
            if (r >= 0) {
                int p = r;
                r = i;
                while (p != r) {
                    r = p;
                    p = L[r];
                }
                mine += r == i;
            }
            R[i] = r;
        }
    }
    int total;
    block_exscan(mine, &total, smem);
    return total;
}

// ---- exclusive scan of the `chunks` chunk counts of one image, in place; returns the image's count
__device__ __forceinline__ int label_scan_image(int chunks, int* __restrict__ c, int* smem /* >= LNT / 64 + 1 */) {
    int running = 0;
    for (int first = 0; first < chunks; first += LNT) {
        const int i = first + threadIdx.x;
        const int v = i < chunks ? c[i] : 0;
        int total;
        const int ex = block_exscan(v, &total, smem);
        if (i < chunks) c[i] = running + ex;
        running += total;
    }
    return running;
}

// ---- rank: the number of every root of chunk `chunk` (written at the root's own pixel of the plane P), its table entry
// initialised; `running` = roots of the image before this chunk
__device__ __forceinline__ void label_rank_chunk(int hw, int chunk, int running, const int* __restrict__ R,
                                                 int* __restrict__ P, long long* __restrict__ T, int max_components,
                                                 int* smem /* >= LNT / 64 + 1 */) {
    for (int j = 0; j < LCHUNK / LNT; ++j) {
        const int i = chunk * LCHUNK + j * LNT + threadIdx.x;
        const int is_root = i < hw && R[i] == i;
        int total;
        const int ex = block_exscan(is_root, &total, smem);
        if (is_root) {
            const int k = running + ex + 1;
            P[i] = k;
            if (k <= max_components) {
                long long* e = T + (size_t)(k - 1) * 8;
                e[0] = i, e[1] = 0, e[2] = INT32_MAX, e[3] = 0, e[4] = INT32_MAX, e[5] = 0, e[6] = 0, e[7] = 0;
            }
        }
        running += total;
    }
}

// ---- final labels + table
struct RunAcc {
    int k;
    long long area, y0, y1, x0, x1, sy, sx;
};
__device__ __forceinline__ void table_flush(long long* table_img, int max_components, const RunAcc& a) {
    if (a.k <= 0 || a.k > max_components) return;
    unsigned long long* e = reinterpret_cast<unsigned long long*>(table_img + (size_t)(a.k - 1) * 8);
    atomicAdd(e + 1, (unsigned long long)a.area);
    atomicMin(e + 2, (unsigned long long)a.y0);
    atomicMax(e + 3, (unsigned long long)a.y1);
    atomicMin(e + 4, (unsigned long long)a.x0);
    atomicMax(e + 5, (unsigned long long)a.x1);
    atomicAdd(e + 6, (unsigned long long)a.sy);
    atomicAdd(e + 7, (unsigned long long)a.sx);
}

// One wave owns the strip (sx_, sy_) of 64 columns x LROWS rows of an h x w image: roots R, plane P, table T.  Per row:
// the heads of runs of equal label come from one ballot; a run that fills the strip's whole width and continues the
// label of the rows above is kept in (wave-uniform) registers and flushed once, by lane 0, when the label changes or the
// strip ends.
__device__ __forceinline__ void label_relabel_strip(int h, int w, int sx_, int sy_, const int* __restrict__ R,
                                                    int* __restrict__ P, long long* __restrict__ T, int max_components) {
    const int lane = threadIdx.x & 63;
    const int gx = sx_ * 64 + lane;
    const int valid_n = min(64, w - sx_ * 64);                      // lanes of this strip inside the image
    const bool valid = lane < valid_n;
    RunAcc acc;
    acc.k = 0;
    const int y_end = min(h, (sy_ + 1) * LROWS);
    for (int gy = sy_ * LROWS; gy < y_end; ++gy) {
        int k = 0;
        if (valid) {
            const int r = R[(size_t)gy * w + gx];
            if (r >= 0) k = P[r];                                   // the root's pixel holds the number (rank step) ...
            if (r != gy * w + gx) P[(size_t)gy * w + gx] = k;       // ... and is the one pixel this launch only reads
        }
        const int prev = __shfl_up(k, 1, 64);
        const bool head = valid && (lane == 0 || k != prev);
        const unsigned long long heads = __ballot(head);
        const int k0 = __shfl(k, 0, 64);
        if (heads == 1ull) {                                        // one run over the whole width: wave-uniform
            if (k0 != acc.k) {
                if (lane == 0) table_flush(T, max_components, acc);
                acc.k = k0, acc.area = 0, acc.sy = 0, acc.sx = 0;
                acc.y0 = gy, acc.x0 = sx_ * 64, acc.x1 = sx_ * 64 + valid_n;
            }
            if (k0 > 0) {
                acc.area += valid_n;
                acc.y1 = gy + 1;
                acc.sy += (long long)gy * valid_n;
                acc.sx += (long long)valid_n * (sx_ * 64) + (long long)valid_n * (valid_n - 1) / 2;
            }
            continue;
        }
        if (lane == 0) table_flush(T, max_components, acc);
        acc.k = 0;
        if (head && k > 0) {
            const unsigned long long later = lane == 63 ? 0ull : (heads >> (lane + 1)) << (lane + 1);
            const int end = later ? __ffsll((long long)later) - 1 : valid_n;
            const long long len = end - lane;
            RunAcc run;
            run.k = k, run.area = len, run.y0 = gy, run.y1 = gy + 1, run.x0 = gx, run.x1 = gx + len;
            run.sy = (long long)gy * len, run.sx = len * gx + len * (len - 1) / 2;
            table_flush(T, max_components, run);
        }
    }
    if (lane == 0) table_flush(T, max_components, acc);
}
