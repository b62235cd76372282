// Shared by the strip kernels of the fused Monochrome block (conv_pair_strip.hip: float32, conv_pair_strip_h.hip:
// binary16 storage): LDS layouts, the MFMA ordering helper, the partial-sum layout and its block reduction, the row
// descriptors, the host rules of all five launch forms (geometry, bands, tag dispatch, the launch with more than 64 KB
// of dynamic LDS) and the finish launch.  Not part of the C ABI.
#pragma once
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <type_traits>

#include "mfma.h"
#include "uocr_common.h"

namespace pair_strip {

constexpr int CH = 16;
constexpr int XROW = 80;      // floats per (ring slot, group) of the x ring: copies tx = 0, 1, 2, ones, dump
constexpr int GROW = 64;      // ... of the g ring: copies tx = 0, 1, 2, dump
// d_a1 transpose scratch of a group: [channel quad q][slot f(pos)][4 channels], plane stride TPL = 64 + 8 floats.
// f sends the positions {0-3, 12-15} to the even and {4-11} to the odd slots: a ds_read_b128 lane group holds exactly
// those two position sets of two neighbouring quads (MI355X LDS lane groups), so its 16 lanes hit 16 different 16-B
// slots, and the 32 lanes of a ds_write_b32 group hit 32 different banks (row stride 20 floats: 2- to 3-way conflicts)
constexpr int TPL = 72;
constexpr int TRSZ = 4 * TPL;
__device__ __forceinline__ int tslot(int pos) { return pos < 4 ? 2 * pos : pos >= 12 ? 2 * (pos - 12) + 8 : 2 * (pos - 4) + 1; }
constexpr int NSLOT = 6;      // rows of the output ring: two batches of three
constexpr int NPLANE = 3;     // tx = 0, 1, 2 (lane quarter 3 does not store)

template <int G>
struct Strip {
    // ring slot strides = 48 mod 64 floats: the three window rows a ds_read_b128 lane group reads (tap rows ty) then
    // fall on different 16-float bank units ((3 ty + tx) mod 4) instead of on the same one
    static constexpr int XSLOT = (G * XROW + 63) / 64 * 64 + 48;
    static constexpr int GSLOT = (G * GROW + 63) / 64 * 64 + 48;
    static constexpr int XS = 3 * XSLOT;             // x ring [slot][group][XROW]
    static constexpr int GS = 3 * GSLOT;
    static constexpr int TR = G * TRSZ;              // one transpose scratch per group
    static constexpr int WAVE = XS + GS + TR;        // floats of wave-private LDS
    static constexpr int COLS = 16 * G;              // computed columns per wave
};

template <int P>
using phase_t = std::integral_constant<int, P>;

// Keeps the MFMAs on either side in program order (everything else may still move across): hipcc otherwise
// clusters the MFMAs of one accumulator back to back, and a dependent v_mfma_f32_16x16x4_f32 issues every 40
// cycles instead of every 32 (measured here: 39.6 cycles per MFMA before, rounds of independent accumulators after)
__device__ __forceinline__ void mfma_round() { __builtin_amdgcn_sched_barrier(0x7F6); }

// partial[block][PAIR_NPART]: dW1^T (16 rows: taps 0..8, row 9 = db1) x 16 channels, dW2^T likewise, db2
constexpr int PAIR_NPART = 2 * 256 + 1;

// Buffer descriptor of one page row (base = the row, size = the row or nothing): the column one past the image and
// whole rows outside it read as 0 without a vector instruction.  In the kernel:
//     const unsigned row_bytes = (unsigned)wd * (unsigned)sizeof(T);  const RowRsrc<T> row_rsrc{h, wd, row_bytes};
// Three references, what the [&] lambda of each kernel captured: with values, or with the product in here, the
// compiler places it elsewhere and the kernels come out in another instruction order (profiles/pair_strip_share.txt)
template <typename T>
struct RowRsrc {
    const int &h, &wd;
    const unsigned& row_bytes;
    __device__ auto operator()(const T* base, int row) const {
        const bool in = row >= 0 && row < h;
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(base + (size_t)min(max(row, 0), h - 1) * wd), 0,
                                                 in ? row_bytes : 0u, 0x00020000);
    }
};

// Block reduction of the weight gradients -> partial[blk][PAIR_NPART] at the end of the three backward kernels: the
// block's LDS becomes red[nw][PAIR_NPART] once every wave has passed the first barrier.  A macro that names everything
// it uses, because every function form tried (coordinates by value, by reference, forced or ordinary inlining) changed
// the instruction stream of all 32 backward kernels (profiles/pair_strip_share.txt); blk is evaluated after the second
// barrier.
#define PAIR_STRIP_REDUCE_TO_PARTIAL(G, lds, partial, blk_expr, acc1, acc2, db2acc, tid, lane, n, kq, wv, nw, wc0, own_lo, \
                                     own_hi)                                                                             \
    do {                                                                                                                 \
        __syncthreads();                                                                                                 \
        float* red = lds;                                                                                                \
        {                                                                                                                \
            const f32x4 s1 = acc1[0] + acc1[1], s2 = acc2[0] + acc2[1];                                                  \
            float* rw = red + wv * pair_strip::PAIR_NPART;                                                               \
            _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                              \
                rw[(4 * kq + i) * 16 + n] = s1[i];                                                                       \
                rw[256 + (4 * kq + i) * 16 + n] = s2[i];                                                                 \
            }                                                                                                            \
            float b2 = 0.f;                                                                                              \
            _Pragma("unroll") for (int g = 0; g < G; ++g) {                                                              \
                const int c = wc0 + 16 * g + n;                                                                          \
                if (kq == 1 && c >= own_lo && c < own_hi) b2 += db2acc[g];                                               \
            }                                                                                                            \
            b2 = wave_reduce_sum(b2);                                                                                    \
            if (lane == 0) rw[512] = b2;                                                                                 \
        }                                                                                                                \
        __syncthreads();                                                                                                 \
        const size_t blk = (blk_expr);                                                                                   \
        for (int i = tid; i < pair_strip::PAIR_NPART; i += blockDim.x) {                                                 \
            float v = 0.f;                                                                                               \
            for (int w = 0; w < nw; ++w) v += red[w * pair_strip::PAIR_NPART + i];                                       \
            partial[blk * pair_strip::PAIR_NPART + i] = v;                                                               \
        }                                                                                                                \
    } while (0)

// ---- host rules of the launch forms (kernels 1..5 of uocr_ctx_last_pair) ----------------------------------------------
// cooperative block: waves, computed columns, column blocks (neighbours overlap by two columns)
struct BlockGeometry { int nw, bwc, nbx; };
inline BlockGeometry pair_block_geometry(int w, int cols_per_wave, int max_waves) {
    const int nw = std::min(max_waves, (w + cols_per_wave - 1) / cols_per_wave);
    const int bwc = nw * cols_per_wave;
    return {nw, bwc, w <= bwc ? 1 : 1 + (w - bwc + (bwc - 2) - 1) / (bwc - 2)};
}
// independent waves: strips of `cols` computed columns every cols - 2, four strips per block
struct WaveGeometry { int nstrips, nw, blocks_x; };
inline WaveGeometry pair_wave_geometry(int w, int cols) {
    const int nstrips = w <= cols ? 1 : 1 + (w - cols + (cols - 2) - 1) / (cols - 2);
    const int nw = std::min(4, nstrips);
    return {nstrips, nw, (nstrips + nw - 1) / nw};
}
struct Bands { int bands, band_h; };
// cooperative kernels: `blocks_wanted` bands (what is resident over n * nbx, at least 1) unless pair_band sets the rows;
// bands raised to 4 rows so that the t = r0-1 .. r1 steps fill whole batches of three, never above h
inline Bands pair_bands_per_cu(int h, int blocks_wanted, int pair_band) {
    int bands = std::max(1, blocks_wanted);
    if (pair_band > 0) bands = (h + pair_band - 1) / pair_band;
    const int band_h = std::min(h, std::max(4, (h + bands - 1) / bands));
    return {(h + band_h - 1) / band_h, band_h};
}
// independent waves: bands so that the blocks make whole rounds of what is resident at once -- a last round that is a
// tenth full costs a full one
inline Bands pair_bands_rounds(int n, int h, int blocks_x, long resident, int pair_band) {
    int bands = 1;
    double best = 1e30;
    for (int b = 1; b <= std::max(1, h / 8); ++b) {
        const int bh = (h + b - 1) / b;
        const long blocks = (long)blocks_x * ((h + bh - 1) / bh) * n;
        const double cost = (double)((blocks + resident - 1) / resident) * (bh + 2);
        if (cost < best * 0.999) { best = cost; bands = (h + bh - 1) / bh; }
    }
    if (pair_band > 0) bands = (h + pair_band - 1) / pair_band;
    const int band_h = (h + bands - 1) / bands;
    return {(h + band_h - 1) / band_h, band_h};
}

// f(dx tag, sig tag): the run-time (dx wanted, sigmoid) as the two compile-time tags of the backward kernels
template <typename F>
int pair_dx_sig(bool dx, bool sig, F&& f) {
    if (dx) return sig ? f(std::true_type{}, std::true_type{}) : f(std::true_type{}, std::false_type{});
    return sig ? f(std::false_type{}, std::true_type{}) : f(std::false_type{}, std::false_type{});
}

// Launch of a kernel that may take more than 64 KB of dynamic LDS: the limit is raised once per kernel instantiation
// and device (one bit per device; a device index past the mask is not remembered), never on the per-launch path
template <auto Kernel, typename... Args>
int pair_launch_big_lds(uocr_ctx* ctx, dim3 grid, dim3 block, size_t lds, Args... args) {
    static std::atomic<uint64_t> raised{0};
    const uint64_t bit = ctx->device >= 0 && ctx->device < 64 ? uint64_t(1) << ctx->device : 0;
    if (!(raised.load(std::memory_order_relaxed) & bit)) {
        UOCR_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        raised.fetch_or(bit, std::memory_order_relaxed);
    }
    hipLaunchKernelGGL(Kernel, grid, block, lds, ctx->stream, args...);
    UOCR_LAUNCH_CHECK(ctx);
    return UOCR_OK;
}

}  // namespace pair_strip

// float64 sum of partial[nblocks][PAIR_NPART] -> dw1 / db1 / dw2 / db2 (x unscale, accumulate or overwrite)
int uocr_pair_strip_finish(uocr_ctx* ctx, const float* partial, float* dw1, float* db1, float* dw2, float* db2,
                           int nblocks, int use_b1, int use_b2, int accumulate, float unscale);
