// Small-channel convolutions of the page nets in float32 on v_mfma_f32_16x16x4_f32: the vertical-Toeplitz
// formulation of conv_h16.hip with one float per lane and MFMA (K = 4 window rows x one element of the row).
// (reference layers: nn/layers/convolutional.py:62-145, nn/layers/upsample.py:21-39, my_model/model.py:194-247)
//
// The vector-ALU kernels of these layers (conv_fast.hip, conv_tiled.hip, conv_up.hip) run 100-400 FMAs per pixel
// at 30-45 % of the packed-FMA rate.  As an im2col GEMM the layers would use 1-4 of the 16 result columns; with
// result rows = (vertical shift dy, output channel) every lane of the MFMA result is a real output:
//       D[(dy, co), col] = sum_{ty', e} Wt[(dy, co), (ty', e)] * X[row0*S + ty'][col*S*C + e]
// e = (tap column, input channel) runs over the KW*C floats of a window row (channels-last: contiguous),
// ty' over the (DY-1)*S + KH window rows of the DY output rows.  MFMA (ib, e): k-group kq = window row 4*ib + kq.
// Executed / useful multiply-adds: 2.4x (5x5 4->2), 1.6x (its backward-data), so 25.6 / 17 us of matrix-core time
// at batch 32 x 256 x 512 where the vector kernels take 37 / 51 us.  Measured (profiles/r02_t32_*): 58 / 39 us,
// 36.7 us against 24.1 for the upsample+conv backward-data, 20 / 20 / 15 us against 28 / 17 / 10 for the 1-channel
// layers: float32 MFMAs and vector instructions do not overlap on a SIMD, so staging,
// epilogue and address arithmetic (4 vector instructions per MFMA in the backward-data kernel) add to the MFMA
// time, and with 3-6 blocks per CU the barrier-separated load / compute phases leave the matrix pipe 40 % busy.
// Since then (profiles/t32_epilogue_*.txt) the epilogue kinds are template tags, a block lives for several tiles of 16
// rows with the next tile's loads in flight, and the 4 -> 2 backward-data takes 32-33 us alone (2.7 vector instructions
// per MFMA); the forward forms were not measured again.
// Hence the default ("t32" option = 2) uses this file for the 4-channel backward-data only; the other
// instantiations stay selectable (bits 1 / 4 / 8 / 16 / 32) and tested.  Results are exact float32 FMA chains
// (the summation order differs from the reference's: tests at 1e-5 normalised, as for the other fused kernels).
// A zero weight still multiplies what the tile holds there: inputs must be finite.
// hipcc-flags: -mllvm -amdgpu-mfma-vgpr-form=1
#include "conv_toeplitz.h"

namespace {

// the geometry of conv_toeplitz.h + what float32 elements decide.  Tile height aimed at: 16 rows -- a block lives for
// several tiles (prologue paid once, the next tile's loads in flight under the chains), so small tiles cost little and
// 32 x 256 x 512 gives 4096 of them to spread over the slots
template <int C_, int COUT_, int KH_, int KW_, int S_, int MODE_, int DY_ = 0>
struct Geo : ToeplitzGeo<C_, COUT_, KH_, KW_, S_, MODE_, 16, DY_> {
    using T = ToeplitzGeo<C_, COUT_, KH_, KW_, S_, MODE_, 16, DY_>;
    using T::C, T::S, T::KW, T::IB, T::IH;
    static constexpr int Q = KW * C;                           // floats per window row
    static constexpr int NM = IB * Q;                          // MFMAs per chain
    static constexpr int BC = S == 1 ? 64 : 32;                // position columns of a block tile
    static constexpr int NCG = BC / 16;                        // chains per row band
    static constexpr int PXU = 4 / C;                          // pixels per 16-byte staging unit
    static constexpr int UW = ((BC - 1) * S * C + Q + 3) / 4;  // staging units per tile row
    // row stride in floats (a multiple of 4: 16-byte staging writes).  The 16 lanes of a k-group read 16 / 8 / 4
    // bytes each (C = 4 / 2 / 1): 4 channels: a k-group covers all banks by itself; 2 channels: the two k-groups of
    // a half wave 32 banks apart; 1 channel: the four k-groups 16 banks apart
    static constexpr int RS = C == 1 ? round_up(UW * 4 - 16, 64) + 16 : C == 2 ? round_up(UW * 4 - 32, 64) + 32 : UW * 4;
    static constexpr int RPP = 256 / UW;                       // tile rows staged per pass of the block
    static constexpr int NPASS = (IH + RPP - 1) / RPP;
    static_assert(UW <= 256 && RS >= UW * 4, "unsupported geometry");
    static_assert(RS % 4 == 0, "16-byte staging writes");
};

// the Q floats of one window row segment, with the widest aligned LDS reads the channel count allows
template <class G>
__device__ __forceinline__ void load_row(float (&bv)[G::Q], const float* p) {
    if constexpr (G::C == 4) {
#pragma unroll
        for (int j = 0; j < G::Q / 4; ++j) {
            const float4 t = *reinterpret_cast<const float4*>(p + 4 * j);
            bv[4 * j] = t.x, bv[4 * j + 1] = t.y, bv[4 * j + 2] = t.z, bv[4 * j + 3] = t.w;
        }
    } else if constexpr (G::C == 2) {
#pragma unroll
        for (int j = 0; j < G::Q / 2; ++j) {
            const float2 t = *reinterpret_cast<const float2*>(p + 2 * j);
            bv[2 * j] = t.x, bv[2 * j + 1] = t.y;
        }
    } else {
#pragma unroll
        for (int e = 0; e < G::Q; ++e) bv[e] = p[e];
    }
}

// The global loads of one input tile, pixel (iy0 + r, ix0 + c) -> unit (r, c*C ..), held in registers until tile_commit
// writes them to LDS: a block requests its next tile before the chains of the current one.  No load is conditional and
// no register is written twice (either makes hipcc wait for one row before it requests the next): a tile whose staged
// window lies wholly inside the image (`plain`, wave-uniform) loads its 16-byte units as they are; at the image's edge
// every pixel is read from its clamped position and the returned bits say which ones are image data (bit k * PXU + px;
// the others become the padding value in tile_commit).
template <class G>
__device__ __forceinline__ bool tile_plain(int strip, int trow, int h_in, int w_in, int ph, int pw) {
    const int iy0 = trow * G::BR * G::S - ph, wx0 = strip * G::BC * G::S - pw;
    return iy0 >= 0 && iy0 + G::IH <= h_in && wx0 >= 0 && wx0 + G::UW * G::PXU <= w_in;
}

template <class G>
__device__ __forceinline__ unsigned tile_fetch(float4 (&v)[G::NPASS], const float* __restrict__ in, bool plain, int strip,
                                               int trow, int img, int h_in, int w_in, int ph, int pw, int sr, int su) {
    constexpr int C = G::C, S = G::S;
    static_assert(G::NPASS * G::PXU <= 32, "one bit per staged pixel");
    const int iy0 = trow * G::BR * S - ph, gx0 = strip * G::BC * S - pw + su * G::PXU;
    const float* inb = in + (size_t)img * h_in * w_in * C;               // (h_in * w_in * C < 2^31: launch_t32)
    if (plain) {
#pragma unroll
        for (int k = 0; k < G::NPASS; ++k) {
            int gy = iy0 + sr + k * G::RPP;
            if (k * G::RPP + G::RPP > G::IH) gy = min(gy, h_in - 1);     // (rows past the tile: loaded, not stored)
            v[k] = *reinterpret_cast<const float4*>(inb + (gy * w_in + gx0) * C);       // (4-byte aligned at least)
        }
        return ~0u;
    }
    unsigned bits = 0;
    int gxc[G::PXU];
    bool in_px[G::PXU];
#pragma unroll
    for (int px = 0; px < G::PXU; ++px) {
        in_px[px] = (unsigned)(gx0 + px) < (unsigned)w_in;
        gxc[px] = min(max(gx0 + px, 0), w_in - 1) * C;
    }
#pragma unroll
    for (int k = 0; k < G::NPASS; ++k) {
        const int gy = iy0 + sr + k * G::RPP;
        const bool row_ok = (unsigned)gy < (unsigned)h_in;
        const float* src = inb + min(max(gy, 0), h_in - 1) * w_in * C;
#pragma unroll
        for (int px = 0; px < G::PXU; ++px) {
            if constexpr (C == 4) {
                v[k] = *reinterpret_cast<const float4*>(src + gxc[px]);
            } else if constexpr (C == 2) {
                const float2 t = *reinterpret_cast<const float2*>(src + gxc[px]);
                if (px == 0) v[k].x = t.x, v[k].y = t.y;
                else v[k].z = t.x, v[k].w = t.y;
            } else {
                const float t = src[gxc[px]];
                if (px == 0) v[k].x = t;
                else if (px == 1) v[k].y = t;
                else if (px == 2) v[k].z = t;
                else v[k].w = t;
            }
            bits |= (row_ok && in_px[px] ? 1u : 0u) << (k * G::PXU + px);
        }
    }
    return bits;
}

template <class G>
__device__ __forceinline__ void tile_commit(float* tile, const float4 (&v)[G::NPASS], bool plain, unsigned bits, float pad,
                                            int sr, int su) {
#pragma unroll
    for (int k = 0; k < G::NPASS; ++k) {
        const int r = sr + k * G::RPP;
        float4 t = v[k];
        if (!plain) {
            float* tf = reinterpret_cast<float*>(&t);
#pragma unroll
            for (int i = 0; i < 4; ++i) tf[i] = (bits >> (k * G::PXU + i / G::C)) & 1u ? tf[i] : pad;
        }
        if (k * G::RPP + G::RPP <= G::IH || r < G::IH) *reinterpret_cast<float4*>(tile + r * G::RS + su * 4) = t;
    }
}

// Persistent blocks over a flat tile index (image, tile row, column strip): block b takes tiles b, b + grid, ...
// A tile is BR x BC positions; wave w owns its row bands w*RPW .. w*RPW + RPW - 1 (DY rows each), NCG chains of 16
// columns per band.  What does not depend on the tile -- the zero fill, the weights, the wa[] operands, the bias -- is
// made once per block; per tile: barrier, registers -> LDS, barrier, request the next tile, chains.
//   in      [n][h_in][w_in][C]      float32
//   out     [n][h_out][w_out][COUT] float32;  mask_y (backward-data: the activation OUTPUT of the layer below, same
//           shape as out) multiplies the result by act'(y)
// ACT / MASK / BIAS: the epilogue kinds as compile-time tags (uocr_common.h), UOCR_ACT_DYN = from the arguments.
template <class G, int ACT, int MASK, int BIAS>
__global__ __launch_bounds__(256) void conv_t32_kernel(const float* __restrict__ in, const float* __restrict__ w,
                                                       const float* __restrict__ bias, float* __restrict__ out,
                                                       const float* __restrict__ mask_y, int h_in, int w_in, int h_out,
                                                       int w_out, int ph, int pw, int tiles_x, int tiles_y, int ntiles,
                                                       float pad, int use_bias, int act, float alpha, int mask_act,
                                                       float mask_alpha) {
    constexpr int C = G::C, COUT = G::COUT, S = G::S, RS = G::RS, U = G::U;
    __shared__ __attribute__((aligned(16))) float tile[G::IHA * RS];
    __shared__ float wl[G::NW];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, n = lane & 15, kq = lane >> 4;
    const int act_k = act_kind<ACT>(act), mask_k = act_kind<MASK>(mask_act);
    const bool biased = act_kind<BIAS>(use_bias) != 0, masked = mask_k != UOCR_ACT_NONE;
    // staging role of this thread: 16-byte unit su of tile rows sr, sr + RPP, ...
    const int sr = tid / G::UW, su = tid - sr * G::UW;
    const bool stager = sr < G::RPP;

    TileWalk walk(blockIdx.x, gridDim.x, tiles_x, tiles_y);
    float4 v[G::NPASS];                                  // the next tile on its way (the first one: under the prologue)
    bool plain = tile_plain<G>(walk.strip, walk.trow, h_in, w_in, ph, pw);
    unsigned bits = 0;
    if (stager) bits = tile_fetch<G>(v, in, plain, walk.strip, walk.trow, walk.img, h_in, w_in, ph, pw, sr, su);

    // the rows / floats no load ever writes must read as zero (their weights are zero, 0 * garbage is not): every tile
    // writes the same floats, so one fill serves all the tiles of the block
    for (int i = tid; i < G::IHA * RS; i += 256) tile[i] = 0.f;
    for (int i = tid; i < G::NW; i += 256) wl[i] = w[i];
    __syncthreads();

    // weight operand: row m = lane % 16 = (dy, (phase,) co), k-group kq = window row 4*ib + kq, element e of the row
    float wa[G::NM];
    {
        const int m = n, dyi = m / G::NCO, co = m % G::NCO;
#pragma unroll
        for (int ib = 0; ib < G::IB; ++ib)
#pragma unroll
            for (int e = 0; e < G::Q; ++e) {
                const int ty = 4 * ib + kq - dyi * S, tx = e / C, ci = e % C;
                const bool live = dyi < G::DY && ty >= 0 && ty < G::KH;
                wa[ib * G::Q + e] = live ? weight_of<G>(wl, min(max(ty, 0), G::KH - 1), tx, ci, co) : 0.f;
            }
    }
    float bias4[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) bias4[i] = biased ? bias[(4 * kq + i) % COUT] : 0.f;

    // where lane (column n, kq) stores: rows m = 4kq + i of a chain's result = (dy, (phase,) co).  Row and column
    // relative to the chain's first output pixel; the i / hh part is added in the epilogue (wave-uniform).
    //   4 channels: the 4 channels of one pixel; depth to space: phase = kq
    //   2 channels: rows 2kq, 2kq + 1, both channels each
    //   1 channel:  rows 4kq + i, or (depth to space) row kq, phase i
    static_assert(COUT != 2 || U == 1, "2 channels: plain store only");
    const int lrow = COUT == 4 ? (U == 2 ? kq >> 1 : kq) : COUT == 2 ? 2 * kq : (U == 2 ? 2 * kq : 4 * kq);
    const int lcol = COUT == 4 && U == 2 ? 2 * n + (kq & 1) : U * n;
    const int loff = (lrow * w_out + lcol) * COUT;       // (the bytes of BR * U + 1 output rows < 2^31: launch_t32)

    for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int strip = walk.strip, trow = walk.trow, img = walk.img;
        __syncthreads();                                 // the previous tile's reads are over
        if (stager) tile_commit<G>(tile, v, plain, bits, pad, sr, su);
        __syncthreads();
        if (t + (int)gridDim.x < ntiles) {
            walk.next(tiles_x, tiles_y);
            plain = tile_plain<G>(walk.strip, walk.trow, h_in, w_in, ph, pw);
            if (stager) bits = tile_fetch<G>(v, in, plain, walk.strip, walk.trow, walk.img, h_in, w_in, ph, pw, sr, su);
        }
        // the tile's first output pixel, and how much of the image lies below / right of it (wave-uniform)
        const size_t tile_off = ((size_t)img * h_out * w_out + (size_t)trow * (G::BR * U) * w_out + strip * (G::BC * U)) * COUT;
        float* ot = out + tile_off;                      // (wave-uniform bases and an unsigned 32-bit lane offset)
        const float* mt = masked ? mask_y + tile_off : nullptr;
        const int hrem = h_out - trow * (G::BR * U) - lrow, wrem = w_out - strip * (G::BC * U) - lcol;
        const bool whole = h_out - trow * (G::BR * U) >= G::BR * U && w_out - strip * (G::BC * U) >= G::BC * U;
        // ---- chains
#pragma unroll
        for (int s = 0; s < G::RPW; ++s) {
            const int rb = (wv * G::RPW + s) * G::DY;    // first position row of the band, relative to the tile
            // steps (chain cg, row quad ib): the B values of step s + 1 are read from LDS before the MFMAs of step s
            // are issued (the compiler orders a read right before its use otherwise, and every batch of MFMAs then
            // waits out the LDS latency)
            const float* band = tile + (rb * S + kq) * RS + n * S * C;
            // result element i of chain cg in this lane: is it an output pixel, and where (floats from ot / mt; a lane
            // without a pixel there points at the tile's first, which it may read but does not write)
            const int crow = U * rb;                     // the band's first output row relative to the tile's
            auto elem_ok = [&](int cg, int i) {
                const int irow = COUT == 4 ? 0 : COUT == 2 ? i >> 1 : (U == 2 ? i >> 1 : i);
                const int icol = COUT == 1 && U == 2 ? i & 1 : 0;
                const bool live = COUT == 4 ? U == 2 || kq < G::DY : COUT == 2 ? 2 * kq + (i >> 1) < G::DY
                                                                             : (U == 2 ? kq : 4 * kq + i) < G::DY;
                return live && (whole || (crow + irow < hrem && U * cg * 16 + icol < wrem));
            };
            auto elem_off = [&](int cg, int i) -> unsigned {
                const int coff = loff + (crow * w_out + U * cg * 16) * COUT;
                int off;
                if constexpr (COUT == 4) off = coff + i;
                else if constexpr (COUT == 2) off = coff + (i >> 1) * w_out * 2 + (i & 1);
                else off = coff + (U == 2 ? (i >> 1) * w_out + (i & 1) : i * w_out);
                return elem_ok(cg, i) ? off : 0;
            };
            // the mask values of a chain's four results, one memory instruction per run of consecutive floats,
            // requested a chain ahead: loads and stores share one in-order counter, so a wait for a mask value
            // requested after the previous chain's store would wait for that store as well
            auto mask_fetch = [&](float (&m)[4], int cg) {
                if constexpr (COUT == 4) {
                    const float4 my = *reinterpret_cast<const float4*>(mt + elem_off(cg, 0));
                    m[0] = my.x, m[1] = my.y, m[2] = my.z, m[3] = my.w;
                } else if constexpr (COUT == 2) {
#pragma unroll
                    for (int hh = 0; hh < 2; ++hh) {
                        const float2 my = *reinterpret_cast<const float2*>(mt + elem_off(cg, 2 * hh));
                        m[2 * hh] = my.x, m[2 * hh + 1] = my.y;
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i) m[i] = mt[elem_off(cg, i)];
                }
            };
            float bcur[G::Q], bnxt[G::Q], mcur[4], mnxt[4];
            if (masked) mask_fetch(mcur, 0);
            load_row<G>(bcur, band);
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int step = 0; step < G::NCG * G::IB; ++step) {
                const int cg = step / G::IB, ib = step % G::IB;
                if (step + 1 < G::NCG * G::IB) {
                    const int cg1 = (step + 1) / G::IB, ib1 = (step + 1) % G::IB;
                    load_row<G>(bnxt, band + cg1 * 16 * S * C + ib1 * 4 * RS);
                }
                if (masked && ib == 0 && cg + 1 < G::NCG) mask_fetch(mnxt, cg + 1);
#pragma unroll
                for (int e = 0; e < G::Q; ++e) acc = mfma4(wa[ib * G::Q + e], bcur[e], acc);
#pragma unroll
                for (int e = 0; e < G::Q; ++e) bcur[e] = bnxt[e];
                if (ib != G::IB - 1) continue;
                const f32x4 res = acc;
                acc = f32x4{0.f, 0.f, 0.f, 0.f};
                float r[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    r[i] = act_apply(res[i] + bias4[i], act_k, alpha);
                    if (masked) r[i] *= act_grad_from_output<float>(mcur[i], mask_k, mask_alpha);
                    if (cg + 1 < G::NCG) mcur[i] = mnxt[i];
                }
                // the results are complete here on every path: were the mask product left to sink into the branch of
                // the store, a wave that skips it would carry a pending mask load round the loop, and the wait-count
                // pass would then drain every load -- the next tile's among them -- in front of the first chain
                asm volatile("" : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]));
                if constexpr (COUT == 4) {
                    if (elem_ok(cg, 0)) *reinterpret_cast<float4*>(ot + elem_off(cg, 0)) = make_float4(r[0], r[1], r[2], r[3]);
                } else if constexpr (COUT == 2) {
#pragma unroll
                    for (int hh = 0; hh < 2; ++hh)
                        if (elem_ok(cg, 2 * hh))
                            *reinterpret_cast<float2*>(ot + elem_off(cg, 2 * hh)) = make_float2(r[2 * hh], r[2 * hh + 1]);
                } else {
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (elem_ok(cg, i)) ot[elem_off(cg, i)] = r[i];
                }
            }
        }
    }
}

// one instantiation: its residency, its grid and the launch
template <class G, int ACT, int MASK, int BIAS>
int launch_t32_kinds(uocr_ctx* ctx, const ToeplitzCall& c) {
    static int resident = 0;                             // blocks of this kernel one CU holds
    ToeplitzTiles t;
    int rc = toeplitz_tiles<G>(ctx, c, &t);
    if (rc != UOCR_OK) return rc;
    UOCR_REQUIRE(ctx, (long)(G::BR * G::U + 1) * c.w_out * G::COUT < (1l << 29));
    // one block per resident slot: at 32 x 256 x 512 a block walks two or three tiles, with its prologue paid once and
    // the next tile's loads under the chains of the current one
    int grid = 0;
    rc = uocr_persistent_grid(ctx, conv_t32_kernel<G, ACT, MASK, BIAS>, t.ntiles, 1, &resident, &grid);
    if (rc != UOCR_OK) return rc;
    hipLaunchKernelGGL((conv_t32_kernel<G, ACT, MASK, BIAS>), dim3(grid), dim3(256), 0, ctx->stream, (const float*)c.in,
                       (const float*)c.w, (const float*)c.bias, (float*)c.out, (const float*)c.mask_y, c.h_in, c.w_in,
                       c.h_out, c.w_out, c.ph, c.pw, t.tiles_x, t.tiles_y, (int)t.ntiles, c.pad, c.use_bias, c.act, c.alpha,
                       c.mask_act, c.mask_alpha);
    UOCR_LAUNCH_CHECK(ctx);
    return UOCR_OK;
}

// SIDE 0: a forward conv (bias, activation), SIDE 1: backward-data (no bias, mask).  The kinds become template tags
// here, once per launch; a pair the nets do not use, a forward conv without bias and "act_dispatch" = 0 take the
// instantiation with the dynamic tags.
template <class G, int SIDE>
int launch_t32(uocr_ctx* ctx, const ToeplitzCall& c) {
    return uocr_act_tags<SIDE>(ctx, c.act, c.mask_act, [&](auto kinds) {
        using K = decltype(kinds);
        if constexpr (!K::dynamic) {
            if ((c.use_bias != 0) == (SIDE == 0)) return launch_t32_kinds<G, K::act, K::mask, SIDE == 0>(ctx, c);
        }
        return launch_t32_kinds<G, UOCR_ACT_DYN, UOCR_ACT_DYN, UOCR_ACT_DYN>(ctx, c);
    });
}

// Bits of the "t32" option: 1 forward / 2 backward-data / 4 upsample+conv backward-data of the 4-channel layers,
// 8 / 16 / 32 the same for the 1-channel layers.
// The default library holds only what is on by default (bit 2: backward-data of the 4-channel layers); the other forms --
// measured slower in the page step, DESIGN.md section 5 -- are built with UOCR_BUILD_EXPERIMENTS=1 ./build.sh.
// bit4: the option bit of the 4-channel form (the 1-channel form's is 8 x that)
bool t32_on(uocr_ctx* ctx, int dtype, const ConvDims& d, int bit4) {
    if (dtype != UOCR_F32 || !ctx->opt_fast || d.n > 65535 || !conv_is5x5_pad2(d, 1)) return false;
    const int built = ctx->opt_t32 & UOCR_T32_BUILT;
    if (d.cin == 4 && (d.cout == 2 || d.cout == 4)) return built & bit4;
    if (d.cin == 1 && d.cout == 1) return built & (8 * bit4);
    return false;
}
bool t32_aligned(const ConvDgrad& c) {
    return uocr_aligned16(c.dy) && uocr_aligned16(c.dx) && (!c.mask.y || uocr_aligned16(c.mask.y));
}

}  // namespace

bool uocr_conv_t32_takes(uocr_ctx* ctx, const ConvFwd& c) {
    return t32_on(ctx, c.dtype, c.d, 1) && uocr_aligned16(c.x) && uocr_aligned16(c.y);
}
bool uocr_conv_t32_takes(uocr_ctx* ctx, const ConvDgrad& c) { return t32_on(ctx, c.dtype, c.d, 2) && t32_aligned(c); }

int uocr_conv_t32_run(uocr_ctx* ctx, const ConvFwd& fc) {
#ifdef UOCR_EXPERIMENTS
    const ConvDims& d = fc.d;
    const ToeplitzCall c = toeplitz_fwd_call(fc, d.ph, d.pw);
    if (d.cin == 1) return launch_t32<Geo<1, 1, 5, 5, 1, M_FWD>, 0>(ctx, c);
    if (d.cout == 2) return launch_t32<Geo<4, 2, 5, 5, 1, M_FWD>, 0>(ctx, c);
    return launch_t32<Geo<4, 4, 5, 5, 1, M_FWD>, 0>(ctx, c);
#else
    UOCR_FAIL(ctx, UOCR_ERR_UNSUPPORTED, "conv_t32 forward: library built without UOCR_BUILD_EXPERIMENTS");
#endif
}

int uocr_conv_t32_run(uocr_ctx* ctx, const ConvDgrad& dc) {
    const ConvDims& d = dc.d;
    // a forward conv over dy with flipped taps: padding kh - 1 - ph
    const ToeplitzCall c = toeplitz_dgrad_call(dc, d.kh - 1 - d.ph, d.kw - 1 - d.pw);
#ifdef UOCR_EXPERIMENTS
    if (d.cin == 1) return launch_t32<Geo<1, 1, 5, 5, 1, M_DGRAD>, 1>(ctx, c);
#endif
    if (d.cout == 2) return launch_t32<Geo<2, 4, 5, 5, 1, M_DGRAD>, 1>(ctx, c);
    return launch_t32<Geo<4, 4, 5, 5, 1, M_DGRAD>, 1>(ctx, c);
}

// backward-data of Upsample2D(2) + conv 5x5 / padding 2 (4 -> 4 or 1 -> 1 channels) on the low-res grid
bool uocr_upconv_t32_takes(uocr_ctx* ctx, const ConvDgrad& c) {
    const int built = ctx->opt_t32 & UOCR_T32_BUILT;
    return c.dtype == UOCR_F32 && ctx->opt_fast &&
           ((c.d.cin == 4 && c.d.cout == 4 && (built & 4)) || (c.d.cin == 1 && c.d.cout == 1 && (built & 32))) &&
           t32_aligned(c);
}

int uocr_upconv_t32_run(uocr_ctx* ctx, const ConvDgrad& dc) {
#ifndef UOCR_EXPERIMENTS
    UOCR_FAIL(ctx, UOCR_ERR_UNSUPPORTED, "upconv_t32: library built without UOCR_BUILD_EXPERIMENTS");
#else
    const ToeplitzCall c = toeplitz_dgrad_call(dc, 2, 2);
    if (dc.d.cin == 1) return launch_t32<Geo<1, 1, 6, 6, 2, M_UPDGRAD, 4>, 1>(ctx, c);
    return launch_t32<Geo<4, 4, 6, 6, 2, M_UPDGRAD>, 1>(ctx, c);
#endif
}
