// Shared between the vertical-Toeplitz convolution kernels (conv_h16.hip: binary16 MFMAs, conv_t32.hip: float32
// MFMAs): what a result row of the weight operand means in each mode and where its value comes from, the part of a
// kernel's geometry that does not depend on the element type, and the host side of a launch (its arguments, its tile
// grid).  tap_group also serves conv_up.hip.
#pragma once
#include "conv_dims.h"
#include "mfma.h"

namespace {

enum Mode {
    M_FWD = 0,       // forward conv, w[ky][kx][ci][co]
    M_DGRAD = 1,     // backward-data of a stride-1 conv: input dy (C = cout), flipped taps, w[ky][kx][co_out][ci_in]
    M_UPDGRAD = 2,   // backward-data of upsample2x + 5x5: stride-2 6x6 window over dy, taps summed per parity phase
    M_UPFWD = 3,     // upsample2x + 5x5 forward: 3x3 window on the low-res input, 4 phases x COUT result rows, the
                     // phases are the 2x2 output pixels of the source pixel (depth to space in the store)
    M_S2DGRAD = 4,   // backward-data of a 5x5 / stride 2 / padding 2 conv: 3x3 window over dy, result rows =
                     // (phase, ci) = the 2x2 input pixels around the source -- the same store
};

// taps k of one axis of the 5x5 kernel that land on source offset mi - 1 for output parity `phase`: [lo, hi)
// (upsample2x + conv: conv_up.hip builds its phase weights with it too)
__host__ __device__ __forceinline__ void tap_group(int phase, int mi, int& lo, int& hi) {
    if (phase == 0) {
        lo = 2 * mi;
        hi = mi == 2 ? 5 : 2 * mi + 2;
    } else {
        lo = mi == 0 ? 0 : 2 * mi - 1;
        hi = mi == 0 ? 1 : 2 * mi + 1;
    }
}

constexpr int round_up(int v, int m) { return (v + m - 1) / m * m; }

// What the binary16 and the float32 kernel agree on: an output block of 16 columns x DY position rows per MFMA chain,
// a block tile of BR position rows (BRT_ = the height aimed at), the staged window.  Each file's Geo derives from this
// and adds what depends on the element type (chunks per window row, tile width, staging units, LDS row stride).
template <int C_, int COUT_, int KH_, int KW_, int S_, int MODE_, int BRT_, int DY_>
struct ToeplitzGeo {
    static constexpr int C = C_, COUT = COUT_, KH = KH_, KW = KW_, S = S_, MODE = MODE_;
    static constexpr int U = (MODE == M_UPFWD || MODE == M_S2DGRAD) ? 2 : 1;   // output pixels per position and axis
    static constexpr int NCO = U * U * COUT;                   // result rows per position: (phase, co)
    static constexpr int DY = DY_ ? DY_ : 16 / NCO;            // position rows of one MFMA chain (fewer: zero rows)
    static constexpr int ROWS = (DY - 1) * S + KH;             // window rows of one chain
    static constexpr int IB = (ROWS + 3) / 4;                  // row quads
    static constexpr int BRT = BRT_;
    static constexpr int RPW = BRT / (4 * DY) > 0 ? BRT / (4 * DY) : 1;  // chains (row bands) per wave
    static constexpr int BR = 4 * RPW * DY;                    // position rows of a block tile
    static constexpr int IH = (BR - 1) * S + KH;               // staged input rows
    static constexpr int IHA = (BR - DY) * S + 4 * IB;         // rows a chain may address (the rest stays zero)
    static constexpr int NW = (MODE == M_UPDGRAD || MODE == M_UPFWD || MODE == M_S2DGRAD ? 25 : KH * KW) * C * COUT;
    static_assert(RPW >= 1 && 16 % NCO == 0 && DY * NCO <= 16 && (C == 1 || C == 2 || C == 4), "unsupported geometry");
};

// One launch of a Toeplitz kernel as the entry points describe it; unpacked into the kernel's arguments at the launch.
//   in  [n][h_in][w_in][C], out [n][h_out][w_out][COUT]; forward: bias / act / alpha, backward-data: mask_y (the
//   activation OUTPUT of the layer below, same shape as out) / mask_act / mask_alpha
struct ToeplitzCall {
    const void *in, *w, *bias;
    void* out;
    const void* mask_y;
    int n, h_in, w_in, h_out, w_out, ph, pw;
    float pad;
    int use_bias, act;
    float alpha;
    int mask_act;
    float mask_alpha;
};

// a forward conv: bias and activation, no mask; ph, pw: the padding of the kernel's window (upsample2x + conv: 1)
inline ToeplitzCall toeplitz_fwd_call(const ConvFwd& c, int ph, int pw) {
    return {c.x, c.w, c.b, c.y, nullptr, c.d.n, c.d.h, c.d.w, c.d.oh, c.d.ow, ph, pw, (float)c.pad_value, c.use_bias,
            c.act, (float)c.act_alpha, UOCR_ACT_NONE, 0.f};
}
// backward-data: a conv over dy (window padding ph, pw; zero padding value), no bias; dx *= act'(mask.y) if there is a mask
inline ToeplitzCall toeplitz_dgrad_call(const ConvDgrad& c, int ph, int pw) {
    return {c.dy, c.w, nullptr, c.dx, c.mask.y, c.d.n, c.d.oh, c.d.ow, c.d.h, c.d.w, ph, pw, 0.f, 0, UOCR_ACT_NONE, 0.f,
            c.mask.y ? c.mask.act : UOCR_ACT_NONE, (float)c.mask.alpha};
}

// the tile grid of a call over its position grid (U x U output pixels per position), and the size the kernels' 32-bit
// offsets inside one input image allow
struct ToeplitzTiles {
    int tiles_x, tiles_y;
    long ntiles;
};
template <class G>
inline int toeplitz_tiles(uocr_ctx* ctx, const ToeplitzCall& c, ToeplitzTiles* t) {
    const int hp = (c.h_out + G::U - 1) / G::U, wp = (c.w_out + G::U - 1) / G::U;
    t->tiles_x = (wp + G::BC - 1) / G::BC, t->tiles_y = (hp + G::BR - 1) / G::BR;
    t->ntiles = (long)c.n * t->tiles_y * t->tiles_x;
    UOCR_REQUIRE(ctx, (long)c.h_in * c.w_in * G::C < (1l << 31));
    return UOCR_OK;
}

// weight of window position (ty, tx), input channel ci, output channel co, from the layer's float32 weights
// (w = their copy in LDS: every lane builds its NM x 4 operand values from it once per block)
template <class G>
__device__ __forceinline__ float weight_of(const float* w, int ty, int tx, int ci, int co) {
    if constexpr (G::MODE == M_FWD) {
        return w[((ty * G::KW + tx) * G::C + ci) * G::COUT + co];
    } else if constexpr (G::MODE == M_DGRAD) {
        // dx[p][co] = sum dy[p + t - pad'][ci] w[K-1-t][co][ci]
        return w[(((G::KH - 1 - ty) * G::KW + (G::KW - 1 - tx)) * G::COUT + co) * G::C + ci];
    } else if constexpr (G::MODE == M_UPDGRAD) {
        // dxl[Q][co] = sum_{a,b in 0..5} dy[2Q - 2 + (a,b)][ci] Weff[phase (a%2, b%2)][o = (4 - a + py) / 2, ..][co][ci],
        // Weff = the 5x5 taps of the phase that share a source pixel (at most 2 x 2 of them), summed
        const int py = ty & 1, px = tx & 1;
        int ylo, yhi, xlo, xhi;
        tap_group(py, (4 - ty + py) >> 1, ylo, yhi);
        tap_group(px, (4 - tx + px) >> 1, xlo, xhi);
        float s = 0.f;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int ky = min(ylo + a, 4), kx = min(xlo + b, 4);
                const float v = w[((ky * 5 + kx) * G::COUT + co) * G::C + ci];
                s += (ylo + a < yhi && xlo + b < xhi) ? v : 0.f;
            }
        return s;
    } else if constexpr (G::MODE == M_UPFWD) {
        // y[2P + phase][o] = sum_{m in 3x3, ci} Weff[phase][m][ci][o] xl[P + m - 1][ci]; row co = phase * COUT + o
        const int phase = co / G::COUT, o = co % G::COUT;
        int ylo, yhi, xlo, xhi;
        tap_group(phase >> 1, ty, ylo, yhi);
        tap_group(phase & 1, tx, xlo, xhi);
        float s = 0.f;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                const int ky = min(ylo + a, 4), kx = min(xlo + b, 4);
                const float v = w[((ky * 5 + kx) * G::C + ci) * G::COUT + o];
                s += (ylo + a < yhi && xlo + b < xhi) ? v : 0.f;
            }
        return s;
    } else {
        // dx[2P + phase][c] = sum_{m in 3x3, o} dy[P + m - 1][o] w[4 - 2 m + phase][c][o] (taps beyond 4: none);
        // row co = phase * COUT + c, input channel ci = o
        const int phase = co / G::COUT, c = co % G::COUT;
        const int ky = 4 - 2 * ty + (phase >> 1), kx = 4 - 2 * tx + (phase & 1);
        const float v = w[((min(ky, 4) * 5 + min(kx, 4)) * G::COUT + c) * G::C + ci];
        return (ky <= 4 && kx <= 4) ? v : 0.f;
    }
}

}  // namespace
