// Shared between the weight-gradient kernels that stage their operands as channel planes in LDS (conv_h16w.hip: binary16
// MFMAs, conv_t32w.hip: float32 MFMAs): the end of a kernel (the four waves' sums -> the block's partial row) and the
// tile of the 5x5 / stride 2 / padding 2 kernels with the tile count of their launch.
// The operand-row maps (a_off / a_ones / b0) and the scatter of the accumulators into red of the two stride-2 kernels are
// the same text in both files but stay there: as inlined helpers they compile to a differently ordered instruction
// stream in one instantiation or another.  A change to either has to be made in both files.
#pragma once
#include "conv_dims.h"

namespace {

// partial[blockIdx.x][0..NV) = the sum of the four waves' rows of red (after the barrier that follows their writes).
// (wgrad_h16_e42_kernel / e11 keep their single guarded store: NV <= 256 there, and the loop orders two instructions
// differently)
template <int NV>
__device__ __forceinline__ void write_partials(const float (&red)[4][NV], float* __restrict__ partial) {
    for (int i = threadIdx.x; i < NV; i += 256)
        partial[(size_t)blockIdx.x * NV + i] = red[0][i] + red[1][i] + red[2][i] + red[3][i];
}

// ------------------------------------------------------------------------------------------------------------
// 5x5 / stride 2 / padding 2 (the encoder convs: 4 -> 4, 1 -> 4, 1 -> 1)
//     dw[ty][tx][ci][co] = sum_{Y, X} xpad[2Y + ty - 2][2X + tx - 2][ci] * dy[Y][X][co]
// x is staged as EVEN / ODD column planes per channel (E[j] = x[2j], O[j] = x[2j+1]); with Q = X + s, s in {-1, 0, +1},
// M = (parity, ty, ci) reads its plane at Q and N = (co, sx = 1 - s) reads dy[Q + sx - 1]; a row of ones yields db.
// Strides in elements of the file's type (binary16 values or pair words / floats).
// ------------------------------------------------------------------------------------------------------------
template <int CI, int CO>
struct S2 {
    static constexpr int BR = 8, BC = 64;            // positions (Y, Q) per tile
    static constexpr int XR = 2 * BR + 3;            // x rows of a tile
    static constexpr int XRS = 72;                   // plane row stride: 68 used
    static constexpr int XP = XR * XRS + 8;          // plane stride
    static constexpr int DRS = 72;                   // dy plane row stride
    static constexpr int DP = BR * DRS + 8;          // dy plane stride
    static constexpr int NT = (10 * CI + 1 + 15) / 16;   // M tiles (the ones row included)
    static constexpr int NV = 25 * CI * CO + CO;
    static constexpr int XU = 17;                    // x staging units (8 pixels) per row: 136 >= 132 pixels
};

// the tiles of a launch: Q runs over [-1, ow]
template <int CI, int CO>
inline long s2_tiles(const ConvDims& d, int* tiles_x, int* tiles_y) {
    using G = S2<CI, CO>;
    *tiles_x = (d.ow + 2 + G::BC - 1) / G::BC, *tiles_y = (d.oh + G::BR - 1) / G::BR;
    return (long)d.n * *tiles_y * *tiles_x;
}

}  // namespace
