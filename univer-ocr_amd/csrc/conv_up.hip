// Upsample2D(2) followed by Convolutional2D(5x5, stride 1, padding 2, zero padding value), 4 -> 4 channels,
// as ONE op on the LOW-RESOLUTION tensor (float32): the decoder blocks of the Line net
// (reference: my_model/model.py:194-247 `up_i` = nn/layers/upsample.py:21-39 + nn/layers/convolutional.py:62-145).
//
// Nearest-neighbour upsampling makes 4 high-res pixels share one source pixel, so the 5x5 window of an
// output pixel only sees a 3x3 block of source pixels, with the 25 taps summed in groups that depend on
// the output's parity phase (py, px).  Per axis, source offset m = floor((phase + k - 2) / 2):
//        phase 0: k {0,1} -> -1, {2,3} -> 0, {4} -> +1          phase 1: k {0} -> -1, {1,2} -> 0, {3,4} -> +1
//   Weff[tap m][c][(phase, o)] = sum of w[ky][kx][c][o] over the groups  (9 x 4 x 16, made by a tiny kernel)
//   y[2P + phase][o] = b[o] + sum_{m,c} Weff[m][c][(phase,o)] xl[P + m][c]
// i.e. a 3x3 convolution 4 -> 16 on the low-res tensor followed by depth-to-space: 2.8x fewer multiply-adds
// than the 5x5 on the upsampled tensor, no 4x larger intermediate (written once, read twice per step before),
// and -- 16 output columns, K = 36 -- a shape the matrix cores take without padding:
//   forward   Y^T[(phase,o), pos] = Weff^T[(phase,o), (m,c)] Xcol[(m,c), pos]      9 MFMAs (16x16x4) per 16 positions;
//             the 4 result registers of a lane are the 4 channels of ONE high-res pixel -> one 16-B store
//   dw        dWeff[(m,c), (phase,o)] += Xcol^T[(m,c), pos] dY[pos, (phase,o)]      12 MFMAs per 16 positions,
//             then dw[ky][kx] (+)= sum over the phases of the group it belongs to (finish kernel)
//   dx        dxl[Q][c] = sum_{m,(phase,o)} Weff[m][c][(phase,o)] dy[2(Q - m) + phase][o]: only 4 output columns,
//             so it stays on the vector ALU: one tap (64 weights in SGPRs) per iteration of a rolled loop,
//             dy window from an LDS tile, optional LeakyReLU' epilogue (ActMask as in conv_dims.h)
// Sums of weights first / different summation order: results agree with the layer-by-layer path to
// float32 rounding (tests: 1e-5 normalised), not bit for bit.
// hipcc-flags: -mllvm -amdgpu-mfma-vgpr-form=1
// (MFMA accumulators in VGPRs: no v_accvgpr copies between the MFMAs and the VALU code that consumes them)
#include "up_phase.h"
#include "finish_group.h"
#include "conv_toeplitz.h"

namespace {

constexpr int CH = 4;
constexpr int RH = 16, RW = 32;                 // low-res positions per tile
constexpr int XH = RH + 2, XW = RW + 2;         // xl tile: halo 1
constexpr int XPLANE = 624;                     // >= XH*XW, = 16 mod 32: the 4 channel planes of a half wave on disjoint banks
constexpr int NWEFF = 9 * CH * 16;

// weff[(m*4 + c)*16 + phase*4 + o], m = my*3 + mx, phase = py*2 + px: entry i, the sum of the taps of its group.  A group has
// at most 2 x 2 taps; all four are read from clamped indices and one outside the group adds +0.f (a sum that starts from
// +0.f is never -0.f, so that changes no bit of it).  Loops over the group's own bounds, which depend on the lane, compile
// to one waited load per trip: 36 round trips in a row for the nine entries of a forward lane when w is in global memory.
// (hipcc still moves some of the four reads behind a branch on their validity: the forward kernel reads w from LDS.)
__device__ __forceinline__ float weff_entry(const float* __restrict__ w, int i) {
    const int o = i & 3, phase = (i >> 2) & 3, c = (i >> 4) & 3, m = i >> 6;
    int ylo, yhi, xlo, xhi;
    tap_group(phase >> 1, m / 3, ylo, yhi);
    tap_group(phase & 1, m % 3, xlo, xhi);
    float v[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) v[a][b] = w[((min(ylo + a, 4) * 5 + min(xlo + b, 4)) * CH + c) * CH + o];
    float s = 0.f;
#pragma unroll
    for (int a = 0; a < 2; ++a)                         // ky ascending, then kx
#pragma unroll
        for (int b = 0; b < 2; ++b) s += (ylo + a < yhi && xlo + b < xhi) ? v[a][b] : 0.f;
    return s;
}
constexpr int NW = 25 * CH * CH;

__global__ __launch_bounds__(256) void upconv_weff_kernel(const float* __restrict__ w, float* __restrict__ weff) {
    for (int i = threadIdx.x; i < NWEFF; i += blockDim.x) weff[i] = weff_entry(w, i);
}

// xl tile (halo 1) of the region at low-res origin (ry, rx): a thread's three pixels, loaded from clamped addresses (no
// branch, so the loads go out together and can be left in flight over other work) ...
template <typename TA>
__device__ __forceinline__ void xl_tile_load(float4 (&v)[3], bool (&in)[3], const TA* __restrict__ xb, int ry, int rx,
                                             int hl, int wl, int tid) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int i = min(tid + 256 * k, XH * XW - 1);
        const int r = i / XW, c = i - r * XW;
        const int gy = ry - 1 + r, gx = rx - 1 + c;
        in[k] = gy >= 0 && gy < hl && gx >= 0 && gx < wl;
        v[k] = ld4(xb + ((size_t)min(max(gy, 0), hl - 1) * wl + min(max(gx, 0), wl - 1)) * CH);
    }
}
// ... and written channel-planar to LDS, zero outside the image
__device__ __forceinline__ void xl_tile_put(float* __restrict__ xs, const float4 (&v)[3], const bool (&in)[3], int tid) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int i = tid + 256 * k;
        if (i >= XH * XW) continue;
        const float4 u = in[k] ? v[k] : make_float4(0.f, 0.f, 0.f, 0.f);
        xs[i] = u.x;
        xs[XPLANE + i] = u.y;
        xs[2 * XPLANE + i] = u.z;
        xs[3 * XPLANE + i] = u.w;
    }
}

// forward.  Block = 16 x 32 low-res positions per tile iteration over a band of rows; wave w owns rows
// 4w..4w+3 (8 groups of 16 consecutive positions).
// (8 waves per SIMD, 64 registers: the 2048 blocks of the budget are then resident together on 256 CUs)
template <typename TA, class K>
__global__ __launch_bounds__(256, 8) void upconv_fwd_kernel(const TA* __restrict__ xl, const float* __restrict__ w,
                                                         const float* __restrict__ bias, TA* __restrict__ y,
                                                         int hl, int wl, int rows_per_block, int use_bias, int act,
                                                         float alpha, float* __restrict__ weff_out) {
    act = act_kind<K::act>(act);                 // (a constant unless the tag is dynamic: uocr_common.h)
    __shared__ float xs[CH * XPLANE];
    __shared__ float ws[512];                    // w, and copies of its last entry up to two per thread
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, n = lane & 15, kq = lane >> 4;
    const int rx = blockIdx.x * RW;
    const int row_begin = blockIdx.y * rows_per_block, row_end = min(hl, row_begin + rows_per_block);
    const TA* xb = xl + (size_t)blockIdx.z * hl * wl * CH;
    const int W = 2 * wl;
    TA* yb = y + (size_t)blockIdx.z * (2 * hl) * W * CH;
    // One batch of loads in front of the block: the 400 weights (to LDS) and the first tile.
    float wr[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) wr[k] = w[min(tid + 256 * k, NW - 1)];
    float4 xv[3];
    bool xin[3];
    xl_tile_load(xv, xin, xb, row_begin, rx, hl, wl, tid);
#pragma unroll
    for (int k = 0; k < 2; ++k) ws[tid + 256 * k] = wr[k];      // (no condition: hipcc would move the load behind it)
    xl_tile_put(xs, xv, xin, tid);
    __syncthreads();
    // the per-phase 3 x 3 weights the backward-data kernel of this layer wants (upconv_weff_kernel's table), written by
    // block 0 while it is here anyway: the caller hands the buffer back to uocr_upconv2x_bwd_data, which then needs no
    // launch of its own for them (a launch costs the lane 8-10 us inside the page step)
    if (weff_out && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0)
        for (int i = tid; i < NWEFF; i += 256) weff_out[i] = weff_entry(ws, i);
    f32x4 b4 = {0.f, 0.f, 0.f, 0.f};
    if (use_bias) b4 = f32x4{bias[0], bias[1], bias[2], bias[3]};
    // A = Weff^T: lane (m = (phase,o) = n, k = channel kq), one register per tap, summed here from the 25 taps of w (each
    // belongs to exactly one source offset for this lane's phase).  Directly in front of the tile loop: with a branch in
    // between, hipcc reads the 36 values here and adds them behind the branch (83 registers, or spills at 64).
    float wa[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) wa[t] = weff_entry(ws, (t * CH + kq) * 16 + n);
    for (int ry = row_begin; ry < row_end; ry += RH) {
        // the next tile of the band is requested before this tile's MFMAs and lands in LDS after them
        const bool more = ry + RH < row_end;
        if (more) xl_tile_load(xv, xin, xb, ry + RH, rx, hl, wl, tid);
#pragma unroll 2
        for (int k = 0; k < 8; ++k) {
            const int gi = wv * 8 + k, r = gi >> 1, c0 = (gi & 1) * 16;
            // B = Xcol: lane (k = channel kq, n = position): x at position + tap
            const float* xr = xs + kq * XPLANE + r * XW + c0 + n;
            f32x4 acc = b4;
#pragma unroll
            for (int t = 0; t < 9; ++t) acc = mfma4(wa[t], xr[(t / 3) * XW + t % 3], acc);
            // lane: phase = kq, registers = the 4 channels of high-res pixel (2P + phase)
            const int py = ry + r, pxl = rx + c0 + n;
            if (py < row_end && pxl < wl) {
                float4 out;
                out.x = act_apply(acc[0], act, alpha);
                out.y = act_apply(acc[1], act, alpha);
                out.z = act_apply(acc[2], act, alpha);
                out.w = act_apply(acc[3], act, alpha);
                st4(yb + ((size_t)(2 * py + (kq >> 1)) * W + 2 * pxl + (kq & 1)) * CH, out);
            }
        }
        if (more) {
            __syncthreads();
            xl_tile_put(xs, xv, xin, tid);
            __syncthreads();
        }
    }
}

// dw: partial[blk][48][16] (rows 36..47 unused) + partial_db[blk][4]
template <typename TA>
__global__ __launch_bounds__(256) void upconv_wgrad_kernel(const TA* __restrict__ xl, const TA* __restrict__ dy,
                                                           float* __restrict__ partial, int hl, int wl,
                                                           int rows_per_block) {
    __shared__ float xs[CH * XPLANE];
    __shared__ float red[4][48][16];
    __shared__ float reddb[4][64];
    const int tid = threadIdx.x, lane = tid & 63, n = lane & 15, kq = lane >> 4;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int rx = blockIdx.x * RW;
    const int row_begin = blockIdx.y * rows_per_block, row_end = min(hl, row_begin + rows_per_block);
    const TA* xb = xl + (size_t)blockIdx.z * hl * wl * CH;
    const int W = 2 * wl;
    const TA* gb = dy + (size_t)blockIdx.z * (2 * hl) * W * CH;
    // A = Xcol^T: lane (m = K index 16j + n -> tap K/4, channel K%4; k = position 4i + kq).  K = 36..47 read the in-range
    // offset of K = 35: those accumulator rows hold sums that no partial row reads (up4_write_row stops at K = 35).
    int aoff[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int Kc = min(16 * j + n, 35), t = Kc >> 2;
        aoff[j] = (Kc & 3) * XPLANE + (t / 3) * XW + t % 3 + kq;
    }
    // B = dY: lane (k = position 4i + kq, n = (phase, o)).  A trip of the depth loop is one low-res row of the tile (two
    // groups of 16 positions, wave w owns rows 4w..4w+3): eight loads at a wave-uniform row base plus these lane offsets,
    // clamped into the image, with the column's validity beside them.
    const int boff = ((n >> 3) * W + ((n >> 2) & 1)) * CH + (n & 3);
    int goff[2][4];
    bool gok[2][4];
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int pl = 16 * h + 4 * i + kq;          // position of this lane's K slot
            gok[h][i] = rx + pl < wl;
            goff[h][i] = boff + 2 * min(pl, wl - 1 - rx) * CH;
        }
    // the dy values of the NEXT trip (across the tile boundary: of the next tile's first trip) are requested before the
    // MFMAs of the current one and wait in registers; a row past the band is clamped into the image and counts as zero
    // (two register sets in turn: with one set and a copy, hipcc moves the loads behind the last use of the copy)
    float ga[2][4], gz[2][4];
    auto load_row = [&](float (&g)[2][4], int py) {
        const TA* gr = gb + ((size_t)(2 * min(py, hl - 1)) * W + 2 * rx) * CH;
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
            for (int i = 0; i < 4; ++i) g[h][i] = ld1(gr + goff[h][i]);
    };
    f32x4 acc[3] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    float dbacc = 0.f;
    auto trip = [&](const float (&g)[2][4], int r, bool row_ok) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float* xr = xs + r * XW + 16 * h;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float gv = row_ok && gok[h][i] ? g[h][i] : 0.f;
                dbacc += gv;
#pragma unroll
                for (int j = 0; j < 3; ++j) acc[j] = mfma4(xr[4 * i + aoff[j]], gv, acc[j]);
            }
        }
    };
    float4 xv[3];
    bool xin[3];
    xl_tile_load(xv, xin, xb, row_begin, rx, hl, wl, tid);
    // (the tile's loads first, as in the loop: loads complete in order, and where the two paths into the loop disagree
    // about which are the oldest, the wait in front of xl_tile_put becomes a wait for everything, the dy row included)
    __builtin_amdgcn_sched_barrier(0);
    load_row(ga, row_begin + wv * 4);
    for (int ry = row_begin; ry < row_end; ry += RH) {
        __syncthreads();
        xl_tile_put(xs, xv, xin, tid);
        __syncthreads();
        if (ry + RH < row_end) xl_tile_load(xv, xin, xb, ry + RH, rx, hl, wl, tid);
#pragma unroll 1
        for (int kp = 0; kp < 4; kp += 2) {
            const int r = wv * 4 + kp, py = ry + r;
            load_row(gz, py + 1);
            __builtin_amdgcn_sched_barrier(0);               // (the loads stay in front of the trip's MFMAs)
            trip(ga, r, py < row_end);
            load_row(ga, kp == 0 ? py + 2 : py + RH - 2);    // (kp == 2: the wave's first row of the next tile)
            __builtin_amdgcn_sched_barrier(0);
            trip(gz, r + 1, py + 1 < row_end);
        }
    }
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int v = 0; v < 4; ++v) red[wv][16 * j + 4 * kq + v][n] = acc[j][v];
    reddb[wv][lane] = dbacc;
    __syncthreads();
    // The block's partial row: dw and db themselves (the four phase entries of dWeff added HERE, up_phase.h), so that the
    // finish is a plain, coalesced column sum of a 404-column matrix (it used to gather four scattered entries of a
    // 580-column row per output and block: 10-13 us inside the step)
    if (tid < 4) {                                       // db[o]: lanes with (n & 3) == o
        float s = 0.f;
        for (int w = 0; w < 4; ++w) {                    // (a wave's 16 values read together, then added in lane order)
            float v[16];
#pragma unroll
            for (int k = 0; k < 16; ++k) v[k] = reddb[w][tid + 4 * k];
#pragma unroll
            for (int k = 0; k < 16; ++k) s += v[k];
        }
        reddb[0][tid] = s;                               // (read back below as entry 576 + o)
    }
    __syncthreads();
    const int blk = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    up4_write_row(partial + (size_t)blk * UP4_NOUT, [&](int i) {
        if (i >= 576) return reddb[0][i - 576];
        const int K = i >> 4, col = i & 15;
        return red[0][K][col] + red[1][K][col] + red[2][K][col] + red[3][K][col];
    }, tid, 256);
}

// out[a] (+)= unscale * (float64 column sum a of the block partials [nblocks][ncols]), a < ndw -> dw, else db.  Block = 8
// columns x 32 segments of the rows (pair_strip_finish's shape: 256 threads are schedulable inside the page step, eight
// loads in flight per thread, 32-byte coalesced segments), segments added in order.
__global__ __launch_bounds__(256) void colsum_finish_kernel(const float* __restrict__ partial, int nblocks, int ncols,
                                                            int ndw, float* __restrict__ dw, float* __restrict__ db,
                                                            int use_bias, int accumulate, float unscale) {
    constexpr int FC = 8, NSEG = 32;
    __shared__ double seg[NSEG][FC];
    const int o = threadIdx.x % FC, sg = threadIdx.x / FC, j = blockIdx.x * FC + o;
    double s = 0.0;
    if (j < ncols) {
        const int per = (nblocks + NSEG - 1) / NSEG, b0 = sg * per, b1 = min(nblocks, b0 + per);
        int b = b0;
        for (; b + 8 <= b1; b += 8) {
            float v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = partial[(size_t)(b + k) * ncols + j];
#pragma unroll
            for (int k = 0; k < 8; ++k) s += (double)v[k];
        }
        for (; b < b1; ++b) s += (double)partial[(size_t)b * ncols + j];
    }
    seg[sg][o] = s;
    __syncthreads();
    if (sg != 0 || j >= ncols) return;
#pragma unroll
    for (int k = 1; k < NSEG; ++k) s += seg[k][o];
    float* dst = j < ndw ? dw + j : db + (j - ndw);
    if (j >= ndw && !use_bias) s = 0.0;
    s *= (double)unscale;                                // UOCR_F16_SCALED(k): 2^-k, else 1
    *dst = accumulate ? (float)((double)*dst + s) : (float)s;
}

// dx on the vector ALU.  Block = 16 x 32 low-res positions, 2 per thread (rows r and r + 8); dy tile of the
// (16 + 2) x (32 + 2) source blocks = 36 x 68 high-res pixels in LDS.
constexpr int GH = 2 * (RH + 2), GW = 2 * (RW + 2);
template <typename TA, class K>
__global__ __launch_bounds__(256) void upconv_dgrad_kernel(const TA* __restrict__ dy, const float* __restrict__ weff,
                                                           TA* __restrict__ dxl, int hl, int wl,
                                                           const TA* __restrict__ mask_y, int mask_act,
                                                           float mask_alpha) {
    mask_act = act_kind<K::mask>(mask_act);                 // (a constant unless the tag is dynamic: uocr_common.h)
    __shared__ float4 gs[GH * GW];
    const int tid = threadIdx.x;
    const int rx = blockIdx.x * RW, ry = blockIdx.y * RH;
    const int H = 2 * hl, W = 2 * wl;
    const TA* gb = dy + (size_t)blockIdx.z * H * W * CH;
    if constexpr (sizeof(TA) == 4) {
        // A thread's ten pixels of the tile in ONE batch of loads from clamped addresses.  A thread past the end of the tile
        // loads and stores the last pixel again: with a condition around the store, hipcc moves that load behind the
        // condition and waits for it there, a round trip of its own after the others.
        constexpr int NK = (GH * GW + 255) / 256;
        float4 v[NK];
        bool in[NK];
#pragma unroll
        for (int k = 0; k < NK; ++k) {
            const int i = min(tid + 256 * k, GH * GW - 1);
            const int r = i / GW, c = i - r * GW;
            const int gy = 2 * (ry - 1) + r, gx = 2 * (rx - 1) + c;
            in[k] = gy >= 0 && gy < H && gx >= 0 && gx < W;
            v[k] = ld4(gb + ((size_t)min(max(gy, 0), H - 1) * W + min(max(gx, 0), W - 1)) * CH);
        }
#pragma unroll
        for (int k = 0; k < NK; ++k)
            gs[min(tid + 256 * k, GH * GW - 1)] = in[k] ? v[k] : make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
        for (int i = tid; i < GH * GW; i += 256) {
            const int r = i / GW, c = i - r * GW;
            const int gy = 2 * (ry - 1) + r, gx = 2 * (rx - 1) + c;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = ld4(gb + ((size_t)gy * W + gx) * CH);
            gs[i] = v;
        }
    }
    const int c = tid & 31, r0 = tid >> 5;               // positions (r0, c) and (r0 + 8, c)
    // the activation outputs the epilogue masks with: requested here, behind the tile's loads, so that they arrive during
    // the tap loop (position clamped into the image: a thread outside it stores nothing)
    float4 yv[2];
    if (mask_act != UOCR_ACT_NONE) {
#pragma unroll
        for (int p = 0; p < 2; ++p)
            yv[p] = ld4(mask_y + (((size_t)blockIdx.z * hl + min(ry + r0 + 8 * p, hl - 1)) * wl + min(rx + c, wl - 1)) * CH);
    }
    __syncthreads();
    float acc[2][4];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[p][j] = 0.f;
#pragma unroll 1
    for (int m = 0; m < 9; ++m) {
        const float* wt = weff + m * 64;                 // [c][phase][o]: uniform -> scalar loads
        const int my = m / 3 - 1, mx = m % 3 - 1;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int r = r0 + 8 * p;
            // source block Q - m: tile rows 2(r - my + 1) + py, cols 2(c - mx + 1) + px
            const float4* g0 = gs + (2 * (r - my + 1)) * GW + 2 * (c - mx + 1);
            const float4 g[4] = {g0[0], g0[1], g0[GW], g0[GW + 1]};
#pragma unroll
            for (int ch = 0; ch < 4; ++ch)
#pragma unroll
                for (int phase = 0; phase < 4; ++phase) {
                    const float* wv = wt + ch * 16 + phase * 4;
                    acc[p][ch] += wv[0] * g[phase].x + wv[1] * g[phase].y + wv[2] * g[phase].z + wv[3] * g[phase].w;
                }
        }
    }
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int qy = ry + r0 + 8 * p, qx = rx + c;
        if (qy >= hl || qx >= wl) continue;
        const size_t off = (((size_t)blockIdx.z * hl + qy) * wl + qx) * CH;
        float4 out = make_float4(acc[p][0], acc[p][1], acc[p][2], acc[p][3]);
        if (mask_act != UOCR_ACT_NONE) {
            out.x *= act_grad_from_output<float>(yv[p].x, mask_act, mask_alpha);
            out.y *= act_grad_from_output<float>(yv[p].y, mask_act, mask_alpha);
            out.z *= act_grad_from_output<float>(yv[p].z, mask_act, mask_alpha);
            out.w *= act_grad_from_output<float>(yv[p].w, mask_act, mask_alpha);
        }
        st4(dxl + off, out);
    }
}

// ---------------------------------------------------------------------------------------------
// 1 -> 1 channel (Paragraph decoder): 36 multiply-adds per low-res position, everything on the vector ALU;
// the kernels are bound by their HBM bytes (low-res tensor + high-res tensor) and launch latency.
// weff1[m*4 + phase], built per thread from the 25 taps (uniform loads)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void weff1_build(float (&we)[36], const float* __restrict__ w) {
#pragma unroll
    for (int m = 0; m < 9; ++m)
#pragma unroll
        for (int phase = 0; phase < 4; ++phase) {
            int ylo, yhi, xlo, xhi;
            tap_group(phase >> 1, m / 3, ylo, yhi);
            tap_group(phase & 1, m % 3, xlo, xhi);
            float s = 0.f;
            for (int ky = ylo; ky < yhi; ++ky)
                for (int kx = xlo; kx < xhi; ++kx) s += w[ky * 5 + kx];
            we[m * 4 + phase] = s;
        }
}

// block = 16 x 32 low-res positions, 2 per thread (rows r0 and r0 + 8)
template <typename TA>
__global__ __launch_bounds__(256) void up1_fwd_kernel(const TA* __restrict__ xl, const float* __restrict__ w,
                                                      const float* __restrict__ bias, TA* __restrict__ y, int hl,
                                                      int wl, int use_bias, int act, float alpha) {
    __shared__ float xs[XH * XW];
    const int tid = threadIdx.x;
    const int rx = blockIdx.x * RW, ry = blockIdx.y * RH;
    const TA* xb = xl + (size_t)blockIdx.z * hl * wl;
    stage_batched<XH * XW, 256, 3, TA>(
        tid,
        [&](int i, bool& inside) {
            const int r = i / XW, c = i - r * XW;
            const int gy = ry - 1 + r, gx = rx - 1 + c;
            inside = gy >= 0 && gy < hl && gx >= 0 && gx < wl;
            return xb + (size_t)min(max(gy, 0), hl - 1) * wl + min(max(gx, 0), wl - 1);
        },
        [&](int i, TA v, bool inside) { xs[i] = inside ? (float)v : 0.f; });
    float we[36];
    weff1_build(we, w);
    const float b0 = use_bias ? bias[0] : 0.f;
    __syncthreads();
    const int c = tid & 31, r0 = tid >> 5;
    const int W = 2 * wl;
    TA* yb = y + (size_t)blockIdx.z * (2 * hl) * W;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int r = r0 + 8 * p, py = ry + r, pxl = rx + c;
        float acc[4] = {b0, b0, b0, b0};
#pragma unroll
        for (int m = 0; m < 9; ++m) {
            const float xv = xs[(r + m / 3) * XW + c + m % 3];
#pragma unroll
            for (int phase = 0; phase < 4; ++phase) acc[phase] += xv * we[m * 4 + phase];
        }
        if (py < hl && pxl < wl) {
            TA* o = yb + (size_t)(2 * py) * W + 2 * pxl;
            st2(o, make_float2(act_apply(acc[0], act, alpha), act_apply(acc[1], act, alpha)));
            st2(o + W, make_float2(act_apply(acc[2], act, alpha), act_apply(acc[3], act, alpha)));
        }
    }
}

template <typename TA>
__global__ __launch_bounds__(256) void up1_dgrad_kernel(const TA* __restrict__ dy, const float* __restrict__ w,
                                                        TA* __restrict__ dxl, int hl, int wl,
                                                        const TA* __restrict__ mask_y, int mask_act,
                                                        float mask_alpha) {
    __shared__ float gs[GH * GW];
    const int tid = threadIdx.x;
    const int rx = blockIdx.x * RW, ry = blockIdx.y * RH;
    const int H = 2 * hl, W = 2 * wl;
    const TA* gb = dy + (size_t)blockIdx.z * H * W;
    stage_batched<GH * GW, 256, 10, TA>(
        tid,
        [&](int i, bool& inside) {
            const int r = i / GW, c = i - r * GW;
            const int gy = 2 * (ry - 1) + r, gx = 2 * (rx - 1) + c;
            inside = gy >= 0 && gy < H && gx >= 0 && gx < W;
            return gb + (size_t)min(max(gy, 0), H - 1) * W + min(max(gx, 0), W - 1);
        },
        [&](int i, TA v, bool inside) { gs[i] = inside ? (float)v : 0.f; });
    float we[36];
    weff1_build(we, w);
    __syncthreads();
    const int c = tid & 31, r0 = tid >> 5;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int r = r0 + 8 * p;
        float acc = 0.f;
#pragma unroll
        for (int m = 0; m < 9; ++m) {
            const int my = m / 3 - 1, mx = m % 3 - 1;
            const float* g0 = gs + (2 * (r - my + 1)) * GW + 2 * (c - mx + 1);   // source block Q - m
            acc += we[m * 4] * g0[0] + we[m * 4 + 1] * g0[1] + we[m * 4 + 2] * g0[GW] + we[m * 4 + 3] * g0[GW + 1];
        }
        const int qy = ry + r, qx = rx + c;
        if (qy >= hl || qx >= wl) continue;
        const size_t off = ((size_t)blockIdx.z * hl + qy) * wl + qx;
        if (mask_act != UOCR_ACT_NONE) acc *= act_grad_from_output<float>(ld1(mask_y + off), mask_act, mask_alpha);
        st1(dxl + off, acc);
    }
}

// partial[blk][37]: dWeff[m*4 + phase] and db
template <typename TA>
__global__ __launch_bounds__(256) void up1_wgrad_kernel(const TA* __restrict__ xl, const TA* __restrict__ dy,
                                                        float* __restrict__ partial, int hl, int wl,
                                                        int rows_per_block) {
    __shared__ float xs[XH * XW];
    __shared__ float red[4][37];
    const int tid = threadIdx.x;
    const int rx = blockIdx.x * RW;
    const int row_begin = blockIdx.y * rows_per_block, row_end = min(hl, row_begin + rows_per_block);
    const TA* xb = xl + (size_t)blockIdx.z * hl * wl;
    const int W = 2 * wl;
    const TA* gb = dy + (size_t)blockIdx.z * (2 * hl) * W;
    const int c = tid & 31, r0 = tid >> 5;
    float acc[36], dbacc = 0.f;
#pragma unroll
    for (int i = 0; i < 36; ++i) acc[i] = 0.f;
    for (int ry = row_begin; ry < row_end; ry += RH) {
        __syncthreads();
        stage_batched<XH * XW, 256, 3, TA>(
            tid,
            [&](int i, bool& inside) {
                const int r = i / XW, cc = i - r * XW;
                const int gy = ry - 1 + r, gx = rx - 1 + cc;
                inside = gy >= 0 && gy < hl && gx >= 0 && gx < wl;
                return xb + (size_t)min(max(gy, 0), hl - 1) * wl + min(max(gx, 0), wl - 1);
            },
            [&](int i, TA v, bool inside) { xs[i] = inside ? (float)v : 0.f; });
        __syncthreads();
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int r = r0 + 8 * p, py = ry + r, pxl = rx + c;
            if (py >= row_end || pxl >= wl) continue;
            const TA* g0 = gb + (size_t)(2 * py) * W + 2 * pxl;
            const float2 ga = ld2(g0), gbv = ld2(g0 + W);
            const float g[4] = {ga.x, ga.y, gbv.x, gbv.y};
            dbacc += (g[0] + g[1]) + (g[2] + g[3]);
#pragma unroll
            for (int m = 0; m < 9; ++m) {
                const float xv = xs[(r + m / 3) * XW + c + m % 3];
#pragma unroll
                for (int phase = 0; phase < 4; ++phase) acc[m * 4 + phase] += xv * g[phase];
            }
        }
    }
    const int lane = tid & 63, wv = tid >> 6;
#pragma unroll
    for (int i = 0; i < 36; ++i) {
        const float v = wave_reduce_sum(acc[i]);
        if (lane == 0) red[wv][i] = v;
    }
    dbacc = wave_reduce_sum(dbacc);
    if (lane == 0) red[wv][36] = dbacc;
    __syncthreads();
    const int blk = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    up1_write_row(partial + (size_t)blk * UP1_NOUT, [&](int i) { return red[0][i] + red[1][i] + red[2][i] + red[3][i]; }, tid);
}


int up_rows_per_block(int strips, int hl, int n, unsigned max_blocks = 2048u) {
    int rows = RH;
    while (rows < hl && (size_t)strips * ((hl + rows - 1) / rows) * n > max_blocks) rows += RH;
    return rows;
}

int check_up(uocr_ctx* ctx, int dtype, int n, int hl, int wl, int cin, int cout, int kh, int kw, int ph, int pw) {
    if (UOCR_DTYPE_BASE(dtype) != UOCR_F32 && UOCR_DTYPE_BASE(dtype) != UOCR_F16)
        UOCR_FAIL(ctx, UOCR_ERR_UNSUPPORTED, "upconv2x: float32 / float16 only");
    if (!((cin == CH && cout == CH) || (cin == 1 && cout == 1)) || kh != 5 || kw != 5 || ph != 2 || pw != 2)
        UOCR_FAIL(ctx, UOCR_ERR_UNSUPPORTED,
                  "upconv2x: 5x5 / padding 2 / 4 -> 4 or 1 -> 1 channels only (got %dx%d pad %d,%d %d -> %d)", kh, kw, ph,
                  pw, cin, cout);
    UOCR_REQUIRE(ctx, n > 0 && hl > 0 && wl > 0 && n <= 65535);
    return UOCR_OK;
}

ConvDims up_dims(int n, int hl, int wl, int cin, int cout) { return {n, hl, wl, cin, cout, 5, 5, 1, 1, 2, 2, 2 * hl, 2 * wl}; }   // (conv_dims.h)
int up_ncols(const ConvWgrad& c) { return c.d.cin == 1 ? UP1_NOUT : UP4_NOUT; }         // floats of a partial row

// A forward / backward-data call as the rows of this file see it: the record, and the entry's weff argument, which only
// the vector kernels use; the MFMA families get the record alone
struct UpFwd { ConvFwd call; void* weff; };
struct UpDgrad { ConvDgrad call; const void* weff; };
template <class Up> bool up_h16_takes(uocr_ctx* ctx, const Up& u) { return uocr_upconv_h16_takes(ctx, u.call); }
template <class Up> int up_h16_run(uocr_ctx* ctx, const Up& u) { return uocr_upconv_h16_run(ctx, u.call); }
bool up_t32_takes(uocr_ctx* ctx, const UpDgrad& u) { return uocr_upconv_t32_takes(ctx, u.call); }
int up_t32_run(uocr_ctx* ctx, const UpDgrad& u) { return uocr_upconv_t32_run(ctx, u.call); }

int up_fwd_vector(uocr_ctx* ctx, const UpFwd& u) {
    const ConvFwd& c = u.call;
    const int n = c.d.n, hl = c.d.h, wl = c.d.w, cin = c.d.cin;
    const int strips = (wl + RW - 1) / RW, rows = up_rows_per_block(strips, hl, n, (unsigned)uocr_budget(ctx, 2048));
    if (cin != 1) uocr_note_split(ctx, (long long)strips * ((hl + rows - 1) / rows) * n, (long long)strips * ((hl + RH - 1) / RH) * n);
    return uocr_act_tags<0>(ctx, c.act, UOCR_ACT_NONE, [&](auto kinds) -> int {
    using K = decltype(kinds);
    UOCR_DISPATCH_TA(ctx, c.dtype, {
        if (cin == 1)
            hipLaunchKernelGGL((up1_fwd_kernel<TA>), dim3((wl + RW - 1) / RW, (hl + RH - 1) / RH, n), dim3(256), 0,
                               ctx->stream, (const TA*)c.x, (const float*)c.w, (const float*)c.b, (TA*)c.y, hl, wl,
                               c.use_bias, c.act, (float)c.act_alpha);
        else
            hipLaunchKernelGGL((upconv_fwd_kernel<TA, K>), dim3(strips, (hl + rows - 1) / rows, n), dim3(256), 0,
                               ctx->stream, (const TA*)c.x, (const float*)c.w, (const float*)c.b, (TA*)c.y, hl, wl, rows,
                               c.use_bias, c.act, (float)c.act_alpha, (float*)u.weff);
    });
    UOCR_LAUNCH_CHECK(ctx);
    return UOCR_OK;
    });
}

int up_dgrad_vector(uocr_ctx* ctx, const UpDgrad& u) {
    const ConvDgrad& c = u.call;
    const int n = c.d.n, hl = c.d.h, wl = c.d.w, cin = c.d.cin;
    const float* weff = (const float*)u.weff;              // from this layer's forward call with the same w, or null
    if (cin != 1 && !weff) {
        const int rc = uocr_need_workspace(ctx, NWEFF * sizeof(float));
        if (rc != UOCR_OK) return rc;
        hipLaunchKernelGGL(upconv_weff_kernel, dim3(1), dim3(256), 0, ctx->stream, (const float*)c.w, (float*)ctx->workspace);
        weff = (const float*)ctx->workspace;
    }
    const dim3 grid((wl + RW - 1) / RW, (hl + RH - 1) / RH, n);
    return uocr_act_tags<1>(ctx, UOCR_ACT_NONE, c.mask.act, [&](auto kinds) -> int {
    using K = decltype(kinds);
    UOCR_DISPATCH_TA(ctx, c.dtype, {
        if (cin == 1)
            hipLaunchKernelGGL((up1_dgrad_kernel<TA>), grid, dim3(256), 0, ctx->stream, (const TA*)c.dy, (const float*)c.w,
                               (TA*)c.dx, hl, wl, (const TA*)c.mask.y, c.mask.act, (float)c.mask.alpha);
        else
            hipLaunchKernelGGL((upconv_dgrad_kernel<TA, K>), grid, dim3(256), 0, ctx->stream, (const TA*)c.dy,
                               weff, (TA*)c.dx, hl, wl, (const TA*)c.mask.y, c.mask.act, (float)c.mask.alpha);
    });
    UOCR_LAUNCH_CHECK(ctx);
    return UOCR_OK;
    });
}

// the block partials are rows of dw and db themselves (up_phase.h); their float64 column sums: recorded when a deferred
// group is open (finish_group.h), else one coalesced launch
int up_wgrad_finish(uocr_ctx* ctx, const ConvWgrad& c, const float* partial, int nblocks) {
    const float unscale = (float)uocr_grad_unscale(c.dtype);
    const int ncols = up_ncols(c), ndw = ncols - c.d.cin;
    const FinishDesc fd = finish_cols(partial, nblocks, ncols, ndw, (float*)c.dw, (float*)c.db, c.use_bias, c.accumulate, unscale);
    return uocr_finish(ctx, fd, [&] {
        hipLaunchKernelGGL(colsum_finish_kernel, dim3((ncols + 7) / 8), dim3(256), 0, ctx->stream, partial, nblocks,
                           ncols, ndw, (float*)c.dw, (float*)c.db, c.use_bias, c.accumulate, unscale);
    });
}

// binary16 MFMAs over channel / phase planes (conv_h16w.hip), same partial rows
int up_wgrad_h16(uocr_ctx* ctx, const ConvWgrad& c) {
    const size_t floats = (size_t)ctx->cu_count * 8 * up_ncols(c);
    int rc = UOCR_OK, nblocks = 0;
    float* partial = uocr_partial_buffer(ctx, floats * sizeof(float), &rc);
    if (rc != UOCR_OK) return rc;
    rc = uocr_upconv_wgrad_h16(ctx, c, partial, floats, &nblocks);
    return rc != UOCR_OK ? rc : up_wgrad_finish(ctx, c, partial, nblocks);
}

int up_wgrad_vector(uocr_ctx* ctx, const ConvWgrad& c) {
    const int n = c.d.n, hl = c.d.h, wl = c.d.w, cin = c.d.cin;
    // fewer, longer blocks than the forward: every block ends with a reduction and a partial row for the finish kernel
    const int strips = (wl + RW - 1) / RW, rows = up_rows_per_block(strips, hl, n, (unsigned)uocr_budget(ctx, 1024));
    const int bands = (hl + rows - 1) / rows, nblocks = strips * bands * n;
    uocr_note_split(ctx, nblocks, (long long)strips * ((hl + RH - 1) / RH) * n);       // (work items: bands of RH rows)
    int rc = UOCR_OK;
    float* partial = uocr_partial_buffer(ctx, (size_t)nblocks * up_ncols(c) * sizeof(float), &rc);
    if (rc != UOCR_OK) return rc;
    UOCR_DISPATCH_TA(ctx, c.dtype, {
        if (cin == 1)
            hipLaunchKernelGGL((up1_wgrad_kernel<TA>), dim3(strips, bands, n), dim3(256), 0, ctx->stream,
                               (const TA*)c.x, (const TA*)c.dy, partial, hl, wl, rows);
        else
            hipLaunchKernelGGL((upconv_wgrad_kernel<TA>), dim3(strips, bands, n), dim3(256), 0, ctx->stream,
                               (const TA*)c.x, (const TA*)c.dy, partial, hl, wl, rows);
    });
    UOCR_LAUNCH_CHECK(ctx);
    return up_wgrad_finish(ctx, c, partial, nblocks);
}

// The ladders of the three entries: the MFMA families first, this file's vector kernels take what is left.  These
// entries report no kernel (uocr_ctx_last_conv speaks of uocr_conv2d_* calls).
constexpr ConvRow<UpFwd> UP_FWD_ROWS[] = {{CONV_NOT_NOTED, up_h16_takes, up_h16_run},
                                          {CONV_NOT_NOTED, uocr_conv_any_takes, up_fwd_vector}};
constexpr ConvRow<UpDgrad> UP_DGRAD_ROWS[] = {{CONV_NOT_NOTED, up_h16_takes, up_h16_run},
                                              {CONV_NOT_NOTED, up_t32_takes, up_t32_run},
                                              {CONV_NOT_NOTED, uocr_conv_any_takes, up_dgrad_vector}};
constexpr ConvRow<ConvWgrad> UP_WGRAD_ROWS[] = {{CONV_NOT_NOTED, uocr_upconv_wgrad_h16_takes, up_wgrad_h16},
                                                {CONV_NOT_NOTED, uocr_conv_any_takes, up_wgrad_vector}};

}  // namespace

extern "C" int uocr_upconv2x_fwd(uocr_ctx* ctx, int dtype, const void* x_low, const void* w, const void* b, void* y,
                                 int n, int hl, int wl, int cin, int cout, int kh, int kw, int ph, int pw,
                                 int use_bias, int act, double act_alpha, void* weff) {
    UOCR_CHECK_CTX(ctx);
    UOCR_REQUIRE(ctx, x_low && w && b && y);
    int rc = check_up(ctx, dtype, n, hl, wl, cin, cout, kh, kw, ph, pw);
    if (rc != UOCR_OK) return rc;
    const ConvFwd call{dtype, up_dims(n, hl, wl, cin, cout), x_low, w, b, y, 0.0, use_bias, act, act_alpha};
    return uocr_conv_dispatch(ctx, 0, UP_FWD_ROWS, UpFwd{call, weff});
}

extern "C" int uocr_upconv2x_bwd_data(uocr_ctx* ctx, int dtype, const void* dy, const void* w, void* dx_low, int n,
                                      int hl, int wl, int cin, int cout, int kh, int kw, int ph, int pw,
                                      const void* x_act, int act, double act_alpha, const void* weff_in) {
    UOCR_CHECK_CTX(ctx);
    UOCR_REQUIRE(ctx, dy && w && dx_low);
    UOCR_REQUIRE(ctx, act == UOCR_ACT_NONE || x_act != nullptr);
    int rc = check_up(ctx, dtype, n, hl, wl, cin, cout, kh, kw, ph, pw);
    if (rc != UOCR_OK) return rc;
    const ActMask mask{act == UOCR_ACT_NONE ? nullptr : x_act, act, act_alpha};
    const ConvDgrad call{dtype, up_dims(n, hl, wl, cin, cout), dy, w, dx_low, mask};
    return uocr_conv_dispatch(ctx, 1, UP_DGRAD_ROWS, UpDgrad{call, weff_in});
}

extern "C" int uocr_upconv2x_bwd_weight(uocr_ctx* ctx, int dtype, const void* x_low, const void* dy, void* dw, void* db,
                                        int n, int hl, int wl, int cin, int cout, int kh, int kw, int ph, int pw,
                                        int use_bias, int accumulate) {
    UOCR_CHECK_CTX(ctx);
    UOCR_REQUIRE(ctx, x_low && dy && dw && db);
    int rc = check_up(ctx, dtype, n, hl, wl, cin, cout, kh, kw, ph, pw);
    if (rc != UOCR_OK) return rc;
    return uocr_conv_dispatch(ctx, 2, UP_WGRAD_ROWS,
                              ConvWgrad{dtype, up_dims(n, hl, wl, cin, cout), x_low, dy, dw, db, 0.0, use_bias, accumulate});
}
