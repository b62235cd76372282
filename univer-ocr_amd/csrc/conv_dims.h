// Shared between the conv translation units (generic, fast paths, MFMA implicit GEMM, API): the shape, one call record
// per direction, the ladder row and its dispatcher, and what every kernel family exports.
#pragma once
#include "uocr_common.h"

struct ConvDims { int n, h, w, cin, cout, kh, kw, sh, sw, ph, pw, oh, ow; };

// 5x5 / stride s / padding 2 with output = ceil(size / s): the shape of every small-channel conv of the page nets
// (s = 1: the same-size convs, s = 2: the encoder convs)
inline bool conv_is5x5_pad2(const ConvDims& d, int stride) {
    return d.kh == 5 && d.kw == 5 && d.sh == stride && d.sw == stride && d.ph == 2 && d.pw == 2 &&
           d.oh == (d.h + stride - 1) / stride && d.ow == (d.w + stride - 1) / stride;
}

// optional epilogue of backward-data: dx *= act'(y) evaluated from the activation OUTPUT y that is
// this conv's input tensor (same shape as dx).  Folds the backward pass of a preceding fused
// conv+LeakyReLU/Sigmoid into this kernel's store (act = UOCR_ACT_NONE: plain dx).
struct ActMask { const void* y; int act; double alpha; };

// What an entry point received, after validation.  The uocr_upconv2x_* entries (Upsample2D(2) + conv) fill the same
// records: d.h, d.w = the low-res size, d.oh = 2 d.h, d.ow = 2 d.w, 5x5, stride 1, padding 2, zero padding value.
struct ConvFwd { int dtype; ConvDims d; const void *x, *w, *b; void* y; double pad_value; int use_bias, act; double act_alpha; };
struct ConvDgrad { int dtype; ConvDims d; const void *dy, *w; void* dx; ActMask mask; };   // mask.y == nullptr <=> act NONE
struct ConvWgrad { int dtype; ConvDims d; const void *x, *dy; void *dw, *db; double pad_value; int use_bias, accumulate; };

// One rung of an entry point's ladder: a family's `takes` (the whole decision: dtype, options, shape and pointer
// alignment) and `run`, overloaded on the record.  kernel: the UOCR_CONV_* value noted when run succeeds; CONV_NOT_NOTED
// for a run that notes its own sub-kind (conv_fast.hip) and for the upconv entries, which report nothing.
template <class Call>
struct ConvRow { int kernel; bool (*takes)(uocr_ctx*, const Call&); int (*run)(uocr_ctx*, const Call&); };
constexpr int CONV_NOT_NOTED = UOCR_CONV_NONE;
template <class Call> bool uocr_conv_any_takes(uocr_ctx*, const Call&) { return true; }

// the first row that takes the call runs it (entry: 0 fwd / 1 bwd_data / 2 bwd_weight; the last row takes every call)
template <class Call, size_t N>
int uocr_conv_dispatch(uocr_ctx* ctx, int entry, const ConvRow<Call> (&rows)[N], const Call& c) {
    for (const ConvRow<Call>& r : rows)
        if (r.takes(ctx, c))
            return r.kernel == CONV_NOT_NOTED ? r.run(ctx, c) : uocr_noted_conv(ctx, entry, r.kernel, r.run(ctx, c));
    UOCR_FAIL(ctx, UOCR_ERR_UNSUPPORTED, "no conv kernel takes this call");
}

// The families, one line per record they serve: f32 MFMA implicit GEMM (gemm_mfma.hip)
bool uocr_conv_mfma_takes(uocr_ctx*, const ConvFwd&);       int uocr_conv_mfma_run(uocr_ctx*, const ConvFwd&);
bool uocr_conv_mfma_takes(uocr_ctx*, const ConvDgrad&);     int uocr_conv_mfma_run(uocr_ctx*, const ConvDgrad&);
bool uocr_conv_mfma_takes(uocr_ctx*, const ConvWgrad&);     int uocr_conv_mfma_run(uocr_ctx*, const ConvWgrad&);
// binary16-MFMA kernels of the small-channel convs, UOCR_F16 only (conv_h16.hip; weight gradients: conv_h16w.hip, the
// stride-1 and the stride-2 convs as two rungs)
bool uocr_conv_h16_takes(uocr_ctx*, const ConvFwd&);        int uocr_conv_h16_run(uocr_ctx*, const ConvFwd&);
bool uocr_conv_h16_takes(uocr_ctx*, const ConvDgrad&);      int uocr_conv_h16_run(uocr_ctx*, const ConvDgrad&);
bool uocr_conv_h16_takes(uocr_ctx*, const ConvWgrad&);      int uocr_conv_h16_run(uocr_ctx*, const ConvWgrad&);
bool uocr_conv_h16_s2_takes(uocr_ctx*, const ConvWgrad&);   int uocr_conv_h16_s2_run(uocr_ctx*, const ConvWgrad&);
// ... of upsample2x + conv; the weight gradient writes block partials for conv_up.hip's finish: *nblocks rows
bool uocr_upconv_h16_takes(uocr_ctx*, const ConvFwd&);      int uocr_upconv_h16_run(uocr_ctx*, const ConvFwd&);
bool uocr_upconv_h16_takes(uocr_ctx*, const ConvDgrad&);    int uocr_upconv_h16_run(uocr_ctx*, const ConvDgrad&);
bool uocr_upconv_wgrad_h16_takes(uocr_ctx*, const ConvWgrad&);
int uocr_upconv_wgrad_h16(uocr_ctx* ctx, const ConvWgrad& c, float* partial, size_t partial_floats, int* nblocks);
// float32 vertical-Toeplitz MFMA kernels of the small-channel convs (conv_t32.hip; weight gradients: conv_t32w.hip)
bool uocr_conv_t32_takes(uocr_ctx*, const ConvFwd&);        int uocr_conv_t32_run(uocr_ctx*, const ConvFwd&);
bool uocr_conv_t32_takes(uocr_ctx*, const ConvDgrad&);      int uocr_conv_t32_run(uocr_ctx*, const ConvDgrad&);
bool uocr_conv_t32_takes(uocr_ctx*, const ConvWgrad&);      int uocr_conv_t32_run(uocr_ctx*, const ConvWgrad&);
bool uocr_upconv_t32_takes(uocr_ctx*, const ConvDgrad&);    int uocr_upconv_t32_run(uocr_ctx*, const ConvDgrad&);
// float32 5x5 4 -> 2 forward on error-compensated binary16 MFMAs (conv_h3.hip; experiment, ctx option h3)
bool uocr_conv_h3_takes(uocr_ctx*, const ConvFwd&);         int uocr_conv_h3_run(uocr_ctx*, const ConvFwd&);
// LDS-tiled forward for the 5x5 stride-1 4-channel convs (conv_tiled.hip), f32 / f16 storage
bool uocr_conv_tiled_takes(uocr_ctx*, const ConvFwd&);      int uocr_conv_tiled_run(uocr_ctx*, const ConvFwd&);
// shape-specialised direct kernels for the skinny my_model convs (conv_fast.hip), f32 / f16 storage; run notes which
bool uocr_conv_fast_takes(uocr_ctx*, const ConvFwd&);       int uocr_conv_fast_run(uocr_ctx*, const ConvFwd&);
bool uocr_conv_fast_takes(uocr_ctx*, const ConvDgrad&);     int uocr_conv_fast_run(uocr_ctx*, const ConvDgrad&);
bool uocr_conv_fast_takes(uocr_ctx*, const ConvWgrad&);     int uocr_conv_fast_run(uocr_ctx*, const ConvWgrad&);
// generic direct kernels (conv.hip): any shape, f32 / f64; takes: uocr_conv_any_takes
int uocr_conv_generic_run(uocr_ctx*, const ConvFwd&);       int uocr_conv_generic_run(uocr_ctx*, const ConvDgrad&);
int uocr_conv_generic_run(uocr_ctx*, const ConvWgrad&);
