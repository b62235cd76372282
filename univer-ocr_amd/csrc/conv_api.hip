// C-ABI entry points of Convolutional2D: argument validation, the call record (conv_dims.h) and the ordered table of
// kernel families per entry point; the first family that takes the record runs it.
#include "conv_dims.h"

namespace {

int check_dims(uocr_ctx* ctx, const ConvDims& d) {
    UOCR_REQUIRE(ctx, d.n > 0 && d.h > 0 && d.w > 0 && d.cin > 0 && d.cout > 0);
    UOCR_REQUIRE(ctx, d.kh > 0 && d.kw > 0 && d.sh > 0 && d.sw > 0 && d.ph >= 0 && d.pw >= 0);
    UOCR_REQUIRE(ctx, d.oh > 0 && d.ow > 0);
    // every window must lie inside the padded input (convolutional.py:290-301 output shape)
    UOCR_REQUIRE(ctx, (d.oh - 1) * d.sh + d.kh <= d.h + 2 * d.ph);
    UOCR_REQUIRE(ctx, (d.ow - 1) * d.sw + d.kw <= d.w + 2 * d.pw);
    return UOCR_OK;
}

// The ladders: per entry point, the kernel families in the order they are asked; generic takes what is left.
constexpr ConvRow<ConvFwd> FWD_ROWS[] = {
    {UOCR_CONV_H16, uocr_conv_h16_takes, uocr_conv_h16_run},
    {UOCR_CONV_T32, uocr_conv_t32_takes, uocr_conv_t32_run},
    {UOCR_CONV_H3, uocr_conv_h3_takes, uocr_conv_h3_run},
    {UOCR_CONV_TILED, uocr_conv_tiled_takes, uocr_conv_tiled_run},
    {CONV_NOT_NOTED, uocr_conv_fast_takes, uocr_conv_fast_run},
    {UOCR_CONV_MFMA, uocr_conv_mfma_takes, uocr_conv_mfma_run},
    {UOCR_CONV_GENERIC, uocr_conv_any_takes, uocr_conv_generic_run},
};
constexpr ConvRow<ConvDgrad> DGRAD_ROWS[] = {
    {UOCR_CONV_H16, uocr_conv_h16_takes, uocr_conv_h16_run},
    {UOCR_CONV_T32, uocr_conv_t32_takes, uocr_conv_t32_run},
    {CONV_NOT_NOTED, uocr_conv_fast_takes, uocr_conv_fast_run},
    {UOCR_CONV_MFMA, uocr_conv_mfma_takes, uocr_conv_mfma_run},
    {UOCR_CONV_GENERIC, uocr_conv_any_takes, uocr_conv_generic_run},
};
constexpr ConvRow<ConvWgrad> WGRAD_ROWS[] = {
    {UOCR_CONV_H16_WGRAD, uocr_conv_h16_takes, uocr_conv_h16_run},
    {UOCR_CONV_T32_WGRAD, uocr_conv_t32_takes, uocr_conv_t32_run},
    {UOCR_CONV_H16_WGRAD_S2, uocr_conv_h16_s2_takes, uocr_conv_h16_s2_run},
    {CONV_NOT_NOTED, uocr_conv_fast_takes, uocr_conv_fast_run},
    {UOCR_CONV_MFMA, uocr_conv_mfma_takes, uocr_conv_mfma_run},
    {UOCR_CONV_GENERIC, uocr_conv_any_takes, uocr_conv_generic_run},
};

}  // namespace

extern "C" {

int uocr_conv2d_fwd(uocr_ctx* ctx, int dtype, const void* x, const void* w, const void* b, void* y, int n, int h,
                    int wd, int cin, int cout, int kh, int kw, int sh, int sw, int ph, int pw, int oh, int ow,
                    double pad_value, int use_bias, int act, double act_alpha) {
    UOCR_CHECK_CTX(ctx);
    const ConvDims d{n, h, wd, cin, cout, kh, kw, sh, sw, ph, pw, oh, ow};
    int rc = check_dims(ctx, d);
    if (rc) return rc;
    UOCR_REQUIRE(ctx, x && w && y && (b || !use_bias));
    UOCR_REQUIRE(ctx, act >= UOCR_ACT_NONE && act <= UOCR_ACT_SIGMOID);
    return uocr_conv_dispatch(ctx, 0, FWD_ROWS, ConvFwd{dtype, d, x, w, b, y, pad_value, use_bias, act, act_alpha});
}

int uocr_conv2d_bwd_data(uocr_ctx* ctx, int dtype, const void* dy, const void* w, void* dx, int n, int h, int wd,
                         int cin, int cout, int kh, int kw, int sh, int sw, int ph, int pw, int oh, int ow,
                         const void* x_act, int act, double act_alpha) {
    UOCR_CHECK_CTX(ctx);
    const ConvDims d{n, h, wd, cin, cout, kh, kw, sh, sw, ph, pw, oh, ow};
    int rc = check_dims(ctx, d);
    if (rc) return rc;
    UOCR_REQUIRE(ctx, dy && w && dx);
    UOCR_REQUIRE(ctx, act == UOCR_ACT_NONE || (x_act && (act == UOCR_ACT_SIGMOID || (act == UOCR_ACT_LEAKY && act_alpha > 0))));
    const ActMask mask{act == UOCR_ACT_NONE ? nullptr : x_act, act, act_alpha};
    return uocr_conv_dispatch(ctx, 1, DGRAD_ROWS, ConvDgrad{dtype, d, dy, w, dx, mask});
}

int uocr_conv2d_bwd_weight(uocr_ctx* ctx, int dtype, const void* x, const void* dy, void* dw, void* db, int n, int h,
                           int wd, int cin, int cout, int kh, int kw, int sh, int sw, int ph, int pw, int oh, int ow,
                           double pad_value, int use_bias, int accumulate) {
    UOCR_CHECK_CTX(ctx);
    const ConvDims d{n, h, wd, cin, cout, kh, kw, sh, sw, ph, pw, oh, ow};
    int rc = check_dims(ctx, d);
    if (rc) return rc;
    UOCR_REQUIRE(ctx, x && dy && dw && db);
    return uocr_conv_dispatch(ctx, 2, WGRAD_ROWS, ConvWgrad{dtype, d, x, dy, dw, db, pad_value, use_bias, accumulate});
}

}  // extern "C"
