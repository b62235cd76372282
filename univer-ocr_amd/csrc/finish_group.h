// Deferred finish kernels of the weight-gradient producers (finish_group.hip).
//
// Every direct weight-gradient kernel ends in block partials [block][accumulator] (float32) and a small "finish" launch
// that adds the columns in float64 and writes dw / db.  Inside the page step even a trivial launch costs the lane that
// issues it 8-10 us (profiles/r03_*: upconv_weff_kernel, one block, 9.9 us), and the Paragraph and Line nets each have
// five of these per step.  Between uocr_wgrad_defer_begin and _flush the producers take their partial buffer from a
// region of its own (it has to survive the kernels that follow) and only RECORD their finish; the flush runs all of
// them as ONE launch: block -> (recorded finish, 8 columns), 32 row segments per column as in pair_strip_finish, then
// the column's destination by the producer's layout rule.  Same sums in the same order as the separate kernels.
#pragma once
#include "uocr_common.h"

enum : int {
    FIN_COLS = 0,      // column a -> dw[a] (a < ndw), db[a - ndw]                                  p: ndw
    FIN_TAPROWS = 1,   // [tap row][NP]: idx < NW -> dw[ky * NW + idx]; tap row 0, idx < NW + NB -> db   p: NP, NW, NB
    FIN_FAST = 2,      // conv_wgrad_fast: groups (kyg, ocg) of NP columns                          p: NP, NW, KW, CIN, COUT, KYR, COB
    FIN_PAIR = 3,      // the Monochrome pair block: dw1 (9 x 16), db1, dw2, db2 at fixed columns
};

struct FinishDesc {
    int kind;
    const float* partial;
    int nblocks;            // rows
    int ncols;              // columns, all groups
    int group_cols;         // columns per group (= ncols when the matrix is one piece)
    size_t group_stride;    // floats between the groups' matrices
    size_t row_stride;      // floats between rows
    float *dw, *db, *dw2, *db2;
    int use_bias, use_bias2, accumulate;
    float unscale;
    int p[7];
    int first_block;        // (filled in by the flush)
};

// partial buffer of `bytes` for a producer: from the deferred region when a group is open and it fits (then the finish
// MUST be offered to uocr_finish_defer), else the ctx workspace (nullptr + error code when that is too small)
float* uocr_partial_buffer(uocr_ctx* ctx, size_t bytes, int* rc);
// true: recorded -- the caller returns without launching its finish kernel
bool uocr_finish_defer(uocr_ctx* ctx, const FinishDesc& d);
void uocr_finish_defer_free(uocr_ctx* ctx);

// ---- the descriptors as their producers fill them: one [nblocks][ncols] matrix unless a builder says otherwise
inline FinishDesc finish_desc(int kind, const float* partial, int nblocks, int ncols, float* dw, float* db, int use_bias,
                              int accumulate, float unscale) {
    FinishDesc fd{};
    fd.kind = kind;
    fd.partial = partial;
    fd.nblocks = nblocks;
    fd.ncols = fd.group_cols = ncols;
    fd.row_stride = (size_t)ncols;
    fd.dw = dw, fd.db = db;
    fd.use_bias = use_bias, fd.accumulate = accumulate;
    fd.unscale = unscale;
    return fd;
}
inline FinishDesc finish_cols(const float* partial, int nblocks, int ncols, int ndw, float* dw, float* db, int use_bias,
                              int accumulate, float unscale) {
    FinishDesc fd = finish_desc(FIN_COLS, partial, nblocks, ncols, dw, db, use_bias, accumulate, unscale);
    fd.p[0] = ndw;
    return fd;
}
// five tap rows of NP columns: NW of dw, then NB of db
inline FinishDesc finish_taprows(const float* partial, int nblocks, int NP, int NW, int NB, float* dw, float* db,
                                 int use_bias, int accumulate, float unscale) {
    FinishDesc fd = finish_desc(FIN_TAPROWS, partial, nblocks, 5 * NP, dw, db, use_bias, accumulate, unscale);
    fd.p[0] = NP, fd.p[1] = NW, fd.p[2] = NB;
    return fd;
}
// ngroups matrices [nblocks][NP] one after the other; p: NP, NW, KW, CIN, COUT, KYR, COB
inline FinishDesc finish_fast(const float* partial, int nblocks, int ngroups, const int (&p)[7], float* dw, float* db,
                              int use_bias, int accumulate, float unscale) {
    FinishDesc fd = finish_desc(FIN_FAST, partial, nblocks, ngroups * p[0], dw, db, use_bias, accumulate, unscale);
    fd.group_cols = p[0];
    fd.group_stride = (size_t)nblocks * p[0];
    fd.row_stride = (size_t)p[0];
    for (int i = 0; i < 7; ++i) fd.p[i] = p[i];
    return fd;
}
inline FinishDesc finish_pair(const float* partial, int nblocks, int ncols, float* dw1, float* db1, float* dw2, float* db2,
                              int use_b1, int use_b2, int accumulate, float unscale) {
    FinishDesc fd = finish_desc(FIN_PAIR, partial, nblocks, ncols, dw1, db1, use_b1, accumulate, unscale);
    fd.dw2 = dw2, fd.db2 = db2;
    fd.use_bias2 = use_b2;
    return fd;
}

// the end of a weight-gradient launcher: the finish is recorded when a deferred group is open and takes it, else
// launch_own() launches the producer's own finish kernel
template <class F>
int uocr_finish(uocr_ctx* ctx, const FinishDesc& fd, F&& launch_own) {
    if (uocr_finish_defer(ctx, fd)) return UOCR_OK;
    launch_own();
    UOCR_LAUNCH_CHECK(ctx);
    return UOCR_OK;
}
