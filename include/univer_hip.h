/*
 * univer_hip.h -- C ABI of libuniver_hip.so, the MI355X (gfx950) backend of the
 * univer-ocr self-written deep-learning framework (KerkDovan/univer-ocr).
 *
 * The reference has no FFI: its device seam is `CP` (web_app/components/nn/gpu.py:5-29) plus the
 * per-layer closure pair `_forward_gpu/_backward_gpu` (nn/layers/layers.py:169-197), implemented
 * with CuPy and numba.cuda JIT kernels.  Every entry point below replaces one of those closures
 * (or one CuPy expression on the hot path) and cites the reference lines it stands in for.
 * Paths are relative to /root/reference/web_app/components/nn/.
 *
 * Conventions
 *  - plain pointers and sizes only; all tensor pointers are DEVICE pointers, caller-owned,
 *    C-contiguous, NHWC for images, (kh,kw,Cin,Cout) for conv weights, (n_in+1,n_out) with the
 *    bias as the LAST ROW for dense weights (layers.py:326-338);
 *  - `dtype` selects the arithmetic/storage type of every tensor argument of the call:
 *    UOCR_F32 (the production type), UOCR_F64 (the reference's own type, used by the parity
 *    and numeric-gradient tests) or UOCR_F16 (BASELINE configs[4], the HBM-bound high-resolution
 *    regime): ACTIVATION tensors (x, y, dy, dx, pred, gt, grad, activation masks) are IEEE binary16
 *    in HBM, PARAMETER tensors (w, b, dw, db, optimizer state) stay float32, every sum is
 *    accumulated in float32 (float64 for the long reductions, as in the other modes).  Activation
 *    GRADIENTS of the F16 mode carry a power-of-two scale so that Dice gradients of a 2-Mpixel page
 *    (~1e-6) do not fall below binary16's range: dtype = UOCR_F16_SCALED(k) makes the loss entry
 *    points write grad * 2^k and the bwd_weight entry points multiply dw/db by 2^-k (exact);
 *    every other entry point is linear in the gradient and ignores k (UOCR_F16 == k = 0);
 *  - every function returns 0 (UOCR_OK) or a negative UOCR_ERR_* code and never throws;
 *    uocr_last_error(ctx) returns a human readable message for the last failure on that ctx;
 *  - all work is enqueued asynchronously on the ctx's HIP stream; nothing synchronises unless
 *    its name ends in _sync.  No call allocates device memory after uocr_ctx_create /
 *    uocr_ctx_reserve_workspace, so a sequence of calls can be captured into a HIP graph;
 *  - loss scalars are written as float64 to a caller-provided device slot and fetched by the
 *    caller when it wants them (the reference does `float(loss)` = one D2H sync per loss).
 */
#ifndef UNIVER_HIP_H
#define UNIVER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UOCR_ABI_VERSION 4

typedef struct uocr_ctx uocr_ctx;

enum { UOCR_F32 = 0, UOCR_F64 = 1, UOCR_F16 = 2 };
/* F16 with activation gradients scaled by 2^k, 0 <= k <= 30 (see the conventions above) */
#define UOCR_F16_SCALED(k) (UOCR_F16 | ((k) << 8))
#define UOCR_DTYPE_BASE(dtype) ((dtype) & 0xff)
#define UOCR_DTYPE_GRAD_SCALE_LOG2(dtype) (((dtype) >> 8) & 0xff)
enum { UOCR_ACT_NONE = 0, UOCR_ACT_RELU = 1, UOCR_ACT_LEAKY = 2, UOCR_ACT_SIGMOID = 3 };
enum { UOCR_LOSS_DICE = 0, UOCR_LOSS_JACCARD = 1 };
enum {
    UOCR_OK = 0,
    UOCR_ERR_ARG = -1,         /* null pointer, negative size, inconsistent shape */
    UOCR_ERR_DTYPE = -2,       /* dtype is not UOCR_F32 / UOCR_F64 / UOCR_F16 (or F16 where a kernel has no F16 form) */
    UOCR_ERR_HIP = -3,         /* a HIP runtime call failed (see uocr_last_error) */
    UOCR_ERR_WORKSPACE = -4,   /* ctx workspace too small: call uocr_ctx_reserve_workspace */
    UOCR_ERR_UNSUPPORTED = -5, /* shape outside what the kernels implement */
    UOCR_ERR_RCCL = -6         /* librccl.so.1 missing, or an RCCL call failed (see uocr_last_error) */
};

/* ---- context, memory, events (stand in for CP / cupy, gpu.py:5-29) ------------------------- */
int uocr_abi_version(void);
int uocr_ctx_create(int device, size_t workspace_bytes, uocr_ctx** out);
/* a context whose own stream runs on a subset of the compute units (hipExtStreamCreateWithCUMask; bit i of the mask =
 * compute unit i in the driver's numbering, which deals consecutive bits round-robin over the 8 XCDs of an MI355X: bits
 * with i % 8 in a set = those whole XCDs).  Independent nets trained on concurrent lanes (PageTrainer) can be given
 * disjoint partitions; kernels that size their grid by the CU count use the partition's. */
int uocr_ctx_create_cu_mask(int device, size_t workspace_bytes, const uint32_t* cu_mask, int mask_words, uocr_ctx** out);
int uocr_ctx_destroy(uocr_ctx* ctx);
/* run on a caller-owned hipStream_t (0 = the legacy default stream) instead of the ctx's own */
int uocr_ctx_set_stream(uocr_ctx* ctx, void* hip_stream);
void* uocr_ctx_get_stream(uocr_ctx* ctx);
/* kernel selection knobs (for parity tests and A/B timing): "mfma" = 0 never / 1 auto / 2 whenever
 * eligible; "fast_paths" = 0 generic kernels only / 1 shape-specialised kernels (default);
 * "tiled" = 0 / 1 (default) LDS-tiled conv kernels where instantiated; MFMA GEMM tuning:
 * "split_blocks" (1024: split the depth until about this many blocks exist, 0 = never),
 * "split_min" (3: smallest number of slabs worth a reduce pass), "gemm_bm" (0 auto / 64 / 128 row
 * tile), "xcd_remap" (1: neighbouring tiles are numbered onto the same XCD / L2), "h16" (1: UOCR_F16
 * convolutions with 1-4 channels run on binary16 MFMAs -- the float32 weights enter the matrix cores
 * rounded to binary16, accumulation stays float32; 0: float32 vector arithmetic on the binary16 data),
 * "t32" (bit mask, default 2: which float32 small-channel convolutions use the float32-MFMA Toeplitz
 * kernels: 1 forward / 2 backward-data / 4 upsample+conv backward-data of the 4-channel layers,
 * 8 / 16 / 32 the same for 1-channel layers, 64 / 128 the float32-MFMA weight gradients of the stride-1 /
 * stride-2 5x5 convolutions -- the default library contains bit 2 only, the others need a library built with
 * UOCR_BUILD_EXPERIMENTS=1 ./build.sh and are refused with UOCR_ERR_UNSUPPORTED otherwise; likewise "h3" = 1, the
 * float32 Line output conv forward on error-compensated binary16 MFMAs); the Monochrome pair kernels:
 * "pair_band" (rows per band, 0 auto; every pair entry point), "pair_g" (4 / 2 groups of 16 columns per wave: honoured
 * by the float32 backward and by the binary16 backward of pages wider than 512 columns; both forwards and the binary16
 * backward up to 512 columns always run 4), "pair_pf" (row prefetch form of the two forward kernels, ignored by the
 * backward kernels: 0 / 1 / 2, -1 auto = form 1 in float32 and form 2 in binary16; any other value is taken as auto);
 * "wgrad_bands" (row bands per tap / channel group of the direct weight-gradient
 * kernels, 0 = 64 or 512 by the kernel's accumulator count); "max_blocks" (k > 0 lowers every block budget that is
 * decided at run time -- persistent tile walks, rows or tiles per block -- to k, so that small shapes make blocks walk
 * several tiles; it never raises one; 0 = the budgets as they are); "act_dispatch" (1 = kernels that have them take the
 * activation / mask kinds the nets use as compile-time tags, 0 = every call runs the instantiation with the run-time
 * switch: the same bits, for A/B runs).  Results do not depend on any of them beyond float32
 * summation order ("h16": beyond the binary16 rounding of the weight operands; "h3": 22 significant bits). */
int uocr_ctx_set_option(uocr_ctx* ctx, const char* key, int value);
/* the block count and the number of work items (tiles, or strips x row bands x images) of the most recent launch on
 * this ctx whose split was decided at run time (the sites "max_blocks" applies to); 0 / 0 before the first */
int uocr_ctx_last_split(uocr_ctx* ctx, int* blocks, long long* items);
/* the most recent float32 MFMA GEMM launched on this ctx (gemm_mfma.hip; "mfma", "gemm_bm", "split_blocks", "split_min",
 * "xcd_remap" steer it): its row tile (64 / 128), its grid of output tiles (gm row tiles x gn 64-column tiles) and its
 * depth slabs (1 = unsplit).  A deferred weight-gradient group flush reports bm = 64, gm = gn = 0 and nsplit = the
 * largest split of its problems; uocr_ctx_last_gemm_group gives the number of problems of that flush and how many of
 * them were split.  All 0 before the first. */
int uocr_ctx_last_gemm(uocr_ctx* ctx, int* bm, int* gm, int* gn, int* nsplit);
int uocr_ctx_last_gemm_group(uocr_ctx* ctx, int* problems, int* split_problems);
/* the most recent Monochrome pair launch accepted on this ctx (uocr_conv_pair_fwd / uocr_conv_pair_bwd on the strip
 * kernels; "pair_band", "pair_g", "pair_pf" steer it).  kernel: 1 float32 forward, 2 float32 backward, 3 binary16 forward,
 * 4 binary16 backward as one cooperative block per band (pages up to 512 columns), 5 binary16 backward on independent
 * waves; g: groups of 16 columns per wave that ran (4 / 2); mode: the masking form the host chose (0 = no position is
 * ever masked, 1 = per-position selects; 0 for kernels 3 and 5, which decide per wave); pf: the prefetch form that ran
 * (0 for the backward kernels); nw: waves per block; blocks_x x bands: the grid per image (column blocks, or blocks of
 * up to four strips, by row bands); band_h: rows per band.  A call that is refused leaves them as they were.  All 0
 * before the first. */
int uocr_ctx_last_pair(uocr_ctx* ctx, int* kernel, int* g, int* mode, int* pf, int* nw, int* blocks_x, int* bands,
                       int* band_h);
/* the kernel family that took the most recent uocr_conv2d_* call accepted on this ctx ("fast_paths", "mfma", "tiled",
 * "t32", "h16", "h3" and the alignment of the pointers steer the choice).  entry: 0 uocr_conv2d_fwd, 1 _bwd_data,
 * 2 _bwd_weight; kernel: one of UOCR_CONV_* below.  A call that is refused leaves them as they were; a weight gradient
 * recorded into a deferred group (uocr_wgrad_defer_begin) still notes its kernel.  Both 0 before the first. */
enum {
    UOCR_CONV_NONE = 0,
    UOCR_CONV_GENERIC = 1,          /* conv.hip: any shape, any dtype */
    UOCR_CONV_MFMA = 2,             /* gemm_mfma.hip: float32 implicit GEMM */
    UOCR_CONV_H16 = 3,              /* conv_h16.hip: binary16-MFMA forward / backward-data */
    UOCR_CONV_H16_WGRAD = 4,        /* conv_h16w.hip: ... weight gradient of the stride-1 5x5 convs */
    UOCR_CONV_H16_WGRAD_S2 = 5,     /* conv_h16w.hip: ... of the stride-2 5x5 convs */
    UOCR_CONV_T32 = 6,              /* conv_t32.hip: float32 vertical-Toeplitz MFMA forward / backward-data */
    UOCR_CONV_T32_WGRAD = 7,        /* conv_t32w.hip: ... weight gradients */
    UOCR_CONV_H3 = 8,               /* conv_h3.hip: float32 4 -> 2 forward on error-compensated binary16 MFMAs */
    UOCR_CONV_TILED = 9,            /* conv_tiled.hip: LDS-tiled forward of the stride-1 4-channel 5x5 convs */
    UOCR_CONV_C16_EXPAND = 10,      /* conv_fast.hip, quad-lane 3x3 kernels: 1 -> 16 forward, 16 -> 1 backward-data */
    UOCR_CONV_C16_REDUCE = 11,      /* ... 16 -> 1 forward, 1 -> 16 backward-data */
    UOCR_CONV_C16_WGRAD = 12,       /* ... weight gradient of the 16 -> 1 conv */
    UOCR_CONV_DGRAD_S2 = 13,        /* conv_fast.hip: backward-data of the 5x5 / stride 2 / padding 2 convs */
    UOCR_CONV_DGRAD_C64S2 = 14,     /* conv_fast.hip: backward-data of the 5x3 / stride (2,1) / padding (0,1) 1 -> 64 conv */
    UOCR_CONV_WGRAD_T542 = 15,      /* conv_fast.hip: LDS-tiled weight gradient of the 5x5 4 -> 2 conv */
    UOCR_CONV_WGRAD_S2_TILED = 16,  /* conv_fast.hip: LDS-tiled weight gradient of the 5x5 / stride 2 1 -> 4 conv */
    UOCR_CONV_TABLE_FAST = 17,      /* conv_fast.hip, the nine table configurations: conv_fwd_fast / conv_dgrad_fast /
                                     * conv_wgrad_fast */
    UOCR_CONV_TABLE_PX = 18         /* ... their row-loop forms conv_fwd_px / conv_dgrad_px */
};
int uocr_ctx_last_conv(uocr_ctx* ctx, int* entry, int* kernel);
int uocr_ctx_reserve_workspace(uocr_ctx* ctx, size_t bytes);   /* synchronises; not capturable */
const char* uocr_last_error(uocr_ctx* ctx);
int uocr_malloc(uocr_ctx* ctx, size_t bytes, void** out);                       /* cupy.zeros/asarray */
int uocr_free(uocr_ctx* ctx, void* ptr);
int uocr_memset_zero(uocr_ctx* ctx, void* ptr, size_t bytes);                   /* Param.clear_grad, layers.py:20-21 */
int uocr_h2d(uocr_ctx* ctx, void* dst, const void* src_host, size_t bytes);     /* CP.copy, gpu.py:19-23 */
int uocr_d2h_sync(uocr_ctx* ctx, void* dst_host, const void* src, size_t bytes);/* CP.asnumpy, gpu.py:25-29 */
int uocr_d2d(uocr_ctx* ctx, void* dst, const void* src, size_t bytes);
int uocr_stream_sync(uocr_ctx* ctx);                                            /* cuda.synchronize() */
int uocr_event_create(void** out_event);
int uocr_event_destroy(void* event);
int uocr_event_record(uocr_ctx* ctx, void* event);
/* the ctx's stream waits (on the device) for `event`, recorded on any other ctx's stream: orders lanes */
int uocr_stream_wait_event(uocr_ctx* ctx, void* event);
int uocr_event_elapsed_ms_sync(void* start, void* stop, float* out_ms);
int uocr_event_synchronize(void* event);                                        /* host waits for the event */
/* HIP-graph capture and replay of a call sequence on the ctx's stream.  The reference pays a Python dispatch and
 * a cuda.synchronize() per layer (layers/layers.py:179-197, convolutional.py:192,278); a train step recorded once
 * between begin_capture and end_capture (every entry point of this header that is not marked "not capturable" or
 * "_sync" may be called in between; no allocation happens inside the library) is replayed with one uocr_graph_launch.
 * Buffers named in the captured calls must stay allocated for the life of the graph; by-value arguments are frozen
 * (optimizer hyper-parameters that change go through the `hyper` device arrays).  Capture mode: relaxed (the caller's
 * allocator may call hipMalloc while capturing).  Other streams join a capture the HIP way: an event recorded on the
 * capturing stream and waited for with uocr_stream_wait_event. */
int uocr_graph_begin_capture(uocr_ctx* ctx);
int uocr_graph_end_capture(uocr_ctx* ctx, void** out_graph_exec);
int uocr_graph_launch(uocr_ctx* ctx, void* graph_exec);
int uocr_graph_destroy(void* graph_exec);
/* Per-step snapshots of a net's losses without a launch of their own.  The reference reads every loss on the host right
 * after the kernel that made it (losses.py:25, models.py:246-254); here losses stay in device slots that the next step
 * overwrites.  With a snapshot configured, the fused optimizer entry points (uocr_momentum_step_fused /
 * uocr_adam_step_fused: the last kernel of a train step) end by copying slots[0..count) into row (n % ring_len) of
 * ring[ring_len][count], n = the number of such calls since `counter` (one device word, zeroed by the caller) was set
 * up -- a device-side count, so a replayed HIP graph advances it by itself.  Every such call with count > 0 parameters
 * writes exactly one row (a call with no parameters launches nothing and writes none); reg_loss_out may be one of the
 * slots, the row then holds the value that call stored.  A row keeps its step's values until ring_len further calls have
 * been made, then it is overwritten without notice: the caller counts its calls and must not read a row that late.
 * slots == NULL switches it off (the counter keeps its value: configured again, the numbering goes on from there);
 * otherwise count > 0, ring != NULL, ring_len > 0 and counter != NULL, or UOCR_ERR_ARG.  Host bookkeeping only. */
int uocr_ctx_set_loss_snapshot(uocr_ctx* ctx, const double* slots, int count, double* ring, int ring_len,
                               unsigned* counter);
/* Deferred weight gradients.  The reference computes dW of a layer right where it computes dX (convolutional.py:101-145,
 * layers.py:341-347); nothing reads dW before the backward pass ends (models.py:226-254).  Between begin and flush the
 * weight-gradient GEMMs of uocr_conv2d_bwd_weight / uocr_dense_bwd(_act) that are small enough to leave the chip
 * mostly idle on their own (the Char net's, my_model/model.py:250-304) are only recorded -- the call returns at once --
 * and flush runs all of them as ONE grid and one reduction; every other call is unaffected.  Operands named in
 * recorded calls must stay valid and unchanged until the flush.  keep_open != 0: flush what is recorded and keep
 * recording (a gradient bucket must be complete now).  Same sums as the separate launches up to float32 summation
 * order (the depth splits are chosen for the group).  The problems of one group run concurrently, so a call whose dw
 * or db overlaps the dw or db of a call already recorded first flushes what is recorded, then records: calls that
 * accumulate into one gradient still add up as they would one after the other.  A group holds at most 8 problems
 * and 4 of each kind (conv / dense); a call beyond that is launched at once, outside the group. */
int uocr_wgrad_defer_begin(uocr_ctx* ctx);
int uocr_wgrad_defer_flush(uocr_ctx* ctx, int keep_open);
/* name, CU count, HBM bytes of the ctx's device (train.py:70-90 prints the numba equivalents) */
int uocr_device_info(uocr_ctx* ctx, char* name_out, size_t name_cap, int* cu_count, size_t* hbm_bytes);

/* ---- Convolutional2D (layers/convolutional.py) -------------------------------------------- */
/* y[b,oy,ox,:] = sum_{ky,kx,ic} x~[b,oy*sh-ph+ky,ox*sw-pw+kx,ic] * w[ky,kx,ic,:] (+ b if use_bias),
 * x~ = x inside, pad_value outside (convolutional.py:62-99; GPU kernel :153-195).  OH/OW follow
 * convolutional.py:290-301 and are passed explicitly.  `act` fuses a following activation layer
 * (UOCR_ACT_NONE = plain conv).  The shape-specialised kernels of conv_fast.hip's table are selected by kernel size,
 * channels and stride only: padding and pad_value are unrestricted for them (the kernels that shadow them at the nets'
 * own padding are not chosen at any other; uocr_ctx_last_conv tells which one ran). */
int uocr_conv2d_fwd(uocr_ctx* ctx, int dtype, const void* x, const void* w, const void* b, void* y,
                    int n, int h, int wd, int cin, int cout, int kh, int kw, int sh, int sw,
                    int ph, int pw, int oh, int ow, double pad_value, int use_bias,
                    int act, double act_alpha);
/* dx (unpadded input shape), overwritten (convolutional.py:101-145 dx part; GPU :203-219,239-250) */
int uocr_conv2d_bwd_data(uocr_ctx* ctx, int dtype, const void* dy, const void* w, void* dx,
                         int n, int h, int wd, int cin, int cout, int kh, int kw, int sh, int sw,
                         int ph, int pw, int oh, int ow,
                         /* optional epilogue dx *= act'(x_act): x_act = this conv's INPUT when that input is
                          * the output of a (fused) LeakyReLU / Sigmoid -- folds that layer's backward
                          * (layers.py:400-402, 412-415) into this store; act = UOCR_ACT_NONE: off */
                         const void* x_act, int act, double act_alpha);
/* dw (+)= x~^T.dy, db (+)= sum dy (only when use_bias: bias_vec = bias*ones, convolutional.py:113,125);
 * the padded border contributes pad_value to dw (:124-128; GPU :221-237).  accumulate!=0 adds
 * into dw/db (`self.w.grad += dw_total`, :137-138), 0 overwrites. */
int uocr_conv2d_bwd_weight(uocr_ctx* ctx, int dtype, const void* x, const void* dy, void* dw, void* db,
                           int n, int h, int wd, int cin, int cout, int kh, int kw, int sh, int sw,
                           int ph, int pw, int oh, int ow, double pad_value, int use_bias,
                           int accumulate);

/* The Monochrome block (my_model/model.py:108-135) as one forward and one backward kernel, float32 / UOCR_F16:
 *   y = act2( conv3x3( LeakyReLU_alpha1( conv3x3(x; w1,b1) ); w2,b2 ) ),  x,y: (n,h,w,1), w1: (3,3,1,16),
 *   w2: (3,3,16,1), both convs stride 1 / padding 1 (convolutional.py:62-99 twice + layers.py:377-418),
 *   conv_2's padding value 0.  The 16-channel activation and its gradient are recomputed in registers /
 *   LDS instead of crossing HBM.  act2 = UOCR_ACT_NONE or UOCR_ACT_SIGMOID.
 * bwd: dy = gradient w.r.t. y (AFTER act2; the kernel multiplies by act2'(y)); dw/db as
 *   uocr_conv2d_bwd_weight (accumulate!=0 adds), dx may be NULL (page-input gradient not wanted).
 * UOCR_ERR_UNSUPPORTED for float64, cmid != 16 or a LeakyReLU slope outside [0, 1] (the kernels take it as
 * max(z, alpha z)): the caller then runs the layers one by one. */
int uocr_conv_pair_fwd(uocr_ctx* ctx, int dtype, const void* x, const void* w1, const void* b1,
                       const void* w2, const void* b2, void* y, int n, int h, int wd, int cmid,
                       double pad_value1, int use_bias1, int use_bias2, double alpha1, int act2);
int uocr_conv_pair_bwd(uocr_ctx* ctx, int dtype, const void* x, const void* y, const void* dy,
                       const void* w1, const void* b1, const void* w2, void* dw1, void* db1, void* dw2,
                       void* db2, void* dx, int n, int h, int wd, int cmid, double pad_value1,
                       int use_bias1, int use_bias2, double alpha1, int act2, int accumulate);

/* Upsample2D(2) + Convolutional2D(5x5, stride 1, padding 2, padding value 0, 4 -> 4 channels) as one op on
 * the LOW-RES tensor x_low (n,hl,wl,4) -> y (n,2hl,2wl,4): the decoder blocks `up_i` of the Line net
 * (my_model/model.py:194-247 = upsample.py:21-39 + convolutional.py:62-145).  Each output parity phase sees
 * a 3x3 block of source pixels with the 5x5 taps summed in groups, so the upsampled tensor is never built
 * (float32; results equal the two-layer path to rounding, not bit for bit).  Arguments as uocr_conv2d_*,
 * with hl, wl the LOW-RES size; bwd_data returns the gradient w.r.t. x_low (= upsample backward of the conv's
 * dx).  UOCR_ERR_UNSUPPORTED for any other shape or dtype: the caller then runs the two layers. */
/* weff (may be NULL): 576 floats owned by the caller.  The float32 4-channel forward writes the per-phase 3 x 3 weights
 * there; handed to bwd_data of the same layer while w is unchanged (the same train step), it saves that call a launch. */
int uocr_upconv2x_fwd(uocr_ctx* ctx, int dtype, const void* x_low, const void* w, const void* b, void* y,
                      int n, int hl, int wl, int cin, int cout, int kh, int kw, int ph, int pw,
                      int use_bias, int act, double act_alpha, void* weff);
int uocr_upconv2x_bwd_data(uocr_ctx* ctx, int dtype, const void* dy, const void* w, void* dx_low,
                           int n, int hl, int wl, int cin, int cout, int kh, int kw, int ph, int pw,
                           const void* x_act, int act, double act_alpha, const void* weff);
int uocr_upconv2x_bwd_weight(uocr_ctx* ctx, int dtype, const void* x_low, const void* dy, void* dw, void* db,
                             int n, int hl, int wl, int cin, int cout, int kh, int kw, int ph, int pw,
                             int use_bias, int accumulate);

/* ---- MaxPool2D (layers/maxpool.py; the NumPy path :24-90 is the semantics) ---------------- */
/* y = window max with zero padding; mask (uint8, shape (n, kh*oh, kw*ow, c), window-major) marks
 * every element equal to the max; windows running past the padded extent (ceil_mode) shrink. */
int uocr_maxpool2d_fwd(uocr_ctx* ctx, int dtype, const void* x, void* y, uint8_t* mask,
                       int n, int h, int wd, int c, int kh, int kw, int sh, int sw, int ph, int pw,
                       int oh, int ow);
/* dx[b,y,x,c] = sum over windows containing (y,x) with mask set of dy/ties (maxpool.py:62-90) */
int uocr_maxpool2d_bwd(uocr_ctx* ctx, int dtype, const void* dy, const uint8_t* mask, void* dx,
                       int n, int h, int wd, int c, int kh, int kw, int sh, int sw, int ph, int pw,
                       int oh, int ow);

/* ---- Upsample2D (layers/upsample.py:21-110) ----------------------------------------------- */
int uocr_upsample2d_fwd(uocr_ctx* ctx, int dtype, const void* x, void* y,
                        int n, int h, int wd, int c, int sy, int sx);
int uocr_upsample2d_bwd(uocr_ctx* ctx, int dtype, const void* dy, void* dx,
                        int n, int h, int wd, int c, int sy, int sx);   /* h,wd = INPUT (dx) size */

/* ---- Relu / LeakyRelu / Sigmoid (layers/layers.py:377-418) -------------------------------- */
int uocr_act_fwd(uocr_ctx* ctx, int dtype, int kind, double alpha, const void* x, void* y, size_t count);
/* x = the layer's stashed INPUT (the reference stashes the mask / X, layers.py:379,396,409) */
int uocr_act_bwd(uocr_ctx* ctx, int dtype, int kind, double alpha, const void* x, const void* dy,
                 void* dx, size_t count);

/* same gradient computed from the layer's OUTPUT y (conv + activation fused: the pre-activation is
 * never stored).  kind = UOCR_ACT_LEAKY (alpha > 0: sign(y) == sign(x)) or UOCR_ACT_SIGMOID (y(1-y)) */
int uocr_act_bwd_from_output(uocr_ctx* ctx, int dtype, int kind, double alpha, const void* y, const void* dy,
                             void* dx, size_t count);

/* ---- FullyConnected (layers/layers.py:307-363) -------------------------------------------- */
int uocr_dense_fwd(uocr_ctx* ctx, int dtype, const void* x, const void* w, void* y,
                   int m, int n_in, int n_out);
/* dx = dy . w[:-1]^T ; dw (+)= [x,1]^T . dy ; dx or dw may be NULL to skip it (the two halves may then run on
 * different ctx: the weight gradient is off the critical path of a backward pass) */
int uocr_dense_bwd(uocr_ctx* ctx, int dtype, const void* x, const void* w, const void* dy,
                   void* dx, void* dw, int m, int n_in, int n_out, int accumulate);
/* FullyConnected followed by LeakyRelu / Sigmoid (my_model/model.py:250-304: dense_1, dense_2) as one
 * GEMM: y = act([x,1] . w) (layers.py:335-339 + :377-418); and the backward of a layer whose input x IS such an
 * activation's output: dx = (dy . w[:-1]^T) * act'(x), act' taken from the output as in uocr_act_bwd_from_output */
int uocr_dense_fwd_act(uocr_ctx* ctx, int dtype, const void* x, const void* w, void* y,
                       int m, int n_in, int n_out, int act, double act_alpha);
int uocr_dense_bwd_act(uocr_ctx* ctx, int dtype, const void* x, const void* w, const void* dy,
                       void* dx, void* dw, int m, int n_in, int n_out, int accumulate,
                       int x_act, double x_act_alpha);

/* ---- Conv2DToBatchedFixedWidthed (layers/convolutional.py:330-373) ------------------------ */
int uocr_fixed_width_fwd(uocr_ctx* ctx, int dtype, const void* x, void* y,
                         int n, int h, int wd, int c, int width);
int uocr_fixed_width_bwd(uocr_ctx* ctx, int dtype, const void* dy, void* dx,
                         int n, int h, int wd, int c, int width);

/* ---- Concat / fan-out sums / fills (layers.py:240-284; models.py:218) --------------------- */
/* dst[r*dst_ld + c] = src[r*src_ld + c], r<rows, c<cols (element strides): one call per Concat input */
int uocr_copy_2d(uocr_ctx* ctx, int dtype, void* dst, size_t dst_ld, const void* src, size_t src_ld,
                 size_t rows, size_t cols);
int uocr_add(uocr_ctx* ctx, int dtype, const void* a, const void* b, void* out, size_t count);
int uocr_axpy(uocr_ctx* ctx, int dtype, double alpha, const void* x, void* y, size_t count); /* y += alpha*x */
int uocr_scale(uocr_ctx* ctx, int dtype, double alpha, void* x, size_t count);
int uocr_fill(uocr_ctx* ctx, int dtype, void* x, double value, size_t count);
int uocr_convert(uocr_ctx* ctx, int src_dtype, const void* src, int dst_dtype, void* dst, size_t count);
/* dst = u8 * scale (page images arrive as uint8, datasets.py:16-19 divides by 255) */
int uocr_u8_to_float(uocr_ctx* ctx, int dtype, const uint8_t* src, void* dst, double scale, size_t count);

/* ---- losses (losses.py) : grad tensor + float64 loss scalar at *loss_out (device) --------- */
/* out_act = UOCR_ACT_SIGMOID: pred is the output of a Sigmoid layer (layers.py:407-418) and grad is taken
 * w.r.t. that layer's INPUT (its backward folded in); UOCR_ACT_NONE: grad w.r.t. pred (losses.py:24,41) */
int uocr_seg_loss(uocr_ctx* ctx, int dtype, int kind /*UOCR_LOSS_DICE|JACCARD*/, const void* pred,
                  const void* gt, void* grad /*may be NULL*/, double* loss_out,
                  int n, int hw, int c, int out_act);                                   /* losses.py:9-42 */
int uocr_softmax_ce(uocr_ctx* ctx, int dtype, const void* pred, const void* gt, void* grad /*may be NULL*/,
                    double* loss_out, int m, int c);                       /* losses.py:60-73 */
int uocr_sigmoid_ce(uocr_ctx* ctx, int dtype, const void* pred, const void* gt, void* grad /*may be NULL*/,
                    double* loss_out, int m, size_t count);                /* losses.py:45-57 */

/* ---- regularizers (regularizations.py:15-26, applied at layers.py:147-155) ----------------- */
/* grad += d/dw, *loss_out (+)= strength*sum(...)  (accumulate_loss=0 overwrites the slot) */
int uocr_l2_reg(uocr_ctx* ctx, int dtype, const void* w, void* grad, size_t count, double strength,
                double* loss_out, int accumulate_loss);
int uocr_l1_reg(uocr_ctx* ctx, int dtype, const void* w, void* grad, size_t count, double strength,
                double* loss_out, int accumulate_loss);

/* ---- optimizers (optimizers.py:47-98), fused in-place updates ------------------------------ */
/* v=b1*v+(1-b1)g; a=b2*a+(1-b2)g^2; w-=lr/(sqrt(a)+eps)*v   -- NO bias correction (:56-61) */
int uocr_adam_step(uocr_ctx* ctx, int dtype, void* w, const void* g, void* v, void* a, size_t count,
                   double lr, double beta1, double beta2, double eps);
/* v=mu*v-lr*g; w+=v  (:75-78; mu=0 is plain SGD) */
int uocr_momentum_step(uocr_ctx* ctx, int dtype, void* w, const void* g, void* v, size_t count,
                       double lr, double momentum);
/* a=rho*a+(1-rho)g^2; w-=lr/(sqrt(a)+eps)*g  (:92-95) */
/* The tail of a train step in one pass over the flat parameter buffer: for up to 4 index ranges [lo, hi)
 * grad += dR/dw (kind 1 = L1, 2 = L2: regularizations.py:15-26 as applied in layers.py:147-155), then the
 * Momentum update (optimizers.py:75-78), then grad = 0 when zero_grad (Param.clear_grad, layers.py:20-21);
 * *reg_loss_out = sum_r strength_r * R_r (float64 device slot).  lo / hi / kind / strength are HOST arrays. */
int uocr_momentum_step_fused(uocr_ctx* ctx, int dtype, void* w, void* g, void* v, size_t count, double lr,
                             double momentum, int nranges, const long long* lo, const long long* hi,
                             const int* kind, const double* strength, double* reg_loss_out, int zero_grad,
                             /* optional DEVICE array {lr, momentum, -, -}: when given the kernel reads the
                              * hyper-parameters from it instead of the by-value arguments, so a call captured in
                              * a HIP graph follows the trainer's learning-rate decay (my_model/trainer.py:260);
                              * NULL = use the arguments */
                             const double* hyper_dev);
/* the same with the Adam update of optimizers.py:56-61 (no bias correction, as the reference) */
int uocr_adam_step_fused(uocr_ctx* ctx, int dtype, void* w, void* g, void* v, void* a, size_t count, double lr,
                         double beta1, double beta2, double eps, int nranges, const long long* lo,
                         const long long* hi, const int* kind, const double* strength, double* reg_loss_out,
                         int zero_grad, const double* hyper_dev /* {lr, beta1, beta2, eps} on the device, or NULL */);
int uocr_rmsprop_step(uocr_ctx* ctx, int dtype, void* w, const void* g, void* a, size_t count,
                      double lr, double rho, double eps);
/* *flag_out (int32, device) = 1 if any element is NaN else 0  (nan_weights, layers.py:139-140) */
int uocr_has_nan(uocr_ctx* ctx, int dtype, const void* x, size_t count, int32_t* flag_out);

/* ---- connected components and masked crops (interpreter/interpreter.py: the ParagraphCrop stage) ---------
 * uocr_label_components replaces label_layer (interpreter.py:16-21: ndimage.label(layer > np.mean(layer))), the
 * thresholds of :437-438 and :549 (0.5 * (mean + max)) and ndimage.find_objects / center_of_mass (:303, :36-39).
 * x: (n, h, w, 1) in `dtype`; foreground is x > t with t chosen by thresh_mode (mean and max are float64 reductions over
 * the WHOLE tensor; thresh_value is read for UOCR_THRESH_VALUE only).  Connectivity is scipy's default structure (four
 * edge neighbours in the h-w plane).  Every image is labelled on its own: for n = 1 exactly the reference's result (its
 * 4-D call would also join equal pixels of neighbouring images; its data path only has n = 1, datasets.py:18,39).
 * labels: int32 (n, h, w), 0 = background, the components of image i numbered 1..count[i] in the order of their first
 * pixel in row-major order (scipy's numbering).  table: int64 [n][max_components][8], entry k-1 of image i =
 * {linear index of the component's first pixel, area, y0, y1, x0, x1, sum of y, sum of x} with half-open boxes equal to
 * find_objects' slices (centre of mass = sums / area); entries past count[i] are zero.  count[i] is the true number of
 * components even when it exceeds max_components: the table then holds the first max_components, the labels stay
 * complete.  Scratch (one int32 per pixel and a little more) comes from the ctx workspace (UOCR_ERR_WORKSPACE).
 * Integer atomics only: results are bit-identical run to run.  Asynchronous and capturable. */
enum { UOCR_THRESH_MEAN = 0, UOCR_THRESH_MEAN_MAX = 1, UOCR_THRESH_VALUE = 2 };
int uocr_label_components(uocr_ctx* ctx, int dtype, const void* x, int n, int h, int w, int thresh_mode,
                          double thresh_value, int* labels, long long* table, int max_components, int* count);
/* (image * mask)[:, ry, rx, :] of interpreter.py:304-308 followed by make_divisible_by's zero frame (my_model/model.py:
 * 26-34) in one pass.  image: (n, h, w, c) in `dtype`, labels as written by uocr_label_components; the box [y0, y0 + ch)
 * x [x0, x0 + cw) of image `image_index` is copied where labels == label_id and zeroed elsewhere, and placed in out
 * (1, out_h, out_w, c) at row (out_h - ch) / 2, column (out_w - cw) / 2 -- where make_divisible_by puts it when out_h =
 * ch + 16 - ch % 16; at (0, 0) when out has the box's size.  Every element of out is written (zero outside the box).
 * UOCR_ERR_ARG for a box outside the image, out smaller than the box, image_index outside [0, n) or label_id < 1;
 * nothing is written then. */
int uocr_masked_crop(uocr_ctx* ctx, int dtype, const void* image, const int* labels, int n, int h, int w, int c,
                     int image_index, int label_id, int y0, int x0, int ch, int cw, void* out, int out_h, int out_w);
/* the tile (rows, columns) of the last uocr_label_components call on this ctx and the kernels it launched (all 0 before the
 * first): tests size their images from it so that components cross tile borders */
int uocr_ctx_last_label(uocr_ctx* ctx, int* tile_h, int* tile_w, int* launches);
/* Connected components of a LIST of images of different sizes, every image one channel of an interleaved tensor, in one
 * call (interpreter.py:437-438, :16-21, :36-39, :494-502 for every paragraph of a page at once).  Entry i is channel
 * channel[i] of x[i]: (1, h[i], w[i], c[i]) in `dtype`, read in place -- pixel (y, x) is the element at
 * (y * w + x) * c + channel; no split copy is made.  Foreground is value > t, t chosen PER ENTRY by thresh_mode as in
 * uocr_label_components: mean and max are float64 reductions over the h * w elements of that entry's channel only, not
 * over its other channels and not over the call.  The summation order is fixed (per 4096 pixels of the entry, then over
 * those partials), so results are bit-identical run to run; it is NOT the order uocr_label_components uses, so a value
 * within rounding of its threshold may fall on the other side there.
 * table: int64 [n_entries][max_components][8] and count: int32 [n_entries], both on the device, with exactly the
 * semantics of uocr_label_components: scipy's numbering (order of the first pixel, row-major), 4-connectivity, half-open
 * boxes; rows past count[i] are zero; count[i] is the true count even above max_components (the table then holds the
 * first max_components rows, the labels stay complete).  labels may be NULL and so may any labels[i]; a given labels[i]
 * is int32 (h[i], w[i]) and every element is written, otherwise the entry's plane lives in the ctx workspace (line
 * finding needs no labels).  x, h, w, c, channel, labels are HOST arrays of n_entries entries (device pointers / sizes).
 * The entries travel as kernel arguments, 32 per group: no descriptor copy, no allocation.  Per group one chain of 6-7
 * kernels (5 without statistics and tile borders) whatever the number of entries, per call one memset of the table.
 * UOCR_ERR_ARG for a null x, table or count, a null x[i], pointers off their element's alignment, h[i], w[i] or c[i] < 1,
 * channel[i] outside [0, c[i]), a bad thresh_mode, max_components < 0 and n_entries < 0; UOCR_ERR_UNSUPPORTED for h * w
 * beyond int32 linear indices or a group with too many blocks for one grid; scratch (two int32 per pixel of a group at
 * most, and a little more) comes from the ctx workspace (UOCR_ERR_WORKSPACE).  Nothing is written on any error;
 * n_entries = 0 is UOCR_OK and launches nothing (the other arguments are not looked at).  Integer atomics only between
 * blocks.  Asynchronous and capturable. */
int uocr_label_batch(uocr_ctx* ctx, int dtype, int n_entries, const void* const* x, const int* h, const int* w,
                     const int* c, const int* channel, int thresh_mode, double thresh_value, int* const* labels,
                     long long* table, int max_components, int* count);
/* sizes the last uocr_label_batch call on this ctx used: the tile (rows, columns), entries per launch group, kernels
 * launched (all 0 before the first call) -- tests size their inputs from it */
int uocr_ctx_last_label_batch(uocr_ctx* ctx, int* tile_h, int* tile_w, int* entries_per_launch, int* launches);

/* ---- char labels (interpreter/interpreter.py:547-571 LabelChar._func1: the CharLabel stage) --------------------
 * The one-hot training labels of the Char net from the bit layers of every cropped line, for ALL lines of a page in one
 * call (the reference runs a Python loop per pixel in a worker pool, :524-545, between a device-to-host and a
 * host-to-device copy of every line, my_model/model.py:614-623).  Line i is x[i]: (1, h[i], w[i], c) in `dtype`, its
 * channels bit_0 .. bit_{bits-1} followed by whatever else the layer tag carries (letter_spacing, my_model/constants.py:
 * 22-25).  t = 0.5 * (mean + max) over ALL h * w * c elements of the line (float64 reductions, :549); bit k of a pixel is
 * set when x[y, x, k] > t; code = sum_k bit_k 2^k (primitives/__init__.py:46-50: least significant digit first);
 * code < n_chars is that class (code 0 -- no bit set -- is class 0, a class like any other), every other code is
 * "unknown".  Column x takes the most frequent candidate among its h pixels, all unknown codes counting as ONE candidate;
 * on a tie the candidate that occurs first from the top (collections.Counter.most_common, :565-566).  Row x of labels[i] is
 * one-hot at the winner, all zeros when "unknown" won (:567-570).
 * x[i]: (1, h[i], w[i], c) in `dtype`; labels[i]: (w[i], n_chars) in `dtype`, every element written;
 * ids: optional (may be NULL) -- ids[i]: int32 (w[i]), the winning class of each column or -1 for a zero row.
 * x, h, w, labels, ids are HOST arrays of n_lines entries (device pointers / sizes).
 * Limits: 1 <= bits <= 8, bits <= c <= 16, 1 <= n_chars <= 2^bits, h[i], w[i] >= 1 (UOCR_ERR_ARG otherwise, as for null
 * pointers, pointers off their element's alignment and n_lines < 0); h[i] <= 256 (UOCR_ERR_UNSUPPORTED; the reference's is CHAR_INPUT_HEIGHT = 32).  Nothing is
 * written on any error; n_lines = 0 is UOCR_OK and launches nothing (the other arguments are not looked at).  Two launches per 64 lines; 16 bytes of the ctx
 * workspace per 8192 elements of a line (UOCR_ERR_WORKSPACE).  No atomics: results are bit-identical run to run.
 * Asynchronous and capturable. */
int uocr_char_label(uocr_ctx* ctx, int dtype, int n_lines, const void* const* x, const int* h, const int* w,
                    int c, int bits, int n_chars, void* const* labels, int* const* ids);
/* sizes the last uocr_char_label call on this ctx used: columns per vote block, elements per stats chunk,
 * lines per launch, launches issued (all 0 before the first call) -- tests size their inputs from it */
int uocr_ctx_last_char_label(uocr_ctx* ctx, int* cols_per_block, int* stats_chunk, int* lines_per_launch, int* launches);

/* ---- line crops (interpreter/interpreter.py:504-523 CropRotateAndZoomLines._func2: the gather half of LineCrop) ----
 * Crop, quarter-turn, zoom and pad every (array, line) pair of a page in one call.  Entry i cuts the box [y0, y0 + box_h)
 * x [x0, x0 + box_w) out of src[i]: (1, src_h, src_w, c) in `dtype` (nothing is masked, :506), turns it by
 * quarter_turns * 90 degrees (np.rot90(.., quarter_turns, axes=(1, 2)), which ndimage.rotate(.., axes=(2, 1), order=1,
 * reshape=True) of 90 / 180 / 270 degrees equals bit for bit; 0 = upright) and zooms the turned box -- rot_h x rot_w,
 * (box_w, box_h) for an odd number of turns -- to zoom_h x zoom_w as ndimage.zoom(.., order=0) does: per axis z =
 * (n_in - 1) / (n_out - 1), one float64 division made on the host (n_out = 1 reads index 0); output index j reads input
 * index floor(j * z + 0.5), the product and the sum each rounded to float64 on their own, and where j * z comes out
 * above n_in - 1 (a rounding artefact of scipy's that only the last index of an axis can show) the element is 0.
 * Columns zoom_w .. out_w - 1 are zero (the reference's padding to CHAR_FIXED_WIDTH, :516-521).  The caller chooses
 * zoom_h, zoom_w (the reference: Python round(n * zoom_h / rot_h), which may give zoom_w = 0) and out_w.
 * out[i]: (1, zoom_h, out_w, c) in `dtype`, EVERY element written.  A pure index map: results are equal to the
 * reference's in every dtype.  All arguments but ctx, dtype and n_entries are HOST arrays of n_entries entries.
 * UOCR_ERR_ARG for null pointers (out[i] may be NULL where out_w[i] = 0), pointers off their element's alignment, a box
 * that is empty or not inside its source, quarter_turns outside 0..3, out_w < zoom_w, zoom_h < 1, zoom_w < 0, c < 1 and
 * n_entries < 0; UOCR_ERR_UNSUPPORTED for an output too large for one grid; nothing is written on any error.  n_entries = 0 is UOCR_OK and launches nothing (the other arguments are not looked at).  One launch per 48
 * entries; no workspace, no atomics.  Asynchronous and capturable. */
int uocr_line_crop(uocr_ctx* ctx, int dtype, int n_entries, const void* const* src, const int* src_h, const int* src_w,
                   const int* c, const int* y0, const int* x0, const int* box_h, const int* box_w,
                   const int* quarter_turns, const int* zoom_h, const int* zoom_w, void* const* out, const int* out_w);
/* sizes the last uocr_line_crop call on this ctx used: output elements per block (an entry's output is cut into flat
 * ranges of that many elements), bytes per vector store, entries per launch, launches issued (all 0 before the first
 * call) -- tests size their inputs from it */
int uocr_ctx_last_line_crop(uocr_ctx* ctx, int* elements_per_block, int* store_bytes, int* entries_per_launch, int* launches);

/* ---- paragraph rotation (interpreter/interpreter.py:188-231, :319-347: the rotation search of ParagraphCrop) ----
 * ndimage.rotate(.., angle, axes=(2, 1), reshape=True) of one paragraph, evaluated per output pixel.  The HOST computes
 * what scipy computes in Python -- the matrix M = {c, s, -s, c}, the shape of the rotated plane and the offset
 * (in_shape - 1) / 2 - M @ ((out_shape - 1) / 2) -- and passes them; the device never evaluates a cosine.  Output pixel
 * (oy, ox) has the source coordinate cy = offset[0] + oy * M[0] + ox * M[1], cx = offset[1] + oy * M[2] + ox * M[3] in
 * float64, every product and sum rounded on its own in this order; outside [0, ch - 1] x [0, cw - 1] (inclusive) it is 0.
 * Order 0 reads (floor(cy + 0.5), floor(cx + 0.5)); order 1 is bilinear over floor(c), floor(c) + 1 without prefilter,
 * and the neighbour at index n (reachable only with weight 0) is not read.
 *
 * Probe i of the extent call: the half-open extent {y0, y1, x0, x1} (find_objects) of the set pixels of the order-0
 * rotation of labels[box] == label_id[i], {0, 0, 0, 0} when none is set; no rotated array is written.  labels: int32
 * (n, h, w) as written by the labelling call above, image `image_index` of it.  HOST arrays of n_probes entries:
 * label_id, box (4 ints per probe: y0, x0, ch, cw), matrix (4 doubles), offset (2 doubles), out_shape (2 ints: the
 * rotated plane).  extent: DEVICE int32 (n_probes, 4), every element written.
 * UOCR_ERR_ARG for null pointers, n, h, w < 1, image_index outside [0, n), label_id < 1, a box that is empty or not
 * inside the image, a non-positive out_shape, a matrix or offset that is not finite and n_probes < 0; nothing is written
 * on any error; n_probes = 0 is UOCR_OK and launches nothing.  One zero fill, then two kernels per 28 probes; vector
 * integer atomics only: bit-identical run to run.  No workspace.  Asynchronous and capturable. */
int uocr_rotated_extent(uocr_ctx* ctx, const int* labels, int n, int h, int w, int image_index, int n_probes,
                        const int* label_id, const int* box, const double* matrix, const double* offset,
                        const int* out_shape, int* extent);
/* Entry i: the order-1 rotation of (image * (labels == label_id))[box], cut to the region {ry0, rx0, rh, rw} of the
 * rotated plane (:340-346) and placed in out[i]: (1, out_h, out_w, c) at row (out_h - rh) / 2, column (out_w - rw) / 2 with
 * zeros around it -- make_divisible_by's frame in the same pass, as the masked crop above does it.  EVERY element of out
 * is written; nothing outside the box is read; a masked-out neighbour contributes 0.  Coordinates, weights and the
 * four-term sum (value * wy * wx, row-major) are float64 for every dtype, the result is rounded once to `dtype`.
 * image[i]: (n, h, w, c) in `dtype`, labels[i]: int32 (n, h, w).  HOST arrays of n_entries entries: image, labels, dims
 * (4 ints per entry: n, h, w, c), image_index, label_id, box (4: y0, x0, ch, cw), matrix (4 doubles), offset (2 doubles),
 * plane (2 ints: the rotated plane the region lies in), region (4), out, out_shape (2: out_h, out_w).
 * UOCR_ERR_ARG for null pointers, pointers off their element's alignment, dims < 1, image_index outside [0, n),
 * label_id < 1, a box that is empty or not inside the image, a region that is empty or not inside the plane, an output
 * smaller than the region, a matrix or offset that is not finite and n_entries < 0; UOCR_ERR_DTYPE for an unknown dtype;
 * nothing is written on any error; n_entries = 0 is UOCR_OK and launches nothing.  One launch per 28 entries, no
 * workspace, no atomics.  Asynchronous and capturable. */
int uocr_rotate_crop(uocr_ctx* ctx, int dtype, int n_entries, const void* const* image, const int* const* labels,
                     const int* dims, const int* image_index, const int* label_id, const int* box, const double* matrix,
                     const double* offset, const int* plane, const int* region, void* const* out, const int* out_shape);
/* sizes the last extent or rotated-crop call on this ctx used: output rows per block of a probe, output pixels per
 * block of an entry, probes / entries per launch, kernels launched (all 0 before the first call) -- tests size their
 * inputs from it */
int uocr_ctx_last_rotate(uocr_ctx* ctx, int* rows_per_band, int* pixels_per_block, int* entries_per_launch, int* launches);
/* The whole angle search of CropAndRotateSingleParagraph._func (:321-336) for ALL paragraphs of a page in one call,
 * without a host step between its rounds.  The search tree does not depend on the data: node 0 is (low, high) = (0, 180),
 * a node probes a = low + (high - low) / 3 and b = high - (high - low) / 3, child 2j + 1 is the branch height_a < height_b
 * (high = b), child 2j + 2 the other (low = a).  table: DEVICE float64 (2^rounds - 1, 4), per node cos a, sin a, cos b,
 * sin b in heap order (nn/ops.py: search_table); the device never evaluates a cosine.  Per round and paragraph the two
 * probes are evaluated as uocr_rotated_extent evaluates them, except that the DEVICE computes the rotated plane and the
 * offset from the box and (c, s) -- in float64, every product and sum rounded on its own:
 *   row0 = {0, s*cw, c*ch, c*ch + s*cw}, row1 = {0, c*cw, (-s)*ch, (-s)*ch + c*cw},
 *   out_h = int((max row0 - min row0) + 0.5), out_w likewise from row1, hy = (out_h - 1) / 2, hx = (out_w - 1) / 2,
 *   offset = {(ch - 1) / 2 - (c*hy + s*hx), (cw - 1) / 2 - ((-s)*hy + c*hx)}, M = {c, s, -s, c}
 * (nn/ops.py: search_geometry; scipy's own matrix products may fuse a multiply-add and differ from it by some 1e-13 in
 * the offset).  The height of a probe is y1 - y0 of its extent, 0 when no pixel is set (then low = a).
 * labels, n, h, w, image_index as above; label_id (n_paragraphs) and box (4 ints per paragraph: y0, x0, ch, cw) are HOST
 * arrays.  result: DEVICE int32 (n_paragraphs, 1 + 2 * rounds): the LEAF the paragraph ends on -- the heap index
 * below node 0 after `rounds` decisions, 2^rounds - 1 <= leaf <= 2^(rounds + 1) - 2; the host replays the decisions for the
 * angle -- then height_a, height_b of every round.  workspace: DEVICE, uocr_rotation_search_workspace bytes, the call
 * zeroes it.  UOCR_ERR_ARG for null pointers, pointers off their element's alignment, n, h, w < 1, image_index outside
 * [0, n), rounds outside 1..16, label_id < 1, a box that is empty or not inside the image and n_paragraphs < 0;
 * UOCR_ERR_UNSUPPORTED for more blocks than one grid takes; nothing is written on any error; n_paragraphs = 0 is UOCR_OK
 * and launches nothing.  One zero fill, then two kernels per round and 14 paragraphs, all enqueued by this call in
 * stream order: no host synchronisation, no spinning, no cooperative launch.  Vector integer atomics only:
 * bit-identical run to run.  Asynchronous and capturable. */
int uocr_rotation_search(uocr_ctx* ctx, const int* labels, int n, int h, int w, int image_index, int n_paragraphs,
                         const int* label_id, const int* box, int rounds, const double* table, int* result, int* workspace);
/* bytes of the workspace of a uocr_rotation_search call on n_paragraphs paragraphs */
int uocr_rotation_search_workspace(int n_paragraphs, size_t* bytes);
/* what the last uocr_rotation_search call on this ctx used: rounds, paragraphs per launch, kernels launched (all 0 before
 * the first call) -- tests size their inputs from it */
int uocr_ctx_last_rotation_search(uocr_ctx* ctx, int* rounds, int* paragraphs_per_launch, int* launches);

/* ---- text of the lines (interpreter/interpreter.py:574-614 PredToText._func1: the PredToText stage) ----------------
 * The character ids of ALL lines of a page in one call (the reference hands every line to a worker pool after a
 * device-to-host copy, my_model/model.py:647-656).  Line i is pred[i]: (w[i], n_chars) in `dtype`, the Char net's raw
 * output, one row per column window.  Per row the maximum (:597); a row whose maximum == 0.0 -- -0.0 included --
 * contributes nothing (:598), a row that holds a NaN neither (its maximum is NaN and nothing equals NaN); a negative
 * maximum is a maximum like any other.  Every column that EQUALS its row's maximum is a candidate (:600-601): an exact tie
 * gives several; candidates are ordered by row and inside a row by column (:602).  The walk (:603-613) starts with
 * prev = none: id 0 (the tab) resets prev and emits nothing; an id similar to prev is skipped and leaves prev alone; every
 * other id is emitted and becomes prev.  similar(a, b) is "a lies in the pair of b" (primitives/__init__.py:16-54):
 * cls[id] is the index of the id's pair, -1 for an id without one -- the library knows no alphabet.  A repeated paired
 * id collapses, a repeated unpaired one does not.  Since prev always lies in the pair class of the last id that was not
 * the tab, candidate s[k] is emitted iff s[k] != 0 and not (cls[s[k]] >= 0 and k > 0 and s[k-1] != 0 and cls[s[k-1]] ==
 * cls[s[k]]), s[k-1] the previous CANDIDATE (rows without candidates are passed over and reset nothing): that is what the
 * kernels evaluate.
 * count[i]: int32, the number of emitted ids, always the full number; ids[i]: uint8 of capacity cap[i], the first
 * min(count, cap) emitted ids in order -- nothing past cap[i] and nothing past count[i] is written (ids[i] may be NULL
 * where cap[i] = 0).  pred, w, ids, cap, count and cls (n_chars entries) are HOST arrays; pred[i], ids[i], count[i] are
 * device pointers.
 * Limits: 1 <= n_chars <= 256, w[i] >= 1, cap[i] >= 0, -1 <= cls[k] < n_chars (UOCR_ERR_ARG otherwise, as for null
 * pointers, pred[i] / count[i] off their element's alignment and n_lines < 0); UOCR_ERR_DTYPE for an unknown dtype;
 * UOCR_ERR_UNSUPPORTED for more rows than one grid takes.  Nothing is written on any error; n_lines = 0 is UOCR_OK and
 * launches nothing (the other arguments are not looked at).  Two launches per 64 lines; 32 bytes of the ctx workspace per
 * row plus 16 per 64 rows of a line (UOCR_ERR_WORKSPACE).  Comparisons only, no floating-point arithmetic: results equal
 * the reference's in every dtype.  No atomics: results are bit-identical run to run.  Asynchronous and capturable. */
int uocr_pred_to_text(uocr_ctx* ctx, int dtype, int n_lines, const void* const* pred, const int* w, int n_chars,
                      const int* cls, unsigned char* const* ids, const int* cap, int* const* count);
/* sizes the last uocr_pred_to_text call on this ctx used: rows of a line per block, lines per launch, launches issued
 * (all 0 before the first call) -- tests size their inputs from it */
int uocr_ctx_last_pred_to_text(uocr_ctx* ctx, int* rows_per_block, int* lines_per_launch, int* launches);

/* ---- text score: how well the lines of a page were read (no counterpart in the reference, whose nn/metrics.py is a
 * stub) ----
 * Line i is pred[i]: (w[i], n_chars) in `dtype`, the Char net's raw output, and label[i]: (w[i], n_chars) in `dtype`,
 * the one-hot labels of the same columns (uocr_char_label).  Both are read by ONE rule.  The id of a row is -1 where the
 * row holds a NaN or its maximum == 0.0 (-0.0 included), otherwise the SMALLEST column that equals the row's maximum (a
 * negative maximum is a maximum like any other): uocr_pred_to_text's conventions with the first candidate taken.  The
 * reading of a matrix is one id per run of equal row ids; id 0 (the tab, the background class) and -1 emit nothing and
 * end a run: row r contributes iff id[r] > 0 and (r == 0 or id[r] != id[r-1]).  The score of the line is the unit-cost
 * Levenshtein distance between reading(label[i]), the EXPECTED string, and reading(pred[i]), the READ string, where ids
 * x and y match when canon[x] == canon[y] -- the library knows no alphabet; the identity table compares ids.
 * scores: DEVICE int32 (n_lines, 4): distance, length of the expected string, length of the read string, 0.
 * read_ids / expected_ids: optional (either may be NULL) HOST arrays of n_lines device pointers to uint8 buffers of
 * w[i] bytes -- a reading is never longer than w[i], so there is no capacity and never a second call; the ids of the
 * reading are written from byte 0 on and nothing behind them.  pred, label, w and canon (n_chars entries) are HOST
 * arrays; pred[i], label[i] are device pointers.
 * Limits: 1 <= n_chars <= 255, 1 <= w[i] <= max_width of uocr_text_score_limits, 0 <= canon[k] < n_chars (UOCR_ERR_ARG
 * otherwise, as for null pointers, pred[i] / label[i] / scores off their element's alignment and n_lines < 0);
 * UOCR_ERR_DTYPE for an unknown dtype; UOCR_ERR_UNSUPPORTED for more rows than one grid takes.  Nothing is written on any
 * error; n_lines = 0 is UOCR_OK and launches nothing (the other arguments are not looked at).  Two launches per
 * lines_per_launch lines; of the ctx workspace 2 bytes per row rounded up to rows_per_block rows per matrix plus
 * 12 * w[i] + 8 bytes per line of the largest launch (UOCR_ERR_WORKSPACE).  Comparisons and integer arithmetic only: no
 * tolerance in any dtype.  No atomics: results are bit-identical run to run.  Asynchronous and capturable.  The call
 * leaves no launch report. */
int uocr_text_score(uocr_ctx* ctx, int dtype, int n_lines, const void* const* pred, const void* const* label, const int* w,
                    int n_chars, const int* canon, unsigned char* const* read_ids, unsigned char* const* expected_ids,
                    int* scores);
/* the sizes uocr_text_score works with, whatever the context: rows of a matrix per block of the reading kernel, lines per
 * launch pair, columns of the expected string per panel of the distance kernel (64 lanes x the most columns per lane; a
 * string of up to 64 K columns runs with K = 1, 2, 4 columns per lane), the widest line it takes.  UOCR_ERR_ARG for a
 * null pointer, before anything is written -- tests size their inputs from it */
int uocr_text_score_limits(int* rows_per_block, int* lines_per_launch, int* columns_per_panel, int* max_width);

/* ---- label overlap: what a mask net found of the true components (the reference's nn/metrics.py has
 * binary_classification_metrics for 0/1 arrays, which nothing there calls; it has no score of components) ----
 * Entry i is a pair of int32 label planes a[i], the EXPECTED labels, and b[i], the PREDICTED labels, (h[i], w[i]) each, as
 * uocr_label_batch writes them: 0 is the background, components are 1, 2, ...  a, b, h, w are HOST arrays; a[i], b[i] are
 * device pointers (4-byte aligned; the two planes of an entry may differ in their 16-byte alignment).
 * bucket(l, cap) = l where 0 <= l <= cap, else cap + 1, the OVERFLOW bucket; labels are compared as unsigned, so a
 * negative label overflows.  All outputs are DEVICE arrays:
 * overlap: int32 [n_entries][cap_a + 2][cap_b + 2]; overlap[i][r][s] = the pixels p of entry i with bucket(a[p], cap_a)
 *   = r and bucket(b[p], cap_b) = s.
 * rows: int32 [n_entries][cap_a + 2][4] = {area, best, inter, other} per row r of the table: area = the sum of the row;
 *   best = the s in 1 .. cap_b with the largest overlap[r][s] > 0, the smallest s on a tie, 0 when there is none; inter =
 *   overlap[r][best]; other = the sum of column best; inter = other = 0 where best is 0.
 * cols: int32 [n_entries][cap_b + 2][4]: the same of the transposed table (best is an r in 1 .. cap_a).
 * summary: int64 [n_entries][8] = {tp, fp, fn, tn, expected, predicted, matched, overflow}: tp = the cells with r >= 1
 *   and s >= 1, fp = row 0 without its first cell, fn = column 0 without its first cell, tn = overlap[0][0] (the overflow
 *   buckets are foreground); expected / predicted = the r in 1 .. cap_a / the s in 1 .. cap_b with area > 0; matched = the
 *   r in 1 .. cap_a with best > 0 and 2 * inter > area + other - inter, an intersection over union above one half, which
 *   makes a match mutual and unique; overflow = the pixels with either bucket in the overflow.
 * With cap_a = cap_b = 0 the table is the 2 x 2 confusion matrix of foreground against foreground.
 * Every element of all four outputs is written by every successful call (one memset of `overlap`, then two launches per
 * entries_per_launch entries); none may be NULL.  UOCR_ERR_ARG for null arrays, a null a[i] / b[i], a pointer off its
 * element's alignment, h[i] or w[i] < 1, a negative cap, n_entries < 0; UOCR_ERR_UNSUPPORTED for a cap above max_cap of
 * uocr_label_overlap_limits, h[i] * w[i] > INT32_MAX or more blocks than one grid takes.  Nothing is written on any error;
 * n_entries = 0 is UOCR_OK and launches nothing (the other arguments are not looked at).  No workspace, no allocation,
 * no copy, no host synchronisation: asynchronous and capturable.  Integer atomics only: results are bit-identical run to
 * run, and no tolerance applies.  The call leaves no launch report. */
int uocr_label_overlap(uocr_ctx* ctx, int n_entries, const int* const* a, const int* const* b, const int* h, const int* w,
                       int cap_a, int cap_b, int* overlap, int* rows, int* cols, long long* summary);
/* the sizes uocr_label_overlap works with, whatever the context: consecutive pixels of an entry per block of the counting
 * kernel, the cells of the largest table a block counts in LDS before it adds to the global one (larger tables are added
 * to directly), entries per launch pair, the largest cap.  UOCR_ERR_ARG for a null pointer, before anything is written --
 * tests size their inputs from it */
int uocr_label_overlap_limits(int* pixels_per_block, int* lds_cells, int* entries_per_launch, int* max_cap);

/* ---- the lines of a page in one strip (the Char net over all lines in one pass; the reference runs a pass per line,
 * nn/model_system.py:150-154) ----
 * A strip is (1, h, strip_w, c) in `dtype`; its columns are cut into SEGMENTS [x0[i], x0[i] + w[i]), i < n_lines, with GAPS
 * in front of, between and behind them (a gap may have no column).  With 4 zero columns between neighbouring lines and the
 * gaps set back to zero after every conv + LeakyReLU, the Char net (three convs of 3 columns with padding 1, then windows
 * of 8 columns padded by 4 zero columns on the left and 3 on the right) gives every column of a line exactly what it gives
 * it when the line is passed alone; the outer ends of the strip need no gap.
 * Pack: segment i of the strip = src[i]: (1, h, w[i], c) in `dtype`, every gap = +0.0; EVERY element of the strip is
 * written, the sources are only read.  src, w and x0 are HOST arrays of n_lines entries; src[i] and strip are device
 * pointers.  A copy, no arithmetic: every element keeps its bits.
 * UOCR_ERR_ARG for null pointers, pointers off their element's alignment, w[i] < 1, h, c or strip_w < 1, n_lines < 0 and
 * segments that are not ascending, that overlap or that reach outside [0, strip_w); UOCR_ERR_DTYPE for an unknown dtype;
 * UOCR_ERR_UNSUPPORTED for a strip row of more than 2^31 - 1 elements and for more blocks than one grid takes.  Nothing
 * is written on any error; n_lines = 0 is UOCR_OK and launches nothing (the other arguments are not looked at).  One launch
 * per 128 lines; no workspace, no atomics.  Asynchronous and capturable. */
int uocr_pack_lines(uocr_ctx* ctx, int dtype, int n_lines, const void* const* src, const int* w, int h, int c,
                    const int* x0, void* strip, int strip_w);
/* Zero gaps, in place on x: (1, h, strip_w, c) in `dtype`: every element of every gap becomes +0.0 -- written, not
 * multiplied: a NaN or an infinity there becomes 0 -- and no element of a segment is touched.  The work is proportional
 * to the gaps, not to the tensor: only the columns of the gaps are visited.  x0 and w are HOST arrays of n_lines entries.
 * Errors and n_lines = 0 as for uocr_pack_lines.  One launch per 128 gaps, none when no gap has a column; no workspace,
 * no atomics.  Asynchronous and capturable. */
int uocr_zero_gaps(uocr_ctx* ctx, int dtype, void* x, int h, int strip_w, int c, int n_lines, const int* x0, const int* w);
/* sizes the last uocr_pack_lines or uocr_zero_gaps call on this ctx used: elements of an entry -- a line with the gap
 * behind it, or a gap -- per block at most (whole rows of the entry, or one piece of a row that is longer), entries per
 * launch, launches issued (all 0 before the first call) -- tests size their inputs from it */
int uocr_ctx_last_pack_lines(uocr_ctx* ctx, int* elements_per_block, int* entries_per_launch, int* launches);

/* ---- training pages made on the device (image_generator/generate.py: LayeredImage.add_paragraph) ----
 * Integer arithmetic only.  Draw `slot` of attempt `a` of page `p` (64-bit) is z = splitmix64's finaliser of
 * seed + (((p * 32 + a) * 1024 + slot) + 1) * 0x9E3779B97F4A7C15 mod 2^64; a draw in [lo, hi] is
 * lo + (((z >> 32) * (hi - lo + 1)) >> 32).  The atlas (univer-ocr_amd/my_model/glyphs.npz) travels as device arrays:
 * metrics (n_faces, 7) int32 = size, ascent, descent, height, x_height, spacing, pitch; adv and offset (n_faces, 162)
 * int32 = columns of the cell of every character id and its start in `cells`, n_cells bytes of coverage 0..255, a cell
 * `height` rows of `adv` columns.
 * Layout: pages first_page .. first_page + n_pages - 1 of `height` x `width` pixels.  Each page makes 32 paragraph attempts
 * in order: slot 0 the face, 1 the number of words 3..30, 2 the wrap width 30..100 characters, 3 + j the length 1..10 of word
 * j, 64 + 10 j + i character i of word j (ids 2..161), 512 + 2 r / 513 + 2 r the position x / y of try r < 64.  Words wrap
 * greedily with one space (id 1) between them.  The paragraph is t_width = the widest line (sum of adv) by t_height =
 * n_lines * pitch - spacing; x is drawn in [20, width - (t_width + 6) - 20], y in [0, height - (t_height + 6)], the attempt is
 * dropped when a range is empty; the first try whose box of t_width + 6 by t_height + 6 at (x, y) meets no paragraph box
 * accepted so far wins and the paragraph lies at (x + 3, y + 3); no such try drops the attempt.  Per page, int32:
 *   paragraphs (32, 8)     x0, y0, w, h, face, n_lines, first_line, attempt
 *   lines      (960, 5)    left, y_ascent, width, first_glyph, n_glyphs     (line k of a paragraph: y0 + k * pitch)
 *   glyphs     (10560, 2)  pen (the first column of the cell), id
 *   counts     (4)         paragraphs, lines, glyphs, 0
 * Rows past the counts are not written.  paragraphs and counts 16-byte aligned, glyphs 8-byte aligned.
 * Render: every pixel finds the first paragraph box that holds it, the line (y - y0) / pitch, row r inside it, and -- on
 * the columns [left, left + width) and rows r < height -- the glyph by binary search over the pens, column u inside the
 * cell, w10 = max(1, adv / 10):
 *   paragraph 1 inside a box; line_top 1 for r < ascent, line_bottom 1 for r >= ascent - x_height;
 *   bit_k (id >> k) & 1 for w10 <= u < adv - w10; letter_spacing 1 for u >= adv - w10 unless the glyph is the last of its
 *   line, and for u < w10 of the glyph before it unless it is the first; monochrome lut[cov], image lut[255 - cov]
 * with cov the cell's coverage there, 0 outside every cell.  lut: 256 values in `dtype`.  image, monochrome, paragraph:
 * (n_pages, height, width, 1) in `dtype`; line: (.., 2) = line_top, line_bottom; chr: (.., 9) = bit_0 .. bit_7,
 * letter_spacing.  EVERY element is written exactly once, by one thread: no memset, no atomics, results are bit-identical
 * run to run.  The tables are only read, every index taken from them is checked against its table: tables that hold
 * anything whatever give pixels without a line or a glyph, never an access outside the arrays.
 * UOCR_ERR_ARG for null pointers, pointers off their alignment, n_pages < 0, height or width outside [1, 2^24] and n_faces
 * outside [1, 256]; UOCR_ERR_DTYPE for an unknown dtype; UOCR_ERR_UNSUPPORTED for a page of more tiles than one grid takes.
 * Nothing is written on any error; n_pages = 0 is UOCR_OK and launches nothing (the other arguments are not looked at).
 * One launch per 256 pages each; no workspace.  Asynchronous and capturable. */
int uocr_page_layout(uocr_ctx* ctx, unsigned long long seed, unsigned long long first_page, int n_pages, int height,
                     int width, int n_faces, const int* metrics, const int* adv, int* paragraphs, int* lines, int* glyphs,
                     int* counts);
int uocr_page_render(uocr_ctx* ctx, int dtype, int n_pages, int height, int width, const int* paragraphs, const int* lines,
                     const int* glyphs, const int* counts, int n_faces, const int* metrics, const int* adv, const int* offset,
                     const unsigned char* cells, long long n_cells, const void* lut, void* image, void* monochrome,
                     void* paragraph, void* line, void* chr);
/* sizes the last uocr_page_layout or uocr_page_render call on this ctx used: rows and columns of a render tile, pages
 * per launch, launches issued (all 0 before the first call) -- tests size their inputs from it.  UOCR_ERR_ARG (-1) for a
 * null ctx or a null out pointer. */
int uocr_ctx_last_page_gen(uocr_ctx* ctx, int* tile_rows, int* tile_cols, int* pages_per_launch, int* launches);

/* ---- data parallel over the GPUs of one node: RCCL over xGMI ------------------------------------
 * The reference has no multi-GPU path; BASELINE.json adds one to the step loop my_model/trainer.py:213-233
 * -> nn/model_system.py:104-118 -> nn/models.py:250-254: between compute_loss_and_gradients and update_grads
 * every rank's flat gradient buffer is summed.  One process per GPU, one communicator per process and device.
 * librccl.so.1 is bound at run time (no link-time dependency; single-GPU use needs no RCCL).
 *   rank 0:   uocr_dp_get_unique_id(id)  -> ship the 128 bytes to the other ranks by ANY channel (file, socket,
 *             MPI, torch.distributed, the launcher's environment)
 *   all:      uocr_dp_init(ctx, rank, world, id)                 (collective; blocks until every rank called)
 *             uocr_dp_broadcast(ctx, weights, n, UOCR_F32, 0)    identical replicas
 *   per step: uocr_dp_allreduce_sum(ctx, grads, n, UOCR_F32)     in place, asynchronous on THAT ctx's stream
 *   all:      uocr_dp_finalize(ctx)
 * Collectives of the communicator must be issued in the same order on every rank and must not overlap each
 * other: issue them through one ctx (a communication lane), or chain the issuing streams with
 * uocr_event_record / uocr_stream_wait_event. */
#define UOCR_DP_UNIQUE_ID_BYTES 128
int uocr_dp_get_unique_id(void* out_bytes /* UOCR_DP_UNIQUE_ID_BYTES */);
int uocr_dp_init(uocr_ctx* ctx, int rank, int world, const void* unique_id_bytes);
int uocr_dp_info(uocr_ctx* ctx, int* rank, int* world /* 0 = no communicator */);
int uocr_dp_allreduce_sum(uocr_ctx* ctx, void* buf, size_t count, int dtype);
int uocr_dp_broadcast(uocr_ctx* ctx, void* buf, size_t count, int dtype, int root);
int uocr_dp_finalize(uocr_ctx* ctx);
int uocr_dp_version(int* out_version);   /* ncclGetVersion of the RCCL this process bound (e.g. 22703), for run records */

#ifdef __cplusplus
}
#endif
#endif /* UNIVER_HIP_H */
