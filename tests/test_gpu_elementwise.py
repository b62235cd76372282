"""y and dx of the conv, upsample+conv, conv-pair and dense kernels ELEMENT BY ELEMENT under the derived bound of
elementwise_bound.py, on inputs whose magnitude varies by powers of two over images, 8-row bands, 24-column strips and
channels.

Every other parity test divides the largest error by the largest expected value (rel_linf), on inputs of one
magnitude: one large element hides relative error everywhere else.  The kernels that carry state across tiles (the
TileWalk kernels of conv_h16*.hip and conv_t32.hip, the band walkers of conv_up.hip, the strip kernels of
conv_pair_strip*.hip) or add partial sums (the GEMM's depth slabs) can lose precision, cancel or leak between regions,
images and channels without moving that figure.  Here every element has its own tolerance

    tol = store_u |ref| + (operand_u + gamma(n + 8)) S + floor          (elementwise_bound.py derives every term)

against the float64 oracle; test_elementwise_bound_host.py shows on the CPU that a float32 restatement of the oracle
keeps to half of it while a constant leak, a sliding sum and binary16 weights do not pass.

Cases (elementwise_bound.CASES), pages of 3 x 37 x 141 (2 x 19 x 71 low-resolution upconv inputs: several tiles, ragged
last tiles in both directions):
  float32   the nine FastConv table configurations at the nets' padding, forward (plain, LeakyReLU) and backward-data
            (plain, LeakyReLU mask), under the default dispatch and with t32 = 0, tiled = 0 (the shadowed table
            kernels); the MFMA implicit GEMM (mfma = 2, 3x3, 32 -> 32); the generic kernel (4x4, 6 -> 7, stride (2, 1),
            padding (1, 2), padding value 0.25); upconv2x 4 -> 4 and 1 -> 1; conv_pair_fwd (act2 none) and the dx of
            conv_pair_bwd; dense_fwd / dense_bwd and windows_dense_fwd / windows_dense_bwd at (67, 200) x (200, 70)
  binary16  the table configurations with h16 = 1 and 0; both upconvs; conv_pair_fwd
Each case runs with max_blocks 0 and 3 (blocks walk several tiles and images); every output buffer starts as NaN; after
each launch on a conv entry point `Runtime.last_conv` must name the family test_gpu_conv_padding.expect_kernel expects.

conv_pair_bwd: where z1 lies within its own bound of 0 the LeakyReLU slope is undecided; the dx pixels whose 3x3 field
holds such a z1 are not judged (the host test caps them at 1 %).

Sigmoid epilogues (elementwise_bound.SIGMOID_CASES): y_sigmoid of every conv, upconv and pair case above and of
dense_fwd, with the last weights times the power of two that spreads v over the Sigmoid (|v| <= 4, v >= 20, v <= -20,
the float32 overflow of expf, binary16 results below the subnormals), under act_dispatch 1 (the kind as a compile-time
tag) and 0 (the run-time switch).  tol = E sigma'(max(0, |v| - E)) + sigma ((1 - sigma) k u + 2 u) + 2^-126 [+ store].

The Sigmoid derivative from a stored output (FROM_OUTPUT_CASES): act_bwd_from_output, and seg_loss(out_act = Sigmoid)
for Dice and Jaccard at c = 1, 2, 4 (seg_grad_vec_kernel on the shape that is a multiple of 16 bytes, the generic
kernel on the other) and c = 3, float32 and binary16, against the same expression in float64 on the same y: 3 u |ref|
and the coefficient roundings of seg_loss; y holds 0, 1 and their neighbours.

dx of the pair with every pixel judged (PAIR_DX_CASES): float32, and the binary16 pair_strip_bwd_h_kernel at 141, 128
(MODE 0) and 71 columns, pad1 0 and 0.25, act2 none and Sigmoid, with and without accumulation, in the default bands
and with one band per image.  The kernel's rounding points are restated on the host; a pixel that a slope the kernel
may take otherwise than the oracle reaches gains (1 - alpha)(|ga1| + Ega) |w1[tap]|; none is left out.

Weight gradients (elementwise_wgrad.WCASES; that module derives the bound tol = gamma(n + 8) S + u32 |init + ref| and
says why its pages are small: n = N OH OW <= 2048, at (3, 20, 32) and (1, 13, 141); upconv inputs (3, 10, 16) and (1, 6,
71)): dw and db of the nine table configurations (float32 under the default dispatch and with t32 = 0, tiled = 0;
binary16 with h16 = 1 and 0, dy carrying a gradient scale 2^k), of the MFMA conv and the generic conv, of upconv2x 4 -> 4
and 1 -> 1 in both types, of dense_bwd (the generic GEMM, the MFMA GEMM, and 1 500 rows whose depth the MFMA GEMM
splits: `Runtime.last_gemm` must report the slabs test_gpu_gemm_configs.expect_gemm / expect_group predict) and
windows_dense_bwd, and dw1 / db1 / dw2 / db2 of the float32 conv_pair_bwd with act2 none and Sigmoid.  Every case runs
with max_blocks 0 and 3, overwriting NaN-filled buffers and accumulating onto init = float32(ref r), with the producer's
own finish and inside `with rt.defer_wgrad():`, where the call is issued TWICE into two sets of buffers so that the
group kernels run two recorded finishes (GEMMs), the second at a non-zero `first_block`; both sets are judged.

The binary16 pair at its own roundings (elementwise_wgrad.PAIR16_KEYS, elementwise_bound.PAIR_WAVE_DX_KEYS): dw1 / db1 / dw2
/ db2 of pair_strip_bwd_h_kernel at (3, 20, 32), (1, 13, 141), (2, 8, 128) and of pair_wave_bwd_h_kernel at (1, 3, 600), (1, 3,
560), (3, 1, 560), and the dx of the wave kernel at (2, 11, 600) and (1, 3, 560), pad1 0 and 0.25, act2 none and Sigmoid,
against the kernel's rounding points restated in float64 with every binary16 rounding of a float32 value as an interval;
pair_band 0 and 2, pair_g 4 and 2, need_dx True and False, overwriting and accumulating, own finish and deferred twice;
`Runtime.last_pair` after every launch.  Measured: dw1 <= 0.021, db1 <= 0.015, dw2 <= 0.048, db2 < 0.0005, dx <= 0.958.

The largest err / tol of every output is printed before it is judged.
"""
import contextlib

import numpy as np
import pytest

import elementwise_bound as B
import elementwise_wgrad as W
from conftest import rel_linf
from test_gpu_conv_padding import DEFAULTS, DGRAD, FWD, KERNELS, KID, ctx  # noqa: F401  (ctx: the NaN-filling fixture)
from test_gpu_gemm_configs import GEMM_DEFAULTS, WS_HALF, expect_gemm, expect_group
from test_gpu_pair_forms import expect_pair

pytestmark = pytest.mark.gpu

CAPS = (0, 3)
EXTRA_DEFAULTS = dict(act_dispatch=1, pair_band=0, pair_g=4)       # options a test sets on top of a case's own, and their defaults


def launches(CP, c):
    """{output: (launch(), conv entry or None)} for the case's problem on the device"""
    from univer_ocr_amd.hip import lib as hiplib
    from univer_ocr_amd.nn import ops
    p, q = c.problem, c.problem.q
    dev = lambda k: CP.copy(q[k])
    par = lambda k: CP.copy(q[k], np.float32)
    if isinstance(p, B.PairDxProblem):
        x, g, yout = dev('x'), dev('g'), dev('yout')
        w1, b1, w2 = (par(k) for k in ('w1', 'b1', 'w2'))
        act2 = hiplib.ACT_SIGMOID if p.sig else hiplib.ACT_NONE

        def bwd(accumulate):
            grads = [CP.full(q[k].shape, 0.0, np.float32) for k in ('w1', 'b1', 'w2', 'b2')]
            return ops.conv_pair_bwd(x, yout, g, w1, b1, w2, *grads, p.pad1, True, True, B.ALPHA, act2, need_dx=True,
                                     accumulate=accumulate)

        return dict(dx=(lambda: bwd(False), None), dx_accumulate=(lambda: bwd(True), None))
    if isinstance(p, B.FromOutputProblem):
        y = dev('y')
        if p.kind == 'act':
            dy = dev('dy')
            return dict(dx=(lambda: ops.act_bwd_from_output('sigmoid', y, dy), None))
        gt = dev('gt')

        def grad():
            out = ops.seg_loss(p.kind, y, gt, True, 'sigmoid')[1]
            assert getattr(out, 'gscale', 0) == p.gscale, (out.gscale, p.gscale)
            return out

        return dict(dx=(grad, None))
    if isinstance(p, B.SigmoidProblem):
        p = p.inner
        x, w = dev('x'), par(c.problem.last)
        if isinstance(p, B.ConvProblem):
            d, b = p.d, par('b')
            return dict(y_sigmoid=(lambda: ops.conv2d_fwd(x, w, b, (d.sh, d.sw), (d.ph, d.pw), p.pad_value, p.bias,
                                                          act='sigmoid'), FWD))
        if isinstance(p, B.UpProblem):
            b = par('b')
            return dict(y_sigmoid=(lambda: ops.upconv2x_fwd(x, w, b, (2, 2), True, 'sigmoid'), None))
        if isinstance(p, B.PairProblem):
            w1, b1, b2 = (par(k) for k in ('w1', 'b1', 'b2'))
            return dict(y_sigmoid=(lambda: ops.conv_pair_fwd(x, w1, b1, w, b2, p.pad1, True, True, B.ALPHA,
                                                             hiplib.ACT_SIGMOID), None))
        assert isinstance(p, B.DenseProblem)
        return dict(y_sigmoid=(lambda: ops.dense_fwd(x, w, act='sigmoid'), None))
    if isinstance(p, B.ConvProblem):
        d = p.d
        st, pd = (d.sh, d.sw), (d.ph, d.pw)
        x, g, m, w, b = dev('x'), dev('g'), dev('m'), par('w'), par('b')
        return dict(
            y=(lambda: ops.conv2d_fwd(x, w, b, st, pd, p.pad_value, p.bias), FWD),
            y_leaky=(lambda: ops.conv2d_fwd(x, w, b, st, pd, p.pad_value, p.bias, act='leaky', alpha=B.ALPHA), FWD),
            dx=(lambda: ops.conv2d_bwd_data(g, w, x.shape, st, pd), DGRAD),
            dx_leaky=(lambda: ops.conv2d_bwd_data(g, w, x.shape, st, pd, x_act=m, act='leaky', alpha=B.ALPHA), DGRAD))
    if isinstance(p, B.UpProblem):
        x, g, m, w, b = dev('x'), dev('g'), dev('m'), par('w'), par('b')
        return dict(
            y=(lambda: ops.upconv2x_fwd(x, w, b, (2, 2), True), None),
            y_leaky=(lambda: ops.upconv2x_fwd(x, w, b, (2, 2), True, 'leaky', B.ALPHA), None),
            dx=(lambda: ops.upconv2x_bwd_data(g, w, x.shape, (2, 2)), None),
            dx_leaky=(lambda: ops.upconv2x_bwd_data(g, w, x.shape, (2, 2), x_act=m, act='leaky', alpha=B.ALPHA), None))
    if isinstance(p, B.PairProblem):
        x, g = dev('x'), dev('g')
        w1, b1, w2, b2 = (par(k) for k in ('w1', 'b1', 'w2', 'b2'))

        def fwd():
            return ops.conv_pair_fwd(x, w1, b1, w2, b2, p.pad1, True, True, B.ALPHA, hiplib.ACT_NONE)

        def bwd():
            grads = [CP.full(q[k].shape, 0.0, np.float32) for k in ('w1', 'b1', 'w2', 'b2')]
            return ops.conv_pair_bwd(x, fwd(), g, w1, b1, w2, *grads, p.pad1, True, True, B.ALPHA, hiplib.ACT_NONE,
                                     need_dx=True, accumulate=False)

        return dict(y=(fwd, None), dx=(bwd, None))
    x, g, w = dev('x'), dev('g'), par('w')
    dw = lambda: CP.full(q['w'].shape, 0.0, np.float32)
    if isinstance(p, B.DenseProblem):
        return dict(y=(lambda: ops.dense_fwd(x, w), None),
                    dx=(lambda: ops.dense_bwd(x, w, g, dw(), accumulate=False, need_dx=True), None))
    assert isinstance(p, B.WindowsProblem)
    return dict(y=(lambda: ops.windows_dense_fwd(x, w, B.WIN_WIDTH), FWD),
                dx=(lambda: ops.windows_dense_bwd(x, w, g, dw(), B.WIN_WIDTH, accumulate=False), DGRAD))


def judge(CP, c, settings=((),)):
    """every output of case `c` with max_blocks 0 and 3 under each of `settings` (tuples of (option, value) on top of the
    case's own): last_conv and every element; returns the misses"""
    rt = CP.runtime()
    p = c.problem
    for key, value in DEFAULTS:
        rt.set_option(key, c.opts.get(key, value))
    CP.set_dtype(p.dtype)
    run = launches(CP, c)
    tols = p.tolerances(c.operand16)
    failures = []
    for form in c.outputs:
        launch, entry = run[form]
        name = form.split('_accumulate')[0]              # (the same output from the accumulating form of the call)
        ref, tol, judged = p.ref[name], tols[name], p.judged(name)
        for extra in settings:
            for cap in CAPS:
                rt.set_option('max_blocks', cap)
                for key, value in extra:
                    rt.set_option(key, value)
                try:
                    got = launch()
                    noted = rt.last_conv()
                finally:
                    rt.set_option('max_blocks', 0)
                    for key, _ in extra:
                        rt.set_option(key, EXTRA_DEFAULTS[key])
                what = f'{c.id} {form} max_blocks={cap}' + ''.join(f' {k}={v}' for k, v in extra)
                if entry is not None:
                    want = (entry, KID[c.kernels[name]])
                    if noted != want:
                        failures.append(f'{what}: last_conv {noted} ({KERNELS[noted[1]]}) != {want} ({c.kernels[name]})')
                host = CP.asnumpy(got)
                assert host.shape == ref.shape and host.dtype == B.STORE[p.dtype], (what, host.shape, host.dtype)
                ratio = B.worst_ratio(host, ref, tol, judged)
                at = np.unravel_index(np.argmax(np.where(judged, np.nan_to_num(np.abs(host - ref) / tol, nan=np.inf), -1.0)),
                                      ref.shape)
                print(f'{what}: largest err / tol {ratio:.3f} at {tuple(int(i) for i in at)} '
                      f'(rel_linf {rel_linf(np.nan_to_num(host.astype(np.float64)), ref):.2e}, NaN {int(np.isnan(host).sum())})')
                if not ratio <= 1.0:
                    over = int((np.abs(host - ref) > tol)[np.broadcast_to(judged, ref.shape)].sum())
                    failures.append(f'{what}: err / tol = {ratio:.3f} at {tuple(int(i) for i in at)}, {over} elements over')
    return failures


@pytest.mark.parametrize('index', range(len(B.CASES)), ids=B.CASE_IDS)
def test_every_element_within_the_derived_bound(index, ctx):
    failures = judge(ctx, B.CASES[index])
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('index', range(len(B.SIGMOID_CASES)), ids=B.SIGMOID_IDS)
def test_every_sigmoid_output_within_the_derived_bound(index, ctx):
    """The Sigmoid epilogue as a compile-time tag (act_dispatch 1) and through the run-time switch (act_dispatch 0)."""
    failures = judge(ctx, B.SIGMOID_CASES[index], ((('act_dispatch', 1),), (('act_dispatch', 0),)))
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('index', range(len(B.FROM_OUTPUT_CASES)), ids=B.FROM_OUTPUT_IDS)
def test_sigmoid_derivative_from_the_output_within_the_bound(index, ctx):
    """dy y (1 - y) of act_bwd_from_output and the Dice / Jaccard gradient of seg_loss(out_act = Sigmoid) against the same
    expression in float64 on the same stored y."""
    failures = judge(ctx, B.FROM_OUTPUT_CASES[index])
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('index', range(len(B.PAIR_DX_CASES)), ids=B.PAIR_DX_IDS)
def test_pair_dx_every_pixel_within_the_bound(index, ctx):
    """dx of conv_pair_bwd (float32; binary16: pair_strip_bwd_h_kernel, MODE 0 and 1, act2 none and Sigmoid) with NO pixel
    left out: a pixel that a contested LeakyReLU slope reaches has a wider tolerance (elementwise_bound.PairDxProblem).
    With and without accumulation of the weight gradients, in the default bands and with one band per image."""
    c = B.PAIR_DX_CASES[index]
    c = c._replace(outputs=('dx', 'dx_accumulate'))
    failures = judge(ctx, c, ((), (('pair_band', c.problem.q['x'].shape[1]),)))
    assert not failures, '\n'.join(failures)


# ---- weight gradients ----------------------------------------------------------------------------------------------------
def wgrad_call(CP, c):
    """call(buffers, accumulate): the case's weight-gradient op into `buffers` = {output: float32 DeviceArray}"""
    from univer_ocr_amd.hip import lib as hiplib
    from univer_ocr_amd.nn import ops
    p = c.problem
    dev = lambda k: CP.copy(p.device(k))
    par = lambda k: CP.copy(p.q[k], np.float32)
    if isinstance(p, W.PairWgradProblem):
        x, g, yout = dev('x'), dev('g'), dev('yout')
        w1, b1, w2 = (par(k) for k in ('w1', 'b1', 'w2'))
        act2 = hiplib.ACT_SIGMOID if p.sig else hiplib.ACT_NONE
        return lambda b, acc: ops.conv_pair_bwd(x, yout, g, w1, b1, w2, b['dw1'], b['db1'], b['dw2'], b['db2'], p.pad1, True,
                                                True, B.ALPHA, act2, need_dx=True, accumulate=acc)
    x, g = dev('x'), dev('g')
    if p.half:
        g.gscale = p.gscale                     # dy is stored times 2^k; the kernels divide dw / db by it
    if isinstance(p, W.ConvWgradProblem):
        d = p.d
        return lambda b, acc: ops.conv2d_bwd_weight(x, g, b['dw'], b['db'], (d.sh, d.sw), (d.ph, d.pw), p.pad_value, p.bias,
                                                    accumulate=acc)
    if isinstance(p, W.UpWgradProblem):
        return lambda b, acc: ops.upconv2x_bwd_weight(x, g, b['dw'], b['db'], (2, 2), True, accumulate=acc)
    w = par('w')
    if isinstance(p, W.DenseWgradProblem):
        return lambda b, acc: ops.dense_bwd(x, w, g, b['dw'], accumulate=acc, need_dx=False)
    assert isinstance(p, W.WindowsWgradProblem)
    return lambda b, acc: ops.windows_dense_bwd(x, w, g, b['dw'], B.WIN_WIDTH, accumulate=acc)


def judge_wgrad(CP, c):
    """every launch form of case `c` (module docstring): last_conv, last_gemm where the case names a GEMM, and every
    element of every output of every set of buffers; returns the misses"""
    rt = CP.runtime()
    p = c.problem
    options = dict(DEFAULTS)
    options.update(GEMM_DEFAULTS)
    options.update(c.opts)
    for key, value in options.items():
        rt.set_option(key, value)
    CP.set_dtype(p.dtype)
    call = wgrad_call(CP, c)
    cu = rt.device_info()['cu_count']
    failures = []
    try:
        for cap in CAPS:
            for accumulate in (False, True):
                tols = p.tolerances(accumulate)
                for deferred in (False, True):
                    what = f'{c.id} max_blocks={cap} accumulate={accumulate} ' + ('deferred' if deferred else 'own finish')
                    sets = [{k: CP.copy(p.init[k], np.float32) if accumulate else CP.empty(p.ref[k].shape, np.float32)
                             for k in p.outputs} for _ in range(2 if deferred else 1)]
                    rt.set_option('max_blocks', cap)
                    try:
                        with rt.defer_wgrad() if deferred else contextlib.nullcontext():
                            for buffers in sets:
                                call(buffers, accumulate)
                                noted = rt.last_conv()
                                if c.kernel is not None and noted != (c.kernel[0], KID[c.kernel[1]]):
                                    failures.append(f'{what}: last_conv {noted} ({KERNELS[noted[1]]}) != {c.kernel}')
                    finally:
                        rt.set_option('max_blocks', 0)
                    if c.gemm is not None:
                        got = rt.last_gemm()
                        if deferred:
                            splits = expect_group([c.gemm] * len(sets), cu, WS_HALF, 0, options['split_blocks'],
                                                  options['split_min'])
                            want, group = (64, 0, 0, max(splits)), (len(sets), sum(s > 1 for s in splits))
                            if rt.last_gemm_group() != group:
                                failures.append(f'{what}: last_gemm_group {rt.last_gemm_group()} != {group}')
                        else:
                            want = expect_gemm(*c.gemm, True, cu, WS_HALF, options)
                        print(f'{what}: last_gemm {got}')
                        if got != want or want[3] < 2:
                            failures.append(f'{what}: last_gemm {got} != host rule {want} with two or more slabs')
                    for i, buffers in enumerate(sets):
                        for name in p.outputs:
                            host = CP.asnumpy(buffers[name])
                            want, tol = p.expected(name, accumulate), tols[name]
                            assert host.shape == want.shape and host.dtype == np.float32, (what, name, host.shape, host.dtype)
                            r = W.ratio(host, want, tol)
                            at = tuple(int(j) for j in np.unravel_index(np.argmax(r), r.shape))
                            print(f'{what} set {i} {name}: largest err / tol {r.max():.3f} at {at} (rel_linf '
                                  f'{rel_linf(np.nan_to_num(host.astype(np.float64)), want):.2e}, NaN {int(np.isnan(host).sum())})')
                            if not r.max() <= 1.0:
                                failures.append(f'{what} set {i} {name}: err / tol = {r.max():.3f} at {at}, '
                                                f'{int((r > 1.0).sum())} of {r.size} elements over')
    finally:
        for key, value in GEMM_DEFAULTS:
            rt.set_option(key, value)
    return failures


@pytest.mark.parametrize('index', range(len(W.WCASES)), ids=W.WCASE_IDS)
def test_every_weight_gradient_element_within_the_derived_bound(index, ctx):
    """dw / db of every weight-gradient kernel under tol = gamma(n + 8) S + u32 |init + ref| (elementwise_wgrad.py), in
    every launch form: max_blocks 0 and 3, overwriting and accumulating, the producer's own finish and the deferred
    group with two recorded calls."""
    failures = judge_wgrad(ctx, W.WCASES[index])
    assert not failures, '\n'.join(failures)


# ---- the binary16 pair at its own roundings ----------------------------------------------------------------------------------
def pair16_launch(CP, st):
    """bwd(buffers, accumulate, need_dx) -> dx or None: conv_pair_bwd on the device operands of Pair16Steps `st`"""
    from univer_ocr_amd.hip import lib as hiplib
    from univer_ocr_amd.nn import ops
    q = st.base.q
    x, yout, g = CP.copy(q['x']), CP.copy(st.yout), CP.copy(st.g_dev)
    g.gscale = st.gscale                        # dy is stored times 2^k; the kernels divide dw / db by it, dx keeps it
    w1, b1, w2 = (CP.copy(q[k], np.float32) for k in ('w1', 'b1', 'w2'))
    act2 = hiplib.ACT_SIGMOID if st.sig else hiplib.ACT_NONE
    return lambda b, acc, need_dx: ops.conv_pair_bwd(x, yout, g, w1, b1, w2, b['dw1'], b['db1'], b['dw2'], b['db2'], st.pad1,
                                                     True, True, B.ALPHA, act2, need_dx=need_dx, accumulate=acc)


def pair16_forms(st):
    """the option sets of a case: pair_band 0 and 2 (three rows: two bands, the second with one row), and for the wave
    kernel pair_g 4 and 2"""
    return [dict(pair_band=band, pair_g=g) for band in (0, 2) for g in ((4, 2) if st.kernel == 'wave' else (4,))]


def judge_dx16(CP, st, dx, what, failures):
    host = CP.asnumpy(dx)
    ref, tol = st.ref['dx'], st.tolerances()['dx']
    assert host.shape == ref.shape and host.dtype == np.float16 and dx.gscale == st.gscale, (what, host.shape, host.dtype)
    r = W.ratio(host, ref, tol)
    at = tuple(int(j) for j in np.unravel_index(np.argmax(r), r.shape))
    print(f'{what} dx: largest err / tol {r.max():.3f} at {at} (rel_linf '
          f'{rel_linf(np.nan_to_num(host.astype(np.float64)), ref):.2e}, NaN {int(np.isnan(host).sum())})')
    if not r.max() <= 1.0:
        failures.append(f'{what} dx: err / tol = {r.max():.3f} at {at}, {int((r > 1.0).sum())} of {r.size} pixels over')


def set_pair_options(rt, opts):
    for key in ('pair_band', 'pair_g'):
        rt.set_option(key, opts.get(key, EXTRA_DEFAULTS[key]))


@pytest.mark.parametrize('index', range(len(W.PAIR16_KEYS)), ids=W.PAIR16_IDS)
def test_binary16_pair_weight_gradients_within_the_bound_at_their_roundings(index, ctx):
    """dw1, db1, dw2, db2 of pair_strip_bwd_h_kernel and pair_wave_bwd_h_kernel element by element against the kernel's own
    rounding points restated in float64, every binary16 rounding of a float32 value an interval (elementwise_wgrad.
    PairWgrad16Problem): pair_band 0 and 2, pair_g 4 and 2 (wave kernel), need_dx True and False (with dx judged as
    stored), overwriting NaN-filled buffers and accumulating onto init = float32(ref r), with the producer's finish and
    inside `rt.defer_wgrad()` issued twice; after each launch `Runtime.last_pair` must be what
    test_gpu_pair_forms.expect_pair predicts (kernel 5: wave, 4: cooperative)."""
    p = W.pair16_problem(*W.PAIR16_KEYS[index])
    st, rt = p.steps, ctx.runtime()
    for key, value in DEFAULTS:
        rt.set_option(key, value)
    ctx.set_dtype('float16')
    call = pair16_launch(ctx, st)
    cu = rt.device_info()['cu_count']
    n, h, w = st.base.shape
    failures, worst = [], {}
    try:
        for opts in pair16_forms(st):
            set_pair_options(rt, opts)
            want = expect_pair('bwd', 'float16', n, h, w, st.pad1, opts, cu)[0]
            assert want[0] == (5 if st.kernel == 'wave' else 4), want
            for need_dx in (True, False):
                for accumulate in (False, True):
                    tols = p.tolerances(accumulate)
                    for deferred in (False, True):
                        what = f'{W.PAIR16_IDS[index]} {opts} need_dx={need_dx} accumulate={accumulate} ' + \
                            ('deferred' if deferred else 'own finish')
                        sets = [{k: ctx.copy(p.init[k], np.float32) if accumulate else ctx.empty(p.ref[k].shape, np.float32)
                                 for k in p.outputs} for _ in range(2 if deferred else 1)]
                        dxs = []
                        with rt.defer_wgrad() if deferred else contextlib.nullcontext():
                            for buffers in sets:
                                dxs.append(call(buffers, accumulate, need_dx))
                                if rt.last_pair() != want:
                                    failures.append(f'{what}: last_pair {rt.last_pair()} != host rule {want}')
                        for i, (buffers, dx) in enumerate(zip(sets, dxs)):
                            if need_dx:
                                judge_dx16(ctx, st, dx, f'{what} set {i}', failures)
                            else:
                                assert dx is None
                            for name in p.outputs:
                                host = ctx.asnumpy(buffers[name])
                                expect, tol = p.expected(name, accumulate), tols[name]
                                assert host.shape == expect.shape and host.dtype == np.float32, (what, name, host.shape, host.dtype)
                                r = W.ratio(host, expect, tol)
                                at = tuple(int(j) for j in np.unravel_index(np.argmax(r), r.shape))
                                worst[name] = max(worst.get(name, 0.0), float(r.max()))
                                print(f'{what} set {i} {name}: largest err / tol {r.max():.3f} at {at} (rel_linf '
                                      f'{rel_linf(np.nan_to_num(host.astype(np.float64)), expect):.2e}, NaN {int(np.isnan(host).sum())})')
                                if not r.max() <= 1.0:
                                    failures.append(f'{what} set {i} {name}: err / tol = {r.max():.3f} at {at}, '
                                                    f'{int((r > 1.0).sum())} of {r.size} elements over')
    finally:
        set_pair_options(rt, {})
    print(f'{W.PAIR16_IDS[index]}: largest err / tol over all forms ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()))
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('index', range(len(B.PAIR_WAVE_DX_KEYS)), ids=B.PAIR_WAVE_DX_IDS)
def test_pair_wave_dx_every_pixel_within_the_bound_at_its_roundings(index, ctx):
    """dx of pair_wave_bwd_h_kernel (pages wider than 512 columns) with every pixel judged at the kernel's own roundings
    (elementwise_bound.PairWaveDxProblem), with and without accumulation of the weight gradients, in the default bands,
    with one band per image and with pair_g 2; `Runtime.last_pair` must report kernel 5 in the form the host rules give."""
    c = B.pair_wave_dx_case(index)
    p, st, rt = c.problem, c.problem.steps, ctx.runtime()
    for key, value in DEFAULTS:
        rt.set_option(key, value)
    ctx.set_dtype('float16')
    call = pair16_launch(ctx, st)
    cu = rt.device_info()['cu_count']
    n, h, w = st.base.shape
    failures = []
    try:
        for opts in ({}, {'pair_band': h}, {'pair_g': 2}):
            set_pair_options(rt, opts)
            want = expect_pair('bwd', 'float16', n, h, w, st.pad1, opts, cu)[0]
            assert want[0] == 5, want
            for accumulate in (False, True):
                grads = {k: ctx.full(st.ref[k].shape, 0.0, np.float32) for k in ('dw1', 'db1', 'dw2', 'db2')}
                dx = call(grads, accumulate, True)
                what = f'{c.id} {opts} accumulate={accumulate}'
                if rt.last_pair() != want:
                    failures.append(f'{what}: last_pair {rt.last_pair()} != host rule {want}')
                judge_dx16(ctx, st, dx, what, failures)
    finally:
        set_pair_options(rt, {})
    assert not failures, '\n'.join(failures)
