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

The largest err / tol of every output is printed before it is judged.
"""
import numpy as np
import pytest

import elementwise_bound as B
from conftest import rel_linf
from test_gpu_conv_padding import DEFAULTS, DGRAD, FWD, KERNELS, KID, ctx  # noqa: F401  (ctx: the NaN-filling fixture)

pytestmark = pytest.mark.gpu

CAPS = (0, 3)
EXTRA_DEFAULTS = dict(act_dispatch=1, pair_band=0)       # options a test sets on top of a case's own, and their defaults


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
