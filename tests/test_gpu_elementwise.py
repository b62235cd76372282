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

Left out:
  Sigmoid epilogues   the error of expf is not part of the bound; the existing tests keep them;
  binary16 pair dx    with roundings of 2^-11 the share of undecided slopes is far above 1 %.

The largest err / tol of every output is printed before it is judged.
"""
import numpy as np
import pytest

import elementwise_bound as B
from conftest import rel_linf
from test_gpu_conv_padding import DEFAULTS, DGRAD, FWD, KERNELS, KID, ctx  # noqa: F401  (ctx: the NaN-filling fixture)

pytestmark = pytest.mark.gpu

CAPS = (0, 3)


def launches(CP, c):
    """{output: (launch(), conv entry or None)} for the case's problem on the device"""
    from univer_ocr_amd.hip import lib as hiplib
    from univer_ocr_amd.nn import ops
    p, q = c.problem, c.problem.q
    dev = lambda k: CP.copy(q[k])
    par = lambda k: CP.copy(q[k], np.float32)
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


@pytest.mark.parametrize('index', range(len(B.CASES)), ids=B.CASE_IDS)
def test_every_element_within_the_derived_bound(index, ctx):
    CP, rt = ctx, ctx.runtime()
    c = B.CASES[index]
    p = c.problem
    for key, value in DEFAULTS:
        rt.set_option(key, c.opts.get(key, value))
    CP.set_dtype(p.dtype)
    run = launches(CP, c)
    tols = p.tolerances(c.operand16)
    failures = []
    for name in c.outputs:
        launch, entry = run[name]
        ref, tol, judged = p.ref[name], tols[name], p.judged(name)
        for cap in CAPS:
            rt.set_option('max_blocks', cap)
            try:
                got = launch()
                noted = rt.last_conv()
            finally:
                rt.set_option('max_blocks', 0)
            what = f'{c.id} {name} max_blocks={cap}'
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
    assert not failures, '\n'.join(failures)
