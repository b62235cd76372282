"""The float32 MFMA GEMM (univer-ocr_amd/csrc/gemm_mfma.hip) across its run-time configuration space, against the
float64 oracle.

At the shapes of the other parity tests the host picks one configuration per GEMM: 64-row tiles, and a depth split
that follows the CU count.  Here the context options steer every choice of `launch_mfma` -- "gemm_bm" (64 / 128-row
tiles), "split_blocks" / "split_min" (unsplit, 2 slabs, 3 slabs with a shorter last one, the slab cap), "xcd_remap"
(block renumbering on / off) -- and `Runtime.last_gemm` (uocr_ctx_last_gemm) must report what a Python copy of the
host rule predicts, so that a forced option that the cap or "split_min" undoes cannot pass unnoticed.  Every form of
the GEMM is swept: conv forward (AConvFwd), conv dx (AConvDgrad, with whole depth tiles skipped for strided convs),
conv dw/db (AConvWgrad with and without the cursor), dense forward / dx / dw, the windows + dense layer of the Char
net, operands off 16-byte alignment (the element-wise loads), a very deep dw at the 256-slab cap, a small workspace
(slab clamp, dx off the MFMA path, group refusals) and the deferred weight-gradient group ("group_blocks", overflow
past 8 problems / 4 of a kind, calls that accumulate into one gradient).

What each configuration must give:
  * y and dx within 1e-5 of the oracle, dw and db within 2e-5 (normalised max error);
  * at one slab count, the same bits whatever the row tile and the block numbering: every output element is the
    same chain of MFMAs over the same depth tiles, and the reduce adds the slabs in a fixed order.
Every array the ops allocate starts as NaN, so an output tile that no block writes cannot pass.
"""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

from conftest import rel_linf
from oracle import nn_oracle as O

pytestmark = pytest.mark.gpu

TOL_Y = 1e-5            # y, dx
TOL_W = 2e-5            # dw, db
BN, BD = 64, 32         # output-tile width and depth tile of the kernel
GEMM_DEFAULTS = (('gemm_bm', 0), ('split_blocks', 1024), ('split_min', 3), ('xcd_remap', 1), ('group_blocks', 0))
DEFAULTS = GEMM_DEFAULTS + (('mfma', 1), ('fast_paths', 1))
WS_HALF = (int(os.environ.get('UOCR_WORKSPACE_MB', '256')) << 20) // 2      # Runtime's workspace, halved (slabs)


def _restore(CP):
    rt = CP.runtime()
    for key, value in DEFAULTS:
        rt.set_option(key, value)
    CP.set_dtype('float32')


@pytest.fixture
def ctx(monkeypatch):
    """The shared context with the defaults restored on both sides, MFMA whenever eligible and no shape-specialised
    kernels; every array the ops allocate is filled with NaN."""
    from univer_ocr_amd.nn import CP
    from univer_ocr_amd.nn import gpu
    CP.use_gpu(0)
    _restore(CP)
    rt = CP.runtime()
    rt.set_option('mfma', 2)
    rt.set_option('fast_paths', 0)
    empty = CP.empty

    def poisoned(shape, dtype=None):
        out = empty(shape, dtype)
        if out.t.is_cuda and out.t.dtype in gpu._CODE and out.size:
            CP.runtime().call('uocr_fill', gpu._CODE[out.t.dtype], out.ptr, float('nan'), out.size)
        return out

    monkeypatch.setattr(CP, 'empty', staticmethod(poisoned))
    yield CP
    monkeypatch.undo()
    _restore(CP)


def cdiv(a, b):
    return (a + b - 1) // b


def host(a):
    from univer_ocr_amd.nn import CP
    return CP.asnumpy(a).astype(np.float64)


def check(a, ref, tol, what):
    got = host(a) if not isinstance(a, np.ndarray) else a
    assert not np.isnan(got).any(), f'{what}: {int(np.isnan(got).sum())} NaN (an output element nobody wrote)'
    err = rel_linf(got, ref)
    assert err <= tol, f'{what}: rel_linf={err:.3e} > {tol:.1e}'


def cu_count(CP):
    return CP.runtime().device_info()['cu_count']


# ---- Python copies of the host rules (gemm_mfma.hip) -------------------------------------------------------------------
def expect_gemm(M, N, depth, allow_split, cu, ws_half, opt):
    """launch_mfma: (bm, gm, gn, nsplit) under the options `opt`."""
    ntiles = cdiv(depth, BD)
    tiles128 = cdiv(M, 128) * cdiv(N, BN)
    deep = min(256, ntiles // 32) if allow_split and opt['split_blocks'] > 0 else 1
    bm = 128 if tiles128 >= 512 or tiles128 * deep >= 512 else 64
    if opt['gemm_bm'] in (64, 128):
        bm = opt['gemm_bm']
    gm, gn = cdiv(M, bm), cdiv(N, BN)
    nsplit = 1
    split = opt['split_blocks']
    target = cu * (3 if bm == 128 else 4) if split == 1024 else split
    if allow_split and target > 0 and gm * gn < target and ntiles >= 4:
        nsplit = max(1, target // (gm * gn)) if split == 1024 else cdiv(target, gm * gn)
        nsplit = min(nsplit, max(min(32, ntiles // 2), min(256, ntiles // 32)))
        if nsplit * M * N * 4 > ws_half:
            nsplit = ws_half // (M * N * 4)
        nsplit = max(nsplit, 1)
        if nsplit < opt['split_min']:
            nsplit = 1
    tps = cdiv(ntiles, nsplit)
    return bm, gm, gn, cdiv(ntiles, tps)


def expect_group(problems, cu, ws_half, group_blocks, split_blocks, split_min):
    """defer_flush: the slab count of every recorded problem (M, N, depth), in recording order."""
    shapes = [(cdiv(M, 64), cdiv(N, BN), cdiv(depth, BD), M * N) for M, N, depth in problems]
    work = [float(gx) * gy * nt for gx, gy, nt, _ in shapes]
    total = 0.0
    for w in work:
        total += w
    target = 0.0 if split_blocks <= 0 else float(group_blocks) if group_blocks > 0 else 4.0 * cu
    slab_floats, out = 0, []
    for (gx, gy, nt, per), w in zip(shapes, work):
        nsplit = int(target * w / total / (gx * gy) + 0.5)
        nsplit = max(1, min(nsplit, max(min(32, nt // 2), min(256, nt // 32))))
        while nsplit > 1 and (slab_floats + nsplit * per) * 4 > ws_half:
            nsplit -= 1
        if nsplit < split_min:
            nsplit = 1
        nsplit = cdiv(nt, cdiv(nt, nsplit))
        if nsplit > 1:
            slab_floats += nsplit * per
        out.append(nsplit)
    return out


def conv_gemms(xs, ks, cout, st, pd, ws_half=WS_HALF):
    """(M, N, depth, allow_split) of the forward, dx and dw GEMMs of a conv (uocr_conv_*_mfma), dw with a bias row."""
    n, h, w, cin = xs
    (kh, kw), (sh, sw), (ph, pw) = ks, st, pd
    oh, ow = O.conv2d_out_hw(h, w, ks, st, pd)
    M_f, D_x = n * oh * ow, kh * kw * cout
    live = sum(1 for iy in range(h) for ky in range(kh)
               if iy + ph - ky >= 0 and (iy + ph - ky) % sh == 0 and (iy + ph - ky) // sh < oh)
    live_tiles = cdiv(D_x, BD) * live // (h * kh)
    return ((M_f, cout, kh * kw * cin, M_f * cout * 32 <= ws_half),
            (n * h * w, cin, D_x, n * h * w * cin * 32 <= ws_half and live_tiles >= 12),
            (kh * kw * cin + 1, cout, n * oh * ow, True))


def configurations(M, N):
    """gemm_bm x {unsplit, 2 slabs, 3 slabs, the cap} x xcd_remap, then the automatic choice."""
    out = []
    for bm in (64, 128):
        tiles = cdiv(M, bm) * cdiv(N, BN)
        for split, smin in ((0, 3), (2 * tiles, 2), (3 * tiles, 2), (1 << 24, 2)):
            for xcd in (0, 1):
                out.append(dict(gemm_bm=bm, split_blocks=split, split_min=smin, xcd_remap=xcd, group_blocks=0))
    out.append(dict(GEMM_DEFAULTS))
    return out


def set_gemm_options(rt, opt):
    for key, value in opt.items():
        rt.set_option(key, value)


def sweep(CP, run, gemm, refs, what):
    """run() under every configuration; `gemm` = (M, N, depth, allow_split) of the GEMM whose choice last_gemm reports
    after run(); `refs` = [(reference, tolerance, name)] for run()'s outputs.  Returns the slab counts seen."""
    rt = CP.runtime()
    M, N, depth, allow = gemm
    cu = cu_count(CP)
    first, seen = {}, set()
    try:
        for opt in configurations(M, N):
            set_gemm_options(rt, opt)
            outs = run()
            got, exp = rt.last_gemm(), expect_gemm(M, N, depth, allow, cu, WS_HALF, opt)
            assert got == exp, f'{what} {opt}: last_gemm {got} != host rule {exp}'
            seen.add(got[3])
            tag = f'{what} bm={got[0]} slabs={got[3]} xcd_remap={opt["xcd_remap"]} split_blocks={opt["split_blocks"]}'
            hs = [host(o) for o in outs]
            for h, (ref, tol, name) in zip(hs, refs):
                check(h, ref, tol, f'{name} [{tag}]')
            base = first.setdefault(got[3], (tag, hs))
            for h, h0, (_, _, name) in zip(hs, base[1], refs):
                assert np.array_equal(h, h0), f'{name}: [{tag}] differs from [{base[0]}] ' \
                    f'(max |diff| {np.max(np.abs(h - h0)):.3e})'
    finally:
        set_gemm_options(rt, dict(GEMM_DEFAULTS))
    want = reachable_slabs(M, N, depth, allow)
    assert want <= seen, f'{what}: slab counts {sorted(seen)} miss {sorted(want - seen)}'
    return seen


def reachable_slabs(M, N, depth, allow):
    """the slab counts the sweep must have run: unsplit, 2 (>= 4 depth tiles), 3 (>= 6) and the cap"""
    ntiles = cdiv(depth, BD)
    if not allow or ntiles < 4:
        return {1}
    cap = expect_gemm(M, N, depth, True, 256, WS_HALF, dict(gemm_bm=64, split_blocks=1 << 24, split_min=2))[3]
    return {1, 2, cap} | ({3} if ntiles >= 6 else set())


def slab_lengths(depth, nsplit):
    ntiles = cdiv(depth, BD)
    tps = cdiv(ntiles, nsplit)
    return [min(ntiles, (z + 1) * tps) - z * tps for z in range(cdiv(ntiles, tps))]


# ---- convolutions --------------------------------------------------------------------------------------------------
# forward: (x shape, kernel, cout, stride, padding, pad_value, bias, fused act): 1, 2 and 3 depth tiles per tap;
# 10 depth tiles in the first (3 slabs of 4, 4, 2)
FWD = [
    ((2, 9, 11, 32), (5, 2), 40, (1, 1), (2, 0), 0.25, True, 'leaky'),
    ((3, 10, 13, 64), (3, 3), 64, (2, 1), (1, 1), 0.0, False, 'sigmoid'),
    ((2, 8, 7, 96), (2, 3), 132, (1, 1), (1, 1), -0.5, True, 'leaky'),
]


def act_ref(kind, z):
    return O.leaky_relu_fwd(z, 0.01) if kind == 'leaky' else O.sigmoid_fwd(z)


@pytest.mark.parametrize('case', range(len(FWD)))
def test_conv_forward_configs(case, ctx):
    from univer_ocr_amd.nn import ops
    CP = ctx
    xs, ks, cout, st, pd, pv, bias, act = FWD[case]
    rng = np.random.default_rng(500 + case)
    X = rng.standard_normal(xs)
    w = rng.standard_normal((*ks, xs[3], cout)) * 0.1
    b = rng.standard_normal(cout)
    ref = O.conv2d_fwd(X, w, b, st, pd, pv, bias)
    Xd, wd, bd = CP.copy(X), CP.copy(w), CP.copy(b)
    gemm = conv_gemms(xs, ks, cout, st, pd)[0]
    if case == 0:
        assert slab_lengths(gemm[2], 3) == [4, 4, 2]
    sweep(CP, lambda: (ops.conv2d_fwd(Xd, wd, bd, st, pd, pv, bias),
                       ops.conv2d_fwd(Xd, wd, bd, st, pd, pv, bias, act=act, alpha=0.01)),
          gemm, [(ref, TOL_Y, 'y'), (act_ref(act, ref), TOL_Y, f'{act}(y)')], f'fwd {xs}')


# dx: (x shape, kernel, cout, stride, padding, mask act).  Stride 1; strides (2, 1) / (3, 2) at w = 64 / 128 (the rows of
# a block lie in one image row: whole depth tiles are skipped with 64-row tiles, and with 128-row tiles at w = 128);
# w = 96 (some blocks straddle two rows: nothing is skipped).  Every strided case has top rows with ty < 0 and bottom
# rows whose tap row lands at gy >= oh.
DGRAD = [
    ((2, 9, 11, 40), (3, 3), 64, (1, 1), (1, 1), 'leaky'),
    ((2, 10, 64, 32), (5, 3), 64, (2, 1), (2, 1), 'sigmoid'),
    ((1, 12, 128, 16), (5, 3), 96, (3, 2), (1, 1), 'leaky'),
    ((1, 12, 64, 16), (5, 3), 96, (3, 2), (1, 1), 'sigmoid'),
    ((1, 9, 128, 8), (5, 3), 64, (2, 1), (2, 1), 'leaky'),
    ((2, 8, 96, 8), (5, 3), 64, (2, 1), (2, 1), 'sigmoid'),
]


def mask_of(kind, rng, shape):
    """x_act (the conv input as the output of `kind`) and act'(x_act)"""
    if kind == 'leaky':
        m = rng.standard_normal(shape)
        return m, np.where(m >= 0, 1.0, 0.01)
    m = rng.random(shape) * 0.9 + 0.05
    return m, m * (1 - m)


@pytest.mark.parametrize('case', range(len(DGRAD)))
def test_conv_dgrad_configs(case, ctx):
    from univer_ocr_amd.nn import ops
    CP = ctx
    xs, ks, cout, st, pd, kind = DGRAD[case]
    n, h, wd_, cin = xs
    oh, ow = O.conv2d_out_hw(h, wd_, ks, st, pd)
    if st[0] > 1:      # (the edges the skip test must get right: tap rows above the image and below the output)
        assert any(y + pd[0] - ky < 0 for y in range(h) for ky in range(ks[0]))
        assert any((y + pd[0] - ky) % st[0] == 0 and (y + pd[0] - ky) // st[0] >= oh
                   for y in range(h) for ky in range(ks[0]) if y + pd[0] - ky >= 0)
    rng = np.random.default_rng(600 + case)
    X = rng.standard_normal(xs)
    w = rng.standard_normal((*ks, cin, cout)) * 0.1
    g = rng.standard_normal((n, oh, ow, cout))
    ref, _, _ = O.conv2d_bwd(X, w, g, st, pd, 0.0, True)
    m, slope = mask_of(kind, rng, xs)
    gd, wd, md = CP.copy(g), CP.copy(w), CP.copy(m)
    gemm = conv_gemms(xs, ks, cout, st, pd)[1]
    sweep(CP, lambda: (ops.conv2d_bwd_data(gd, wd, xs, st, pd),
                       ops.conv2d_bwd_data(gd, wd, xs, st, pd, x_act=md, act=kind, alpha=0.01)),
          gemm, [(ref, TOL_Y, 'dx'), (ref * slope, TOL_Y, f'{kind}-masked dx')], f'dx {xs} stride {st}')


# dw/db: (x shape, kernel, cout, stride, padding, pad_value, bias).  ow >= 32: the cursor, with row wraps every ow pixels
# and an image wrap inside a slab; ow < 32: the divisions per load.
WGRAD = [
    ((2, 4, 40, 16), (3, 3), 24, (1, 1), (1, 1), 0.0, True),      # 10 depth tiles: slabs of 4, 4, 2; image wrap at 160
    ((2, 9, 70, 8), (3, 3), 20, (2, 2), (1, 1), 0.5, False),      # ow = 35
    ((3, 7, 9, 12), (3, 2), 36, (1, 1), (1, 0), -0.25, True),      # ow = 8: no cursor
    ((2, 6, 20, 32), (3, 3), 72, (1, 1), (1, 1), 0.0, False),      # ow = 20: no cursor; N = 72 (two column tiles)
]


@pytest.mark.parametrize('case', range(len(WGRAD)))
def test_conv_wgrad_configs(case, ctx):
    from univer_ocr_amd.nn import ops
    CP = ctx
    xs, ks, cout, st, pd, pv, bias = WGRAD[case]
    n, h, wd_, cin = xs
    oh, ow = O.conv2d_out_hw(h, wd_, ks, st, pd)
    rng = np.random.default_rng(700 + case)
    X = rng.standard_normal(xs)
    g = rng.standard_normal((n, oh, ow, cout))
    _, ref_dw, ref_db = O.conv2d_bwd(X, np.zeros((*ks, cin, cout)), g, st, pd, pv, bias)
    Xd, gd = CP.copy(X), CP.copy(g)
    wshape = (*ks, cin, cout)
    M, N, depth, allow = conv_gemms(xs, ks, cout, st, pd)[2]
    gemm = (M - (0 if bias else 1), N, depth, allow)
    if case == 0:
        assert slab_lengths(depth, 3) == [4, 4, 2] and ow >= BD

    def acc():
        dw, db = CP.full(wshape, 0.5, np.float32), CP.full((cout,), 0.25, np.float32)
        ops.conv2d_bwd_weight(Xd, gd, dw, db, st, pd, pv, bias, accumulate=True)
        return dw, db

    def over():
        dw, db = CP.empty(wshape, np.float32), CP.empty((cout,), np.float32)      # NaN: nothing may be read
        ops.conv2d_bwd_weight(Xd, gd, dw, db, st, pd, pv, bias, accumulate=False)
        return dw, db

    sweep(CP, acc, gemm, [(ref_dw + 0.5, TOL_W, 'dw (onto 0.5)'), (ref_db + 0.25, TOL_W, 'db (onto 0.25)')],
          f'dw {xs}')
    sweep(CP, over, gemm, [(ref_dw, TOL_W, 'dw (overwritten)'), (ref_db, TOL_W, 'db (overwritten)')], f'dw {xs}')


def test_very_deep_wgrad_reaches_the_slab_cap(ctx):
    """dw of a 3x3 16 -> 16 conv over 4 x 256 x 256 output pixels (8192 depth tiles, through the cursor): with a large
    split_blocks the split stops at the 256-slab cap; so does the automatic choice, with 128-row tiles."""
    from univer_ocr_amd.nn import ops
    CP = ctx
    rt = CP.runtime()
    xs, cout = (4, 256, 256, 16), 16
    rng = np.random.default_rng(800)
    X = rng.standard_normal(xs).astype(np.float32)
    g = rng.standard_normal((*xs[:3], cout)).astype(np.float32)
    Xp = np.pad(X.astype(np.float64), ((0, 0), (1, 1), (1, 1), (0, 0)))
    g2 = g.reshape(-1, cout).astype(np.float64)
    ref_dw = np.stack([np.stack([Xp[:, ky:ky + 256, kx:kx + 256, :].reshape(-1, 16).T @ g2 for kx in range(3)])
                       for ky in range(3)])                                      # float64, tap by tap
    ref_db = g2.sum(axis=0)
    Xd, gd = CP.copy(X, np.float32), CP.copy(g, np.float32)
    M, N, depth = 145, cout, 4 * 256 * 256
    cu = cu_count(CP)
    try:
        for opt in (dict(gemm_bm=64, split_blocks=1 << 20, split_min=3, xcd_remap=1, group_blocks=0),
                    dict(GEMM_DEFAULTS)):
            set_gemm_options(rt, opt)
            dw, db = CP.full((3, 3, 16, cout), 0.5, np.float32), CP.full((cout,), 0.25, np.float32)
            ops.conv2d_bwd_weight(Xd, gd, dw, db, (1, 1), (1, 1), 0.0, True, accumulate=True)
            got = rt.last_gemm()
            assert got == expect_gemm(M, N, depth, True, cu, WS_HALF, opt) and got[3] == 256, (opt, got)
            check(dw, ref_dw + 0.5, TOL_W, f'dw {opt}')
            check(db, ref_db + 0.25, TOL_W, f'db {opt}')
    finally:
        set_gemm_options(rt, dict(GEMM_DEFAULTS))


# ---- dense layers ----------------------------------------------------------------------------------------------------
def dense_call(CP, x, w, dy, dx, dw, accumulate, x_act=None):
    """uocr_dense_bwd_act with dx or dw left out, so that last_gemm reports the GEMM of the one that is asked for."""
    from univer_ocr_amd.nn import ops
    m, n_in = x.shape
    CP.runtime().call('uocr_dense_bwd_act', 0, x.ptr, w.ptr, dy.ptr, None if dx is None else dx.ptr,
                      None if dw is None else dw.ptr, m, n_in, w.shape[1], int(accumulate), ops.ACT_CODES[x_act], 0.01)


DENSE = [(300, 200, 162), (100, 96, 64), (37, 64, 64)]       # (m, n_in, n_out)


def dense_problem(rng, m, n_in, n_out):
    X = rng.standard_normal((m, n_in))
    w = rng.standard_normal((n_in + 1, n_out)) * 0.1
    g = rng.standard_normal((m, n_out))
    return X, w, g


@pytest.mark.parametrize('case', range(len(DENSE)))
def test_dense_configs(case, ctx):
    """dense forward (ARowMajor with the ones column), dx (BDepthContig) and dw (AColMajor with the ones row)."""
    from univer_ocr_amd.nn import ops
    CP = ctx
    m, n_in, n_out = DENSE[case]
    rng = np.random.default_rng(900 + case)
    X, w, g = dense_problem(rng, m, n_in, n_out)
    ref_y = O.dense_fwd(X, w)
    ref_dx, ref_dw = O.dense_bwd(X, w, g)
    Xd, wd, gd = CP.copy(X), CP.copy(w), CP.copy(g)
    slope = np.where(X >= 0, 1.0, 0.01)
    sweep(CP, lambda: (ops.dense_fwd(Xd, wd), ops.dense_fwd(Xd, wd, act='sigmoid')), (m, n_out, n_in + 1, True),
          [(ref_y, TOL_Y, 'y'), (O.sigmoid_fwd(ref_y), TOL_Y, 'sigmoid(y)')], f'dense fwd {DENSE[case]}')

    def dx():
        out, outm = CP.empty((m, n_in)), CP.empty((m, n_in))
        dense_call(CP, Xd, wd, gd, out, None, False)
        dense_call(CP, Xd, wd, gd, outm, None, False, x_act='leaky')
        return out, outm

    sweep(CP, dx, (m, n_in, n_out, True), [(ref_dx, TOL_Y, 'dx'), (ref_dx * slope, TOL_Y, 'leaky-masked dx')],
          f'dense dx {DENSE[case]}')

    def dw_acc():
        out = CP.full(w.shape, 0.5)
        dense_call(CP, Xd, wd, gd, None, out, True)
        return (out,)

    def dw_over():
        out = CP.empty(w.shape)
        dense_call(CP, Xd, wd, gd, None, out, False)
        return (out,)

    gemm = (n_in + 1, n_out, m, True)
    sweep(CP, dw_acc, gemm, [(ref_dw + 0.5, TOL_W, 'dw (onto 0.5)')], f'dense dw {DENSE[case]}')
    sweep(CP, dw_over, gemm, [(ref_dw, TOL_W, 'dw (overwritten)')], f'dense dw {DENSE[case]}')


def test_windows_dense_configs(ctx):
    """The Char net's windows + flatten + dense layer as one implicit conv GEMM (ops.windows_dense_*)."""
    from univer_ocr_amd.nn import ops
    CP = ctx
    xs, width, n_out = (2, 3, 20, 32), 8, 64
    rng = np.random.default_rng(950)
    X = rng.standard_normal(xs)
    W = rng.standard_normal((xs[1] * width * xs[3] + 1, n_out)) * 0.1
    G = rng.standard_normal((xs[0] * xs[2], n_out))
    windows = O.fixed_width_fwd(X, width)
    flat = windows.reshape(xs[0] * xs[2], -1)
    ref_y = O.dense_fwd(flat, W)
    dflat, ref_dw = O.dense_bwd(flat, W, G)
    ref_dx = O.fixed_width_bwd(dflat.reshape(windows.shape), xs, width)
    Xd, Wd, Gd = CP.copy(X), CP.copy(W), CP.copy(G)
    fwd, dgrad, wgrad = conv_gemms(xs, (xs[1], width), n_out, (1, 1), (0, width // 2))
    fwd = (xs[0] * xs[2],) + fwd[1:]                    # (the output is cut to W columns)
    sweep(CP, lambda: (ops.windows_dense_fwd(Xd, Wd, width, act='leaky', alpha=0.01),),
          fwd, [(O.leaky_relu_fwd(ref_y, 0.01), TOL_Y, 'leaky(y)')], 'windows fwd')

    def bwd():
        dw = CP.full(W.shape, 0.5)
        dx = ops.windows_dense_bwd(Xd, Wd, Gd, dw, width, accumulate=True)
        return dx, dw

    # (bwd runs dw, then dx: last_gemm reports the dx GEMM; dw is checked against the oracle in every configuration)
    sweep(CP, bwd, dgrad, [(ref_dx, TOL_Y, 'dx'), (ref_dw + 0.5, TOL_W, 'dw (onto 0.5)')], 'windows bwd')
    assert wgrad[0] == W.shape[0]


# ---- operands off 16-byte alignment (the element-wise loads of the loaders that check it) ---------------------------
def misaligned(CP, a):
    """a DeviceArray 4 bytes past a 16-byte boundary holding `a` (float32)"""
    import torch
    from univer_ocr_amd.nn.gpu import DeviceArray
    a = np.ascontiguousarray(a, dtype=np.float32)
    flat = torch.empty(a.size + 4, dtype=torch.float32, device=CP.storage_device())
    t = flat[1:1 + a.size].view(*a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.data_ptr() % 16 == 4
    return DeviceArray(t)


def test_misaligned_operands(ctx):
    """dense x, w, dy and conv w at a 4-byte offset: sizes that are otherwise multiples of 4 take load_slow."""
    from univer_ocr_amd.nn import ops
    CP = ctx
    rng = np.random.default_rng(1000)
    m, n_in, n_out = 100, 96, 64
    X, w, g = dense_problem(rng, m, n_in, n_out)
    ref_y = O.dense_fwd(X, w)
    ref_dx, ref_dw = O.dense_bwd(X, w, g)
    Xd, wd, gd = misaligned(CP, X), misaligned(CP, w), misaligned(CP, g)
    sweep(CP, lambda: (ops.dense_fwd(Xd, wd),), (m, n_out, n_in + 1, True), [(ref_y, TOL_Y, 'y')], 'misaligned fwd')

    def dx():
        out = CP.empty((m, n_in))
        dense_call(CP, Xd, wd, gd, out, None, False)
        return (out,)

    sweep(CP, dx, (m, n_in, n_out, True), [(ref_dx, TOL_Y, 'dx')], 'misaligned dense dx')

    def dw():
        out = CP.full(w.shape, 0.5)
        dense_call(CP, Xd, wd, gd, None, out, True)
        return (out,)

    sweep(CP, dw, (n_in + 1, n_out, m, True), [(ref_dw + 0.5, TOL_W, 'dw')], 'misaligned dense dw')

    xs, ks, cout, st, pd = (2, 9, 11, 32), (3, 3), 64, (1, 1), (1, 1)
    Xc = rng.standard_normal(xs)
    wc = rng.standard_normal((*ks, xs[3], cout)) * 0.1
    bc = rng.standard_normal(cout)
    ref_yc = O.conv2d_fwd(Xc, wc, bc, st, pd, 0.0, True)
    gc = rng.standard_normal(ref_yc.shape)
    ref_dxc, _, _ = O.conv2d_bwd(Xc, wc, gc, st, pd, 0.0, True)
    Xcd, wcd, bcd, gcd = CP.copy(Xc), misaligned(CP, wc), CP.copy(bc), CP.copy(gc)
    fwd, dgrad, _ = conv_gemms(xs, ks, cout, st, pd)
    sweep(CP, lambda: (ops.conv2d_fwd(Xcd, wcd, bcd, st, pd, 0.0, True),), fwd, [(ref_yc, TOL_Y, 'y')],
          'misaligned conv fwd')
    sweep(CP, lambda: (ops.conv2d_bwd_data(gcd, wcd, xs, st, pd),), dgrad, [(ref_dxc, TOL_Y, 'dx')],
          'misaligned conv dx')


# ---- a context with a 1 MB workspace -----------------------------------------------------------------------------------
@contextlib.contextmanager
def small_workspace(CP, mb=1):
    """The runtime's calls go to a context of its own with an `mb` MB workspace, on the current stream."""
    import torch
    rt = CP.runtime()
    handle = C.c_void_p()
    assert rt.lib.uocr_ctx_create(rt.device_index, mb << 20, C.byref(handle)) == 0
    from univer_ocr_amd.nn.gpu import Lane
    try:
        with rt.on(Lane(torch.cuda.current_stream(), handle)):
            rt.call('uocr_ctx_set_stream', C.c_void_p(torch.cuda.current_stream().cuda_stream))
            for key, value in (('mfma', 2), ('fast_paths', 0)) + GEMM_DEFAULTS:
                rt.call('uocr_ctx_set_option', key.encode(), value)
            yield (mb << 20) // 2
            rt.call('uocr_stream_sync')
    finally:
        rt.lib.uocr_ctx_destroy(handle)


def test_small_workspace(ctx):
    """The slab count is clamped to what fits in half the workspace; a conv dx whose weights do not fit leaves the MFMA
    path; the deferred group launches a problem whose slabs could not fit at once instead of recording it."""
    from univer_ocr_amd.nn import ops
    CP = ctx
    rt = CP.runtime()
    rng = np.random.default_rng(1100)
    cu = cu_count(CP)
    xs, ks, cout, st, pd = (2, 16, 40, 16), (3, 3), 64, (1, 1), (1, 1)
    X = rng.standard_normal(xs)
    g = rng.standard_normal((*xs[:3], cout))
    _, ref_dw, ref_db = O.conv2d_bwd(X, np.zeros((*ks, 16, cout)), g, st, pd, 0.0, True)
    Xd, gd = CP.copy(X), CP.copy(g)
    xs2, cout2 = (1, 6, 8, 128), 128                            # dx weights: 3*3*128*128*4 bytes > 512 KB
    w2 = rng.standard_normal((3, 3, 128, cout2)) * 0.05
    g2 = rng.standard_normal((*xs2[:3], cout2))
    ref_dx2, _, _ = O.conv2d_bwd(rng.standard_normal(xs2), w2, g2, st, pd, 0.0, True)
    g2d, w2d = CP.copy(g2), CP.copy(w2)
    m, n_in, n_out = 64, 400, 200                               # dense dw: 401 x 200 floats, twice > 512 KB
    Xb, wb, gb = dense_problem(rng, m, n_in, n_out)
    _, ref_dwb = O.dense_bwd(Xb, wb, gb)
    Xbd, wbd, gbd = CP.copy(Xb), CP.copy(wb), CP.copy(gb)
    with small_workspace(CP) as ws_half:
        opt = dict(gemm_bm=64, split_blocks=1 << 24, split_min=2, xcd_remap=1, group_blocks=0)
        set_gemm_options_ctx(rt, opt)
        dw, db = CP.full((*ks, 16, cout), 0.5), CP.full((cout,), 0.25)
        ops.conv2d_bwd_weight(Xd, gd, dw, db, st, pd, 0.0, True, accumulate=True)
        got = rt.last_gemm()
        M, N, depth = 145, cout, 2 * 16 * 40
        assert got == expect_gemm(M, N, depth, True, cu, ws_half, opt), got
        assert got[3] == ws_half // (M * N * 4) < expect_gemm(M, N, depth, True, cu, WS_HALF, opt)[3], got
        check(dw, ref_dw + 0.5, TOL_W, 'dw (clamped split)')
        check(db, ref_db + 0.25, TOL_W, 'db (clamped split)')
        before = rt.last_gemm()
        dx = ops.conv2d_bwd_data(g2d, w2d, xs2, st, pd)
        assert rt.last_gemm() == before, 'a conv dx whose weights exceed half the workspace ran on the MFMA GEMM'
        check(dx, ref_dx2, TOL_Y, 'dx (off the MFMA path)')
        dw, db = CP.full((*ks, 16, cout), 0.5), CP.full((cout,), 0.25)
        dwb = CP.full(wb.shape, 0.5)
        with rt.defer_wgrad():
            ops.conv2d_bwd_weight(Xd, gd, dw, db, st, pd, 0.0, True, accumulate=True)     # recorded
            assert rt.last_gemm() == before
            ops.dense_bwd(Xbd, wbd, gbd, dwb, accumulate=True, need_dx=False)            # refused: launched now
            assert rt.last_gemm()[1:3] == (cdiv(n_in + 1, 64), cdiv(n_out, 64)), rt.last_gemm()
        assert rt.last_gemm()[:3] == (64, 0, 0) and rt.last_gemm_group()[0] == 1
        check(dw, ref_dw + 0.5, TOL_W, 'dw (group)')
        check(db, ref_db + 0.25, TOL_W, 'db (group)')
        check(dwb, ref_dwb + 0.5, TOL_W, 'dense dw (refused by the group)')
        set_gemm_options_ctx(rt, dict(GEMM_DEFAULTS))


def set_gemm_options_ctx(rt, opt):
    """options of the CURRENT ctx only (Runtime.set_option sets them on the runtime's own lanes)"""
    for key, value in opt.items():
        rt.call('uocr_ctx_set_option', key.encode(), int(value))


# ---- the deferred weight-gradient group ------------------------------------------------------------------------------
GROUP_CONVS = [
    ((2, 9, 20, 32), (3, 3), 48, (1, 1), (1, 1)),
    ((2, 14, 64, 16), (5, 3), 64, (2, 1), (0, 1)),
    ((3, 7, 9, 12), (3, 2), 36, (1, 1), (1, 0)),
    ((2, 4, 40, 16), (3, 3), 24, (1, 1), (1, 1)),
    ((1, 5, 33, 8), (3, 3), 20, (1, 1), (1, 1)),
    ((2, 6, 20, 32), (3, 3), 72, (1, 1), (1, 1)),
]
GROUP_DENSE = [(300, 200, 162), (100, 96, 64), (256, 128, 162), (37, 64, 64)]


def group_jobs(CP, rng, nconv, ndense):
    jobs = []
    for xs, ks, cout, st, pd in GROUP_CONVS[:nconv]:
        X = rng.standard_normal(xs)
        oh, ow = O.conv2d_out_hw(xs[1], xs[2], ks, st, pd)
        g = rng.standard_normal((xs[0], oh, ow, cout))
        _, ref_dw, ref_db = O.conv2d_bwd(X, np.zeros((*ks, xs[3], cout)), g, st, pd, 0.0, True)
        gemm = (ks[0] * ks[1] * xs[3] + 1, cout, xs[0] * oh * ow)
        jobs.append(('conv', (CP.copy(X), CP.copy(g), (*ks, xs[3], cout), st, pd), (ref_dw, ref_db), gemm))
    for m, n_in, n_out in GROUP_DENSE[:ndense]:
        X, w, g = dense_problem(rng, m, n_in, n_out)
        jobs.append(('dense', (CP.copy(X), CP.copy(w), CP.copy(g)), (O.dense_bwd(X, w, g)[1],), (n_in + 1, n_out, m)))
    return jobs


def run_job(CP, job):
    from univer_ocr_amd.nn import ops
    kind, args, refs, _ = job
    if kind == 'conv':
        Xd, gd, wshape, st, pd = args
        dw, db = CP.full(wshape, 0.5), CP.full((wshape[3],), 0.25)
        ops.conv2d_bwd_weight(Xd, gd, dw, db, st, pd, 0.0, True, accumulate=True)
        return dw, db
    Xd, wd, gd = args
    dw = CP.full(wd.shape, 0.5)
    ops.dense_bwd(Xd, wd, gd, dw, accumulate=True, need_dx=False)
    return (dw,)


def check_job(job, outs, what):
    for out, ref, name in zip(outs, job[2], ('dw', 'db')):
        check(out, ref + (0.5 if name == 'dw' else 0.25), TOL_W, f'{what} {job[0]} {job[3]} {name}')


def test_group_blocks_configs(ctx):
    """3 conv dw + 2 dense dw recorded and run as one group, with group_blocks = 1 (nothing split), a value that splits
    some problems and leaves the others unsplit, the default (four blocks per CU), and split_blocks = 0."""
    CP = ctx
    rt = CP.runtime()
    cu = cu_count(CP)
    jobs = group_jobs(CP, np.random.default_rng(1200), 3, 2)
    problems = [j[3] for j in jobs]
    mixed = next(v for v in range(2, 4096)
                 if len({s > 1 for s in expect_group(problems, cu, WS_HALF, v, 1024, 3)}) == 2)
    try:
        for group_blocks, split in ((1, 1024), (mixed, 1024), (0, 1024), (0, 0)):
            set_gemm_options(rt, dict(group_blocks=group_blocks, split_blocks=split))
            splits = expect_group(problems, cu, WS_HALF, group_blocks, split, 3)
            with rt.defer_wgrad():
                outs = [run_job(CP, job) for job in jobs]
            assert rt.last_gemm() == (64, 0, 0, max(splits)), (group_blocks, split, rt.last_gemm(), splits)
            assert rt.last_gemm_group() == (len(jobs), sum(s > 1 for s in splits)), (group_blocks, splits)
            if group_blocks == mixed:
                assert 0 < rt.last_gemm_group()[1] < len(jobs)
            for job, out in zip(jobs, outs):
                check_job(job, out, f'group_blocks={group_blocks} split_blocks={split}')
    finally:
        set_gemm_options(rt, dict(GEMM_DEFAULTS))


def test_group_overflow(ctx):
    """10 calls, 6 of them conv dw: the 5th conv finds 4 conv problems recorded and the 10th call 8 problems -- both
    are launched at once, outside the group.  Every result matches the oracle and the separate launches."""
    CP = ctx
    rt = CP.runtime()
    jobs = group_jobs(CP, np.random.default_rng(1300), 6, 4)
    from univer_ocr_amd.nn import ops
    order = [0, 1, 2, 3, 4, 6, 7, 8, 9, 5]                      # conv 1-5, dense 1-4, conv 6
    separate = [[host(o) for o in run_job(CP, job)] for job in jobs]
    outs = [None] * len(jobs)
    cu = cu_count(CP)
    ops.dense_fwd(CP.zeros((1000, 64)), CP.zeros((65, 300)))    # a GEMM none of the calls below matches
    expected = rt.last_gemm()
    assert expected[1:3] == (16, 5), expected
    with rt.defer_wgrad():
        for k, i in enumerate(order):
            outs[i] = run_job(CP, jobs[i])
            if k in (4, 9):
                expected = expect_gemm(*jobs[i][3], True, cu, WS_HALF, dict(GEMM_DEFAULTS))
            assert rt.last_gemm() == expected, f'call {k + 1}: last_gemm {rt.last_gemm()}, expected {expected}'
    assert rt.last_gemm()[:3] == (64, 0, 0) and rt.last_gemm_group()[0] == 8, rt.last_gemm_group()
    for job, out, sep in zip(jobs, outs, separate):
        check_job(job, out, 'overflowing group')
        for o, s in zip(out, sep):
            check(o, s, TOL_W, f'group vs separate launch {job[3]}')


@pytest.mark.parametrize('kind', ['conv', 'dense'])
def test_group_calls_accumulating_into_one_gradient(kind, ctx):
    """Two recorded calls that accumulate into the SAME dw / db (a layer applied twice) give what the two calls give one
    after the other: the second call flushes the first before it is recorded."""
    from univer_ocr_amd.nn import ops
    CP = ctx
    rt = CP.runtime()
    rng = np.random.default_rng(1400)
    if kind == 'conv':
        xs, ks, cout, st, pd = GROUP_CONVS[0]
        a = [(rng.standard_normal(xs), rng.standard_normal((xs[0], xs[1], xs[2], cout))) for _ in range(2)]
        refs = [O.conv2d_bwd(X, np.zeros((*ks, xs[3], cout)), g, st, pd, 0.0, True)[1:] for X, g in a]
        dev = [(CP.copy(X), CP.copy(g)) for X, g in a]

        def call(i, dw, db):
            ops.conv2d_bwd_weight(*dev[i], dw, db, st, pd, 0.0, True, accumulate=True)

        shapes = [(*ks, xs[3], cout), (cout,)]
    else:
        m, n_in, n_out = GROUP_DENSE[1]
        a = [dense_problem(rng, m, n_in, n_out) for _ in range(2)]
        refs = [(O.dense_bwd(X, w, g)[1],) for X, w, g in a]
        dev = [tuple(CP.copy(v) for v in p) for p in a]

        def call(i, dw):
            ops.dense_bwd(*dev[i], dw, accumulate=True, need_dx=False)

        shapes = [(n_in + 1, n_out)]
    seq = [CP.full(s, 0.5) for s in shapes]
    call(0, *seq)
    call(1, *seq)
    apart = [[CP.full(s, 0.5) for s in shapes] for _ in range(2)]
    with rt.defer_wgrad():                                       # the same two calls into two gradients: one group
        call(0, *apart[0])
        call(1, *apart[1])
    assert rt.last_gemm_group()[0] == 2, rt.last_gemm_group()
    for bufs, r in zip(apart, refs):
        for o, rr, name in zip(bufs, r, ('dw', 'db')):
            check(o, rr + 0.5, TOL_W, f'{kind} {name}, two gradients in one group')
    out = [CP.full(s, 0.5) for s in shapes]
    with rt.defer_wgrad():
        call(0, *out)
        call(1, *out)
        flushed = rt.last_gemm_group()[0]
    for o, s, r0, r1, name in zip(out, seq, *refs, ('dw', 'db')):
        check(s, r0 + r1 + 0.5, TOL_W, f'{kind} {name}, one call after the other')
        check(o, r0 + r1 + 0.5, TOL_W, f'{kind} {name}, two recorded calls')
        check(o, host(s), TOL_W, f'{kind} {name}, recorded vs one after the other')
    assert flushed == 1, 'the second call did not flush the first'
    assert rt.last_gemm_group()[0] == 1
