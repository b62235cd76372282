"""Work splits decided at run time: persistent tile walks (a block starts at tile blockIdx.x and steps by gridDim.x,
TileWalk in uocr_common.h), tiles or rows per block under a fixed block budget, row bands of the direct weight-gradient
and conv-pair kernels.

On an MI355X a persistent grid holds at least 256 blocks and the budgets are 1024 / 2048 blocks, so at the shapes of
the other parity tests every block handles exactly one tile.  Here the context option "max_blocks" lowers every
run-time budget (auto, 1, 2, 3, 7 and items - 1 blocks), so that blocks walk several tiles -- across a column strip,
a tile row and an image -- and `Runtime.last_split` (uocr_ctx_last_split) confirms the split each launch made.

What each cap must give:
  * forward / backward-data (plain, fused activation, masked dx): every output pixel is computed by one tile, so the
    result is BIT-IDENTICAL to the auto run; the auto run against the float64 oracle (float32 1e-5, binary16 1e-3);
  * dw / db: against the oracle at 2e-5 for every cap -- accumulating into 0.5 / 0.25, overwriting, with a binary16
    gradient scale, and inside a deferred weight-gradient group (the deferred finish sums the few partial rows).
Every output buffer the ops allocate starts as NaN here, so a tile that no block writes cannot pass.
"""
import numpy as np
import pytest

from conftest import rel_linf
from oracle import nn_oracle as O

pytestmark = pytest.mark.gpu

TOL_STORE = 1e-3       # a tensor stored in binary16 by one kernel (test_gpu_f16.py)
TOL_EXACT = 2e-5       # dw / db
CAPS = (1, 2, 3, 7)
DEFAULTS = (('max_blocks', 0), ('wgrad_bands', 0), ('pair_band', 0), ('t32', 2), ('h16', 1), ('mfma', 1),
            ('fast_paths', 1), ('tiled', 1))


def _restore(CP):
    rt = CP.runtime()
    for key, value in DEFAULTS:
        rt.set_option(key, value)
    CP.set_dtype('float32')
    CP.f16_grad_scale_log2 = None


@pytest.fixture
def ctx(monkeypatch):
    """The shared context with the defaults restored on both sides; every array the ops allocate is filled with NaN."""
    from univer_ocr_amd.nn import CP
    from univer_ocr_amd.nn import gpu
    CP.use_gpu(0)
    _restore(CP)
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


def force_t32(CP, bits):
    """conv_t32 / conv_t32w forms other than the default (bit 2) exist only in a UOCR_BUILD_EXPERIMENTS library."""
    from univer_ocr_amd.hip.lib import HipError
    try:
        CP.runtime().set_option('t32', bits)
    except HipError as e:
        if 'built without' not in str(e):
            raise
        pytest.skip('library built without UOCR_BUILD_EXPERIMENTS')


def r16(a):
    return np.asarray(a, dtype=np.float64).astype(np.float16).astype(np.float64)


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def host(a):
    from univer_ocr_amd.nn import CP
    return CP.asnumpy(a)


def cdiv(a, b):
    return (a + b - 1) // b


# ---- expected splits of the budget loops (Python copies of the host code) ----------------------------------------------
def per_block_split(tiles_x, tiles_y, n, budget):
    """conv_fast.hip, conv_wgrad_t542 / conv_wgrad_s2_tiled: tiles per block down a column strip."""
    per = 1
    while per < tiles_y and tiles_x * cdiv(tiles_y, per) * n > budget:
        per += 1
    return tiles_x * cdiv(tiles_y, per) * n, tiles_x * tiles_y * n


def up_rows_split(hl, wl, n, budget):
    """conv_up.hip, up_rows_per_block: rows of 16 per band step, strips of 32 columns."""
    strips, rows = cdiv(wl, 32), 16
    while rows < hl and strips * cdiv(hl, rows) * n > budget:
        rows += 16
    return strips * cdiv(hl, rows) * n, strips * cdiv(hl, 16) * n


def c16_split(h, n, budget):
    """conv_fast.hip, conv_c16_wgrad: row bands (multiples of 4 rows) under a block budget."""
    rows = cdiv(n * h, budget)
    rows = cdiv(rows, 4) * 4
    if rows > h:
        rows = cdiv(h, 4) * 4
    return cdiv(h, rows) * n, cdiv(h, 4) * n


def sweep(CP, run, split):
    """run() once per cap (auto first); returns [(cap, result)].  `split`: None (the op has no run-time split: only
    auto), 'walk' (persistent grid: blocks == min(cap, items)) or a function budget -> (blocks, items)."""
    rt = CP.runtime()
    rt.set_option('max_blocks', 0)
    out = [(0, run())]
    if split is None:
        return out
    blocks0, items = rt.last_split()
    if split == 'walk':
        assert blocks0 == items, (blocks0, items)            # (auto: one tile per block at these shapes)
    else:
        assert (blocks0, items) == split(1 << 30)
    assert items >= 12, items                                # (at least 3 x 2 tiles or bands in each of 2 images)
    for k in sorted({c for c in CAPS + (items - 1,) if 0 < c < items}):
        rt.set_option('max_blocks', k)
        try:
            got = run()
            blocks, its = rt.last_split()
        finally:
            rt.set_option('max_blocks', 0)
        assert its == items, (k, its, items)
        if split == 'walk':
            assert blocks == k, (k, blocks)
        else:
            assert (blocks, its) == split(k), (k, blocks, its)
        out.append((k, got))
    # non-vacuous: with one block, the block walks every tile (each strip -> row -> image carry at least once)
    rt.set_option('max_blocks', 1)
    try:
        run()
        assert rt.last_split()[0] < items
    finally:
        rt.set_option('max_blocks', 0)
    return out


def same_bits(results, what):
    """every cap's result equals the auto run's bit for bit"""
    ref = host(results[0][1])
    for k, r in results[1:]:
        got = host(r)
        assert np.array_equal(got, ref), f'{what}: max_blocks={k} differs from the auto split ' \
            f'(max |diff| {np.nanmax(np.abs(got.astype(np.float64) - ref)):.3e}, NaN {int(np.isnan(got).sum())})'


def check(a, ref, tol, what):
    err = rel_linf(host(a), ref)
    assert err <= tol, f'{what}: rel_linf={err:.3e} > {tol:.1e}'


def wgrad_checks(CP, run_wgrad, wshape, cout, ref_dw, ref_db, split, tol=TOL_EXACT):
    """dw / db for every cap: accumulating into 0.5 / 0.25, overwriting, and inside a deferred group."""
    rt = CP.runtime()

    def acc():
        dw, db = CP.full(wshape, 0.5, np.float32), CP.full((cout,), 0.25, np.float32)
        run_wgrad(dw, db, True)
        return dw, db

    def over():
        dw, db = CP.full(wshape, 7.0, np.float32), CP.full((cout,), -3.0, np.float32)
        run_wgrad(dw, db, False)
        return dw, db

    def deferred():
        dw, db = CP.full(wshape, 0.5, np.float32), CP.full((cout,), 0.25, np.float32)
        with rt.defer_wgrad():
            run_wgrad(dw, db, True)
        return dw, db

    for form, run, add_w, add_b in (('accumulate', acc, 0.5, 0.25), ('overwrite', over, 0.0, 0.0),
                                     ('deferred', deferred, 0.5, 0.25)):
        for k, (dw, db) in sweep(CP, run, split):
            check(dw, ref_dw + add_w, tol, f'{form} dw, max_blocks={k}')
            check(db, ref_db + add_b, tol, f'{form} db, max_blocks={k}')


# ---- convolutions ------------------------------------------------------------------------------------------------------
# (dtype, x shape, cout, stride, pad_value, bias, options, splits of (forward, backward-data, weight gradient)):
# 'walk' = persistent TileWalk grid; ('t542' / 's2t' / 'c16') = budget loops; None = no run-time split.
# Tiles: 64 columns for every walker, so widths 150 (stride 1) / 270 (stride 2) make 3 column strips; 70 rows make
# 3 - 9 tile rows; two images.
PB = {'t542': (64, 16, 1), 's2t': (32, 8, 2)}       # tile columns, tile rows, stride of the output grid
CONVS = [
    # float32: conv_t32.hip backward-data (on by default) + conv_wgrad_t542 / conv_wgrad_s2_tiled / conv_c16_wgrad
    ('float32', (2, 70, 150, 4), 2, 1, 0.0, True, {}, (None, 'walk', 't542')),
    ('float32', (2, 67, 150, 4), 4, 1, 0.5, False, {}, (None, 'walk', None)),
    ('float32', (2, 70, 270, 1), 4, 2, 0.25, True, {}, (None, None, 's2t')),
    ('float32', (2, 37, 83, 16), 1, 1, 0.0, True, {}, (None, None, 'c16')),
    # float32 experiments: conv_t32.hip forward / 1-channel forms, conv_t32w.hip weight gradients
    ('float32', (2, 70, 150, 4), 2, 1, 0.75, True, {'t32': 255}, ('walk', 'walk', 'walk')),
    ('float32', (2, 67, 150, 1), 1, 1, 0.0, False, {'t32': 255}, ('walk', 'walk', 'walk')),
    ('float32', (2, 70, 270, 4), 4, 2, 0.5, True, {'t32': 255}, (None, None, 'walk')),
    ('float32', (2, 67, 270, 1), 4, 2, 0.0, True, {'t32': 255}, (None, None, 'walk')),
    ('float32', (2, 70, 270, 1), 1, 2, 0.0, False, {'t32': 255}, (None, None, 'walk')),
    # binary16 MFMA kernels: conv_h16.hip (every Geo of conv2d) + conv_h16w.hip (e42, e11, s2<4,4>, s2<1,4>, s2<1,1>)
    ('float16', (2, 70, 150, 4), 2, 1, 0.0, True, {}, ('walk', 'walk', 'walk')),
    ('float16', (2, 67, 150, 4), 4, 1, 0.5, False, {}, ('walk', 'walk', None)),
    ('float16', (2, 70, 150, 1), 1, 1, 0.25, True, {}, ('walk', None, 'walk')),
    ('float16', (2, 70, 270, 4), 4, 2, 0.5, True, {}, ('walk', 'walk', 'walk')),
    ('float16', (2, 67, 270, 1), 4, 2, 0.0, False, {}, (None, 'walk', 'walk')),
    ('float16', (2, 70, 270, 1), 1, 2, 0.25, True, {}, (None, None, 'walk')),
    # binary16 storage on the vector kernels: conv_wgrad_t542 / conv_wgrad_s2_tiled
    ('float16', (2, 70, 150, 4), 2, 1, 0.5, False, {'h16': 0}, (None, None, 't542')),
    ('float16', (2, 70, 270, 1), 4, 2, 0.0, True, {'h16': 0}, (None, None, 's2t')),
]


def _split_fn(kind, xs, cout, s):
    if kind in (None, 'walk'):
        return kind
    n, h, w, _ = xs
    oh, ow = (h + s - 1) // s, (w + s - 1) // s
    if kind == 'c16':
        return lambda budget: c16_split(h, n, min(2048, budget))
    tw, th, _ = PB[kind]
    return lambda budget: per_block_split(cdiv(ow, tw), cdiv(oh, th), n, min(1024, budget))


@pytest.mark.parametrize('case', range(len(CONVS)))
def test_conv_results_do_not_depend_on_the_split(case, ctx):
    from univer_ocr_amd.nn import ops
    CP = ctx
    dtype, xs, cout, s, pv, bias, opts, splits = CONVS[case]
    if 't32' in opts:
        force_t32(CP, opts['t32'])
    for key, value in opts.items():
        if key != 't32':
            CP.runtime().set_option(key, value)
    CP.set_dtype(dtype)
    half = dtype == 'float16'
    ks = (3, 3) if xs[3] == 16 else (5, 5)
    pd = (ks[0] // 2, ks[1] // 2)
    st = (s, s)
    rng = np.random.default_rng(4000 + case)
    X = rng.standard_normal(xs)
    w = rng.standard_normal((*ks, xs[3], cout)) * 0.2
    b = rng.standard_normal(cout)
    Xq, wq, bq = (r16(X), f32(w), f32(b)) if half else (X, w, b)
    h16 = half and opts.get('h16', 1) == 1 and ks == (5, 5)
    # binary16-MFMA kernels: the float32 master weights enter the matrix cores rounded to binary16
    h16_fwd = h16 and (xs[3] == 4 or (s == 1 and cout == 1))
    h16_dx = h16 and (xs[3] == 4 or (s == 2 and cout == 4))
    ref_y = O.conv2d_fwd(Xq, r16(wq) if h16_fwd else wq, bq, st, pd, pv, bias)
    g = rng.standard_normal(ref_y.shape)
    gq = r16(g) if half else g
    ref_dx, ref_dw, ref_db = O.conv2d_bwd(Xq, r16(wq) if h16_dx else wq, gq, st, pd, pv, bias)
    mask = np.where(rng.random(xs) < 0.5, -1.0, 1.0) * np.abs(X)
    slope = np.where(mask >= 0, 1.0, 0.01)
    tol = TOL_STORE if half else 1e-5
    Xd, gd, md = CP.copy(X), CP.copy(g), CP.copy(mask)
    wd, bd = CP.copy(w, np.float32), CP.copy(b, np.float32)
    scale = 2 ** 4 if half else 1
    if half:
        gd.gscale = 4                                        # the gradient carries 2^4: dx keeps it, dw removes it
    fwd, dgrad, wgrad = (_split_fn(k, xs, cout, s) for k in splits)

    ys = sweep(CP, lambda: ops.conv2d_fwd(Xd, wd, bd, st, pd, pv, bias), fwd)
    check(ys[0][1], ref_y, tol, 'y')
    same_bits(ys, 'y')
    ya = sweep(CP, lambda: ops.conv2d_fwd(Xd, wd, bd, st, pd, pv, bias, act='leaky', alpha=0.01), fwd)
    check(ya[0][1], O.leaky_relu_fwd(ref_y, 0.01), tol, 'leaky(y)')
    same_bits(ya, 'leaky(y)')
    dxs = sweep(CP, lambda: ops.conv2d_bwd_data(gd, wd, xs, st, pd), dgrad)
    check(dxs[0][1], ref_dx, tol, 'dx')
    same_bits(dxs, 'dx')
    dxm = sweep(CP, lambda: ops.conv2d_bwd_data(gd, wd, xs, st, pd, x_act=md, act='leaky', alpha=0.01), dgrad)
    check(dxm[0][1], ref_dx * slope, tol, 'masked dx')
    same_bits(dxm, 'masked dx')

    def run_wgrad(dw, db, accumulate):
        ops.conv2d_bwd_weight(Xd, gd, dw, db, st, pd, pv, bias, accumulate=accumulate)

    wgrad_checks(CP, run_wgrad, w.shape, cout, ref_dw / scale, ref_db / scale, wgrad)


# ---- upsample(2) + conv 5x5 (conv_up.hip vector kernels: row bands; conv_h16 / conv_h16w: tile walks) -----------------
UPS = [
    # (dtype, channels, low-res shape, bias, options, splits of (forward, backward-data, weight gradient))
    ('float32', 4, (2, 40, 70), True, {}, ('rows2048', None, 'rows1024')),
    ('float32', 1, (2, 37, 70), False, {}, (None, None, 'rows1024')),
    ('float16', 4, (2, 40, 70), False, {'h16': 0}, ('rows2048', None, 'rows1024')),
    ('float16', 1, (2, 37, 70), True, {}, (None, None, 'walk')),           # wgrad_h16_up1
    ('float16', 4, (2, 36, 140), True, {}, ('walk', 'walk', 'walk')),      # conv_h16 M_UPFWD / M_UPDGRAD, wgrad_h16_up
    ('float32', 4, (2, 36, 140), False, {'t32': 255}, ('rows2048', 'walk', 'rows1024')),
    ('float32', 1, (2, 37, 150), True, {'t32': 255}, (None, 'walk', 'rows1024')),
]


@pytest.mark.parametrize('case', range(len(UPS)))
def test_upconv_results_do_not_depend_on_the_split(case, ctx):
    from univer_ocr_amd.nn import ops
    CP = ctx
    dtype, ch, (n, hl, wl), bias, opts, splits = UPS[case]
    if 't32' in opts:
        force_t32(CP, opts['t32'])
    for key, value in opts.items():
        if key != 't32':
            CP.runtime().set_option(key, value)
    CP.set_dtype(dtype)
    half = dtype == 'float16'
    rng = np.random.default_rng(5000 + case)
    xl = rng.standard_normal((n, hl, wl, ch))
    w = rng.standard_normal((5, 5, ch, ch)) * 0.2
    b = rng.standard_normal(ch)
    xq, wq, bq = (r16(xl), f32(w), f32(b)) if half else (xl, w, b)
    up = O.upsample2d_fwd(xq, (2, 2))
    ref_y = O.conv2d_fwd(up, wq, bq, 1, 2, 0.0, bias)
    g = rng.standard_normal(ref_y.shape)
    gq = r16(g) if half else g
    dx_hi, ref_dw, ref_db = O.conv2d_bwd(up, wq, gq, 1, 2, 0.0, bias)
    ref_dx = O.upsample2d_bwd(dx_hi, (2, 2))
    mask = np.where(rng.random(xl.shape) < 0.5, -1.0, 1.0) * np.abs(xl)
    slope = np.where(mask >= 0, 1.0, 0.01)
    # binary16 MFMAs with the phase-summed weights rounded to binary16 (test_gpu_f16.test_upconv2x_f16): 3e-3
    tol = (3e-3 if ch == 4 and opts.get('h16', 1) else TOL_STORE) if half else 1e-5
    xd, gd, md = CP.copy(xl), CP.copy(g), CP.copy(mask)
    wd, bd = CP.copy(w, np.float32), CP.copy(b, np.float32)
    scale = 2 ** 2 if half else 1
    if half:
        gd.gscale = 2

    def kind(k):
        if k is None or k == 'walk':
            return k
        return lambda budget: up_rows_split(hl, wl, n, min(int(k[4:]), budget))

    fwd, dgrad, wgrad = (kind(k) for k in splits)
    ys = sweep(CP, lambda: ops.upconv2x_fwd(xd, wd, bd, (2, 2), bias), fwd)
    check(ys[0][1], ref_y, tol, 'y')
    same_bits(ys, 'y')
    ya = sweep(CP, lambda: ops.upconv2x_fwd(xd, wd, bd, (2, 2), bias, act='leaky', alpha=0.01), fwd)
    check(ya[0][1], O.leaky_relu_fwd(ref_y, 0.01), tol, 'leaky(y)')
    same_bits(ya, 'leaky(y)')
    dxs = sweep(CP, lambda: ops.upconv2x_bwd_data(gd, wd, xl.shape, (2, 2)), dgrad)
    check(dxs[0][1], ref_dx, tol, 'dx')
    same_bits(dxs, 'dx')
    dxm = sweep(CP, lambda: ops.upconv2x_bwd_data(gd, wd, xl.shape, (2, 2), x_act=md, act='leaky', alpha=0.01), dgrad)
    check(dxm[0][1], ref_dx * slope, tol, 'masked dx')
    same_bits(dxm, 'masked dx')
    if callable(fwd):
        # the cap forces several row bands of 16 per block
        CP.runtime().set_option('max_blocks', 1)
        ops.upconv2x_fwd(xd, wd, bd, (2, 2), bias)
        blocks, items = CP.runtime().last_split()
        CP.runtime().set_option('max_blocks', 0)
        assert blocks < items and blocks == n * cdiv(wl, 32)

    def run_wgrad(dw, db, accumulate):
        ops.upconv2x_bwd_weight(xd, gd, dw, db, (2, 2), bias, accumulate=accumulate)

    wgrad_checks(CP, run_wgrad, w.shape, ch, ref_dw / scale, ref_db / scale, wgrad)


# ---- the existing band knobs, swept against the oracle -----------------------------------------------------------------
WGRAD_SHAPES = [
    # FastConv weight-gradient kernels (conv_fast.hip, row bands per tap / channel group): (x shape, kernel, cout, stride,
    # padding, pad_value)
    ((3, 37, 83, 1), (3, 3), 16, (1, 1), (1, 1), 0.25),
    ((3, 37, 83, 16), (3, 3), 1, (1, 1), (1, 1), 0.25),
    ((2, 41, 77, 1), (5, 5), 1, (2, 2), (2, 2), 0.0),
    ((2, 41, 77, 4), (5, 5), 4, (2, 2), (2, 2), 0.5),
    ((2, 41, 77, 4), (5, 5), 4, (1, 1), (2, 2), 0.0),
    ((2, 41, 77, 1), (5, 5), 1, (1, 1), (2, 2), 0.25),
    ((3, 32, 70, 1), (5, 3), 64, (2, 1), (0, 1), 0.0),
]


@pytest.mark.parametrize('case,dtype', [(c, dt) for c in range(len(WGRAD_SHAPES)) for dt in ('float32', 'float16')
                                        if dt == 'float32' or WGRAD_SHAPES[c][1] != (5, 3)])
def test_wgrad_bands_against_oracle(case, dtype, ctx):
    from univer_ocr_amd.hip.lib import HipError
    from univer_ocr_amd.nn import ops
    CP = ctx
    CP.set_dtype(dtype)
    CP.runtime().set_option('h16', 0)                    # (binary16: the FastConv kernels, not conv_h16w.hip)
    half = dtype == 'float16'
    xs, ks, cout, st, pd, pv = WGRAD_SHAPES[case]
    rng = np.random.default_rng(6000 + case)
    X = rng.standard_normal(xs)
    w = rng.standard_normal((*ks, xs[3], cout)) * 0.2
    ref_y = O.conv2d_fwd(X, w, np.zeros(cout), st, pd, pv, True)
    g = rng.standard_normal(ref_y.shape)
    Xq, gq = (r16(X), r16(g)) if half else (X, g)
    _, ref_dw, ref_db = O.conv2d_bwd(Xq, w, gq, st, pd, pv, True)
    Xd, gd = CP.copy(X), CP.copy(g)
    if half:
        gd.gscale = 3                                    # (dw / db come out divided by 2^3)
        ref_dw, ref_db = ref_dw / 8, ref_db / 8
    for bands in (1, 2, 3, 7, 0):
        CP.runtime().set_option('wgrad_bands', bands)
        dw, db = CP.full(w.shape, 0.5, np.float32), CP.full((cout,), 0.25, np.float32)
        ops.conv2d_bwd_weight(Xd, gd, dw, db, st, pd, pv, True, accumulate=True)
        check(dw, ref_dw + 0.5, TOL_EXACT, f'dw, wgrad_bands={bands}')
        check(db, ref_db + 0.25, TOL_EXACT, f'db, wgrad_bands={bands}')
    with pytest.raises(HipError):
        CP.runtime().set_option('wgrad_bands', -1)


@pytest.mark.parametrize('shape', [(2, 37, 83), (2, 16, 300), (3, 9, 40)])
def test_pair_band_against_oracle_f32(shape, ctx):
    """The conv-pair strip kernels (conv_pair_strip.hip) with one band for the whole height, an odd band height and the
    smallest the kernels take (band heights below 4 are raised to 4), at the tolerances of
    test_gpu_kernels.test_conv_pair_kernels_against_oracle."""
    from univer_ocr_amd.hip import lib as hiplib
    from univer_ocr_amd.nn import ops
    CP = ctx
    n, h, w_ = shape
    rng = np.random.default_rng(sum(shape) + 7)
    X = rng.standard_normal((n, h, w_, 1))
    w1, b1 = rng.standard_normal((3, 3, 1, 16)) * 0.4, rng.standard_normal(16) * 0.3
    w2, b2 = rng.standard_normal((3, 3, 16, 1)) * 0.2, rng.standard_normal(1)
    pad1, alpha = 0.25, 0.01
    z1 = O.conv2d_fwd(X, w1, b1, 1, 1, pad1, True)
    a1 = O.leaky_relu_fwd(z1, alpha)
    z2 = O.conv2d_fwd(a1, w2, b2, 1, 1, 0.0, True)
    ref_y = O.sigmoid_fwd(z2)
    g = rng.standard_normal(ref_y.shape)
    ga1, ref_dw2, ref_db2 = O.conv2d_bwd(a1, w2, O.sigmoid_bwd(z2, g), 1, 1, 0.0, True)
    ref_dx, ref_dw1, ref_db1 = O.conv2d_bwd(X, w1, O.leaky_relu_bwd(z1, ga1, alpha), 1, 1, pad1, True)
    Xd, w1d, b1d, w2d, b2d, gd = (CP.copy(a) for a in (X, w1, b1, w2, b2, g))
    for band in (0, h, 7, 1):
        CP.runtime().set_option('pair_band', band)
        y = ops.conv_pair_fwd(Xd, w1d, b1d, w2d, b2d, pad1, True, True, alpha, hiplib.ACT_SIGMOID)
        check(y, ref_y, 1e-5, f'y, pair_band={band}')
        grads = [CP.full(a.shape, 0.5) for a in (w1, b1, w2, b2)]
        dx = ops.conv_pair_bwd(Xd, y, gd, w1d, b1d, w2d, *grads, pad1, True, True, alpha, hiplib.ACT_SIGMOID,
                               need_dx=True, accumulate=True)
        check(dx, ref_dx, 2e-5, f'dx, pair_band={band}')
        for name, got, ref in zip(('dw1', 'db1', 'dw2', 'db2'), grads, (ref_dw1, ref_db1, ref_dw2, ref_db2)):
            check(got, ref + 0.5, 2e-5, f'{name}, pair_band={band}')


@pytest.mark.parametrize('shape', [(2, 45, 70), (2, 16, 300), (3, 9, 40)])
def test_pair_band_against_oracle_f16(shape, ctx):
    """The binary16 conv-pair kernels (conv_pair_strip_h.hip: one-block strips and independent waves) over the same
    band heights, against the float64 oracle with the roundings the kernels make (test_gpu_f16.test_conv_pair_f16:
    stored tensors 1e-3, parameter gradients 2e-4, db1 4e-3)."""
    from univer_ocr_amd.hip import lib as hiplib
    from univer_ocr_amd.nn import ops
    CP = ctx
    CP.set_dtype('float16')
    n, h, w_ = shape
    rng = np.random.default_rng(h + w_)
    x = rng.random((n, h, w_, 1))
    w1, b1 = rng.standard_normal((3, 3, 1, 16)) * 0.4, rng.standard_normal(16) * 0.1
    w2, b2 = rng.standard_normal((3, 3, 16, 1)) * 0.2, rng.standard_normal(1) * 0.1
    x16, g16 = r16(x), r16(rng.standard_normal((n, h, w_, 1)))
    xd, gd = CP.copy(x), CP.copy(g16)
    p = [CP.copy(a, np.float32) for a in (w1, b1, w2, b2)]
    z1 = O.conv2d_fwd(x16, r16(f32(w1)), f32(b1), 1, 1, 0.0, True)
    a1 = r16(O.leaky_relu_fwd(z1, 0.01))
    z2 = O.conv2d_fwd(a1, r16(f32(w2)), f32(b2), 1, 1, 0.0, True)
    ref_y = O.sigmoid_fwd(z2)
    for band in (0, h, 7, 1):
        CP.runtime().set_option('pair_band', band)
        y = ops.conv_pair_fwd(xd, *p, act2=hiplib.ACT_SIGMOID)
        check(y, ref_y, TOL_STORE, f'y, pair_band={band}')
        y16 = host(y).astype(np.float64)                 # the backward starts from the STORED output
        gz2 = r16(g16 * y16 * (1 - y16))
        ga1, ref_dw2, ref_db2 = O.conv2d_bwd(a1, r16(f32(w2)), gz2, 1, 1, 0.0, True)
        gz1 = r16(O.leaky_relu_bwd(z1, ga1, 0.01))
        ref_dx, ref_dw1, ref_db1 = O.conv2d_bwd(x16, r16(f32(w1)), gz1, 1, 1, 0.0, True)
        grads = [CP.zeros(a.shape, np.float32) for a in (w1, b1, w2, b2)]
        gd.gscale = 6
        dx = ops.conv_pair_bwd(xd, y, gd, p[0], p[1], p[2], *grads, act2=hiplib.ACT_SIGMOID, accumulate=False)
        check(dx, ref_dx, TOL_STORE, f'dx, pair_band={band}')
        for name, got, ref in zip(('dw1', 'db1', 'dw2', 'db2'), grads, (ref_dw1, ref_db1, ref_dw2, ref_db2)):
            check(got, ref / 64, 4e-3 if name == 'db1' else 2e-4, f'{name}, pair_band={band}')
