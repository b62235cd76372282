"""Upsample2D(2) + 5x5 conv, 4 -> 4 channels, float32 (csrc/conv_up.hip): the kernels keep loads in flight across their
tile and trip boundaries -- the weights and the first tile in one batch in front of the forward, the next xl tile and the
dy values of the next depth trip (across the tile boundary: of the next tile's first trip) in registers in the weight
gradient, the activation outputs of the masked backward-data before its tap loop.

Shapes (n, hl, wl) against the 16 x 32 tile: less than one tile; exactly one tile per image; one full tile plus a
one-row and a one-column tile; four row tiles with a ragged last one in three strips with a ragged last one, so that a
block that walks a band takes the first, a middle and the last step of every prefetch, and bands carry across strips
and images.  The context option "max_blocks" (auto, 1, 2, 3, 7, items - 1) makes the bands longer than one tile.

Against the float64 oracle composition (upsample2d + conv2d): y and dx at 1e-5, dw / db at 2e-5 (rel_linf), with random
asymmetric weights, bias on and off; y and dx are bit-identical for every cap, and dx does not depend on whether the
per-phase weights come from the forward call or from the backward call's own kernel.  Every output buffer starts as NaN.
"""
import functools

import numpy as np
import pytest

from conftest import rel_linf
from oracle import nn_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-5             # y, dx
TOL_W = 2e-5           # dw, db
CAPS = (1, 2, 3, 7)
SHAPES = [(1, 7, 9), (3, 16, 32), (2, 33, 33), (2, 53, 70)]
DEFAULTS = (('max_blocks', 0), ('t32', 2), ('h16', 1), ('mfma', 1), ('fast_paths', 1), ('tiled', 1))


def _restore(CP):
    for key, value in DEFAULTS:
        CP.runtime().set_option(key, value)
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


def cdiv(a, b):
    return (a + b - 1) // b


def rows_split(n, hl, wl, budget):
    """conv_up.hip, up_rows_per_block: (blocks, items) of a launch under a block budget"""
    strips, rows = cdiv(wl, 32), 16
    while rows < hl and strips * cdiv(hl, rows) * n > budget:
        rows += 16
    return strips * cdiv(hl, rows) * n, strips * cdiv(hl, 16) * n


@functools.lru_cache(maxsize=None)
def reference(case):
    """Inputs and float64 oracle results of one shape, computed once and read-only: the keys with a bias flag are
    (name, bias)."""
    n, hl, wl = SHAPES[case]
    rng = np.random.default_rng(8100 + case)
    r = {'xl': rng.standard_normal((n, hl, wl, 4)), 'w': rng.standard_normal((5, 5, 4, 4)) * 0.2,
         'b': rng.standard_normal(4)}
    up = O.upsample2d_fwd(r['xl'], (2, 2))
    r['g'] = rng.standard_normal((n, 2 * hl, 2 * wl, 4))
    r['mask'] = np.where(rng.random(r['xl'].shape) < 0.5, -1.0, 1.0) * np.abs(r['xl'])
    r['slope'] = np.where(r['mask'] >= 0, 1.0, 0.01)
    for bias in (False, True):
        r['y', bias] = O.conv2d_fwd(up, r['w'], r['b'], 1, 2, 0.0, bias)
        dx_hi, r['dw', bias], r['db', bias] = O.conv2d_bwd(up, r['w'], r['g'], 1, 2, 0.0, bias)
        r['dx', bias] = O.upsample2d_bwd(dx_hi, (2, 2))
    for a in r.values():
        a.setflags(write=False)
    return r


def sweep(CP, run, split):
    """run() for auto and for every cap: [(cap, host result)]; `split`: budget -> (blocks, items) the launch must report,
    or None for a launch that does not depend on the cap"""
    rt = CP.runtime()
    out = []
    items = split(1 << 30)[1] if split else 0
    for k in (0,) + tuple(sorted({c for c in CAPS + (items - 1,) if c > 0})):
        rt.set_option('max_blocks', k)
        try:
            got = run()
            if split:
                assert tuple(rt.last_split()) == split(k if k else 1 << 30), (k, rt.last_split())
        finally:
            rt.set_option('max_blocks', 0)
        out.append((k, tuple(CP.asnumpy(a) for a in got) if isinstance(got, tuple) else CP.asnumpy(got)))
    return out


def check(a, ref, tol, what):
    err = rel_linf(a, ref)
    print(f'{what}: rel_linf={err:.3e}')
    assert err <= tol, f'{what}: rel_linf={err:.3e} > {tol:.1e}'


def same_bits(results, what):
    ref = results[0][1]
    for k, got in results[1:]:
        assert np.array_equal(got, ref), f'{what}: max_blocks={k} differs from the auto split ' \
            f'(max |diff| {np.nanmax(np.abs(got.astype(np.float64) - ref)):.3e}, NaN {int(np.isnan(got).sum())})'


@pytest.mark.parametrize('bias', [True, False], ids=['bias', 'nobias'])
@pytest.mark.parametrize('case', range(len(SHAPES)), ids=['x'.join(map(str, s)) for s in SHAPES])
def test_forward_and_backward_data(case, bias, ctx):
    from univer_ocr_amd.nn import ops
    CP = ctx
    n, hl, wl = SHAPES[case]
    r = reference(case)
    xd, gd, md = CP.copy(r['xl']), CP.copy(r['g']), CP.copy(r['mask'])
    wd, bd = CP.copy(r['w'], np.float32), CP.copy(r['b'], np.float32)
    fwd = lambda budget: rows_split(n, hl, wl, min(2048, budget))

    ys = sweep(CP, lambda: ops.upconv2x_fwd(xd, wd, bd, (2, 2), bias), fwd)
    check(ys[0][1], r['y', bias], TOL, 'y')
    same_bits(ys, 'y')
    ya = sweep(CP, lambda: ops.upconv2x_fwd(xd, wd, bd, (2, 2), bias, act='leaky', alpha=0.01), fwd)
    check(ya[0][1], O.leaky_relu_fwd(r['y', bias], 0.01), TOL, 'leaky(y)')
    same_bits(ya, 'leaky(y)')

    dxs = sweep(CP, lambda: ops.upconv2x_bwd_data(gd, wd, r['xl'].shape, (2, 2)), None)
    check(dxs[0][1], r['dx', bias], TOL, 'dx')
    same_bits(dxs, 'dx')
    dxm = sweep(CP, lambda: ops.upconv2x_bwd_data(gd, wd, r['xl'].shape, (2, 2), x_act=md, act='leaky', alpha=0.01),
                None)
    check(dxm[0][1], r['dx', bias] * r['slope'], TOL, 'masked dx')
    same_bits(dxm, 'masked dx')

    # the per-phase weights written by the forward call (any band length) and handed to the backward call
    for k in (0, 1):
        weff = CP.empty((576,), np.float32)
        CP.runtime().set_option('max_blocks', k)
        try:
            y = ops.upconv2x_fwd(xd, wd, bd, (2, 2), bias, weff=weff)
        finally:
            CP.runtime().set_option('max_blocks', 0)
        assert np.array_equal(CP.asnumpy(y), ys[0][1]), f'y with weff written, max_blocks={k}'
        dx = ops.upconv2x_bwd_data(gd, wd, r['xl'].shape, (2, 2), weff=weff)
        assert np.array_equal(CP.asnumpy(dx), dxs[0][1]), f'dx with the forward\'s weff, max_blocks={k}'
        dx = ops.upconv2x_bwd_data(gd, wd, r['xl'].shape, (2, 2), x_act=md, act='leaky', alpha=0.01, weff=weff)
        assert np.array_equal(CP.asnumpy(dx), dxm[0][1]), f'masked dx with the forward\'s weff, max_blocks={k}'


@pytest.mark.parametrize('bias', [True, False], ids=['bias', 'nobias'])
@pytest.mark.parametrize('case', range(len(SHAPES)), ids=['x'.join(map(str, s)) for s in SHAPES])
def test_weight_gradient(case, bias, ctx):
    from univer_ocr_amd.nn import ops
    CP = ctx
    n, hl, wl = SHAPES[case]
    r = reference(case)
    xd, gd = CP.copy(r['xl']), CP.copy(r['g'])
    split = lambda budget: rows_split(n, hl, wl, min(1024, budget))

    def accumulate():
        dw, db = CP.full((5, 5, 4, 4), 0.5, np.float32), CP.full((4,), 0.25, np.float32)
        ops.upconv2x_bwd_weight(xd, gd, dw, db, (2, 2), bias, accumulate=True)
        return dw, db

    def overwrite():
        dw, db = CP.empty((5, 5, 4, 4), np.float32), CP.empty((4,), np.float32)       # (NaN: the fixture)
        ops.upconv2x_bwd_weight(xd, gd, dw, db, (2, 2), bias, accumulate=False)
        return dw, db

    for form, run, add_w, add_b in (('accumulate', accumulate, 0.5, 0.25), ('overwrite', overwrite, 0.0, 0.0)):
        for k, (dw, db) in sweep(CP, run, split):
            check(dw, r['dw', bias] + add_w, TOL_W, f'{form} dw, max_blocks={k}')
            check(db, r['db', bias] + add_b, TOL_W, f'{form} db, max_blocks={k}')
