"""conv_t32.hip after its epilogue kinds became compile-time tags and its blocks persistent with the next tile's
loads in flight: the backward-data of the Line net's output conv (5x5, 4 -> 2, stride 1, padding 2; dx * act'(x)).

  * every mask kind of `conv2d_bwd_data`, at shapes chosen by what a tile of 16 rows x 64 columns makes of them, per
    IMAGE against the float64 oracle (float32, rel_linf <= 1e-5: the tolerance of test_gpu_work_split.py), with the
    first image 1e3 times and the last 1e-3 times the size of the others: a block that walks several tiles keeps its
    LDS tile, its weights and the next tile's loads across them, and what it left of a large image must not show in a
    small one (rel_linf over the batch would divide by the large image's maximum and hide it);
  * the same launch under `max_blocks` 1, 2, 3 and tiles - 1: bit-identical to the auto run, and `last_split` says that
    a block walked more than one tile;
  * `act_dispatch` 1 (kinds as template tags) against 0 (the instantiation with the run-time switch): bit-identical,
    for this kernel and, at one tiny shape each, for every kernel family whose launcher goes through `uocr_act_tags`
    (conv_fwd_px, conv_dgrad_s2, conv_fwd_t542, upconv_fwd_kernel, upconv_dgrad_kernel) and their untagged neighbours;
  * a pair of kinds the nets never use -- a Sigmoid mask on the 4 -> 2 layer, a ReLU on a stride-2 forward -- still
    reaches the run-time instantiation and matches the oracle (a Sigmoid there is tagged, and matches it too).

The entry point refuses a ReLU mask (conv_api.hip: a mask is LeakyReLU with alpha > 0 or Sigmoid, both expressed
through the activation's output), so the ReLU case asserts that refusal; Sigmoid is the other kind it accepts.
Outputs the ops allocate start as NaN, so a pixel no tile writes cannot pass.
"""
import functools

import numpy as np
import pytest

from conftest import rel_linf
from oracle import nn_oracle as O

pytestmark = pytest.mark.gpu

TOL = 1e-5
BR, BC = 16, 64                 # output rows / columns of a conv_t32 tile (Geo::BR, Geo::BC of the 4-channel forms)
# (n, h, w) and the role of the shape
SHAPES = [
    (1, 5, 7),                  # one partial tile
    (2, 17, 65),                # one row and one column past a tile in each direction, two images
    (1, 48, 192),               # only whole tiles; the middle one loads without bounds tests, beside eight that do not
    (3, 40, 200),               # several strips and tile rows, partial ones last, three images
]
MASKS = [None, ('leaky', 0.01), ('leaky', 0.3), ('relu', 0.0), ('sigmoid', 0.0)]
DEFAULTS = (('max_blocks', 0), ('act_dispatch', 1), ('t32', 2), ('mfma', 1), ('fast_paths', 1), ('tiled', 1))


def _restore(CP):
    for key, value in DEFAULTS:
        CP.runtime().set_option(key, value)
    CP.set_dtype('float32')


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


def host(a):
    from univer_ocr_amd.nn import CP
    return CP.asnumpy(a)


@functools.lru_cache(maxsize=None)
def problem(shape):
    """Inputs and the float64 dx of the 4 -> 2 layer at (n, h, w), computed once and shared (read-only) by every case."""
    n, h, w = shape
    rng = np.random.default_rng(7100 + 1000 * n + h + w)
    xs = (n, h, w, 4)
    wt = rng.standard_normal((5, 5, 4, 2)) * 0.2
    g = rng.standard_normal((n, h, w, 2))
    g[0] *= 1e3
    g[-1] *= 1e-3
    # the activation output the mask kinds read: both signs, and exact +0.0 / -0.0 elements
    m = rng.standard_normal(xs)
    zero = rng.random(xs)
    m[zero < 0.05] = 0.0
    m[zero > 0.95] = -0.0
    dx, _, _ = O.conv2d_bwd(np.zeros(xs), wt, g, (1, 1), (2, 2), 0.0, False)
    for a in (wt, g, m, dx):
        a.setflags(write=False)
    return xs, wt, g, m, dx


def mask_factor(kind, m):
    if kind is None:
        return np.ones_like(m), None
    name, alpha = kind
    if name == 'leaky':
        return np.where(m >= 0, 1.0, alpha), m
    y = O.sigmoid_fwd(m)                        # a Sigmoid mask is a Sigmoid OUTPUT: (0, 1) ...
    y[m == 0] = m[m == 0]                       # ... and it keeps the +0.0 / -0.0 elements (a saturated Sigmoid)
    y32 = y.astype(np.float32).astype(np.float64)
    return y32 * (1.0 - y32), y32


def per_image(got, ref, what):
    got = host(got)
    assert got.shape == ref.shape
    for i in range(ref.shape[0]):
        err = rel_linf(got[i], ref[i])
        print(f'{what}: image {i} rel_linf {err:.3e}')
        assert err <= TOL, f'{what}: image {i}: rel_linf={err:.3e} > {TOL:.1e}'


def tiles_of(shape):
    n, h, w = shape
    return n * -(-h // BR) * -(-w // BC)


@pytest.mark.parametrize('mask', range(len(MASKS)))
@pytest.mark.parametrize('shape', range(len(SHAPES)))
def test_dx_of_the_output_conv_per_image_and_under_every_cap(shape, mask, ctx):
    from univer_ocr_amd.hip.lib import CONV_KERNELS, HipError
    from univer_ocr_amd.nn import ops
    CP, rt = ctx, ctx.runtime()
    xs, wt, g, m, ref_dx = problem(SHAPES[shape])
    kind = MASKS[mask]
    gd, wd = CP.copy(g), CP.copy(wt, np.float32)
    if kind is not None and kind[0] == 'relu':
        with pytest.raises(HipError):           # (not a kind this entry point takes: see the module docstring)
            ops.conv2d_bwd_data(gd, wd, xs, (1, 1), (2, 2), x_act=CP.copy(m), act='relu', alpha=0.0)
        return
    factor, y = mask_factor(kind, m)
    md = None if y is None else CP.copy(y)

    def run():
        if kind is None:
            return ops.conv2d_bwd_data(gd, wd, xs, (1, 1), (2, 2))
        return ops.conv2d_bwd_data(gd, wd, xs, (1, 1), (2, 2), x_act=md, act=kind[0], alpha=kind[1])

    auto = run()
    assert CONV_KERNELS[rt.last_conv()[1]] == 't32'
    blocks, items = rt.last_split()
    assert items == tiles_of(SHAPES[shape]) and blocks == items, (blocks, items)
    per_image(auto, ref_dx * factor, f'{SHAPES[shape]} mask {kind}')
    ref_bits = host(auto)
    walked = False
    for k in sorted({c for c in (1, 2, 3, items - 1) if 0 < c}):
        rt.set_option('max_blocks', k)
        try:
            got = run()
            blocks, its = rt.last_split()
        finally:
            rt.set_option('max_blocks', 0)
        assert (blocks, its) == (min(k, items), items), (k, blocks, its)
        walked = walked or blocks < its
        got = host(got)
        assert np.array_equal(got, ref_bits), f'max_blocks={k} differs from the auto split (max |diff| ' \
            f'{np.nanmax(np.abs(got.astype(np.float64) - ref_bits)):.3e}, NaN {int(np.isnan(got).sum())})'
    assert walked == (items > 1)


def _both_dispatches(rt, run):
    out = []
    for value in (1, 0):
        rt.set_option('act_dispatch', value)
        try:
            out.append(host(run()))
        finally:
            rt.set_option('act_dispatch', 1)
    return out


def _experiments(rt):
    """The forward forms of conv_t32.hip exist only in a UOCR_BUILD_EXPERIMENTS library."""
    from univer_ocr_amd.hip.lib import HipError
    try:
        rt.set_option('t32', 255)
    except HipError as e:
        if 'built without' not in str(e):
            raise
        return False
    return True


def test_tags_and_run_time_switch_give_the_same_bits(ctx):
    from univer_ocr_amd.hip.lib import CONV_KERNELS
    from univer_ocr_amd.nn import ops
    CP, rt = ctx, ctx.runtime()
    xs, wt, g, m, _ = problem(SHAPES[1])
    gd, wd = CP.copy(g), CP.copy(wt, np.float32)
    for kind in (None, ('leaky', 0.01), ('leaky', 0.3), ('sigmoid', 0.0)):
        _, y = mask_factor(kind, m)
        md = None if y is None else CP.copy(y)
        if kind is None:
            tags, switch = _both_dispatches(rt, lambda: ops.conv2d_bwd_data(gd, wd, xs, (1, 1), (2, 2)))
        else:
            tags, switch = _both_dispatches(
                rt, lambda: ops.conv2d_bwd_data(gd, wd, xs, (1, 1), (2, 2), x_act=md, act=kind[0], alpha=kind[1]))
        assert CONV_KERNELS[rt.last_conv()[1]] == 't32'
        assert not np.isnan(tags).any() and np.array_equal(tags, switch), f'mask {kind}'
    if _experiments(rt):                        # the forward kernel, every activation kind, with and without bias
        xd, w2 = CP.copy(m), CP.copy(wt, np.float32)
        bd = CP.copy(np.array([0.3, -0.2]), np.float32)
        for act, alpha in ((None, 0.0), ('relu', 0.0), ('leaky', 0.01), ('sigmoid', 0.0)):
            for bias in (True, False):
                tags, switch = _both_dispatches(
                    rt, lambda: ops.conv2d_fwd(xd, w2, bd, (1, 1), (2, 2), 0.5, bias, act=act, alpha=alpha))
                assert CONV_KERNELS[rt.last_conv()[1]] == 't32'
                assert not np.isnan(tags).any() and np.array_equal(tags, switch), f'forward {act}, bias {bias}'


def _family_cases(CP, ops):
    """(name, run(kind)) per kernel family whose launcher turns the kinds into tags, at a tiny shape; kind = (act, alpha)."""
    rng = np.random.default_rng(7300)

    def dev(shape, scale=1.0):
        return CP.copy(rng.standard_normal(shape) * scale, np.float32)

    def conv(xs, ws, st, pd):
        x, w, b = dev(xs), dev(ws, 0.2), dev((ws[3],))
        oh, ow = ops.conv_out_hw(xs[1], xs[2], ws[:2], st, pd)
        g, m = dev((xs[0], oh, ow, ws[3])), dev(xs)
        fwd = lambda k: ops.conv2d_fwd(x, w, b, st, pd, 0.25, True, act=k[0], alpha=k[1])
        bwd = lambda k: ops.conv2d_bwd_data(g, w, xs, st, pd, x_act=None if k[0] is None else m, act=k[0], alpha=k[1])
        return fwd, bwd

    def up(ch):
        xl, w, b = dev((2, 5, 9, ch)), dev((5, 5, ch, ch), 0.2), dev((ch,))
        g = dev((2, 10, 18, ch))
        fwd = lambda k: ops.upconv2x_fwd(xl, w, b, (2, 2), True, k[0], k[1])
        bwd = lambda k: ops.upconv2x_bwd_data(g, w, xl.shape, (2, 2), x_act=None if k[0] is None else xl, act=k[0],
                                              alpha=k[1])
        return fwd, bwd

    f11, d11 = conv((2, 9, 21, 1), (5, 5, 1, 1), (1, 1), (2, 2))         # conv_fwd_px / conv_dgrad_px
    f11s, d11s = conv((2, 9, 21, 1), (5, 5, 1, 1), (2, 2), (2, 2))       # conv_fwd_px / conv_dgrad_s2<1, 1>
    f14s, d14s = conv((2, 9, 21, 1), (5, 5, 1, 4), (2, 2), (2, 2))       # conv_fwd_px / conv_dgrad_s2<1, 4>
    f44s, d44s = conv((2, 9, 21, 4), (5, 5, 4, 4), (2, 2), (2, 2))       # conv_fwd_px / conv_dgrad_s2<4, 4>
    f42, _ = conv((2, 9, 21, 4), (5, 5, 4, 2), (1, 1), (2, 2))           # conv_fwd_t542
    fch, dch = conv((2, 9, 21, 1), (5, 3, 1, 64), (2, 1), (0, 1))        # conv_fwd_fast / (Char conv_1 dx kernel)
    fu4, du4 = up(4)                                                      # upconv_fwd_kernel / upconv_dgrad_kernel
    fu1, _ = up(1)                                                        # up1_fwd_kernel
    fwd = [('fwd 1->1', f11), ('fwd 1->1 /2', f11s), ('fwd 1->4 /2', f14s), ('fwd 4->4 /2', f44s), ('fwd 4->2', f42),
           ('fwd 1->64 5x3', fch), ('upconv fwd 4', fu4), ('upconv fwd 1', fu1)]
    bwd = [('dx 1->1', d11), ('dx 1->1 /2', d11s), ('dx 1->4 /2', d14s), ('dx 4->4 /2', d44s), ('upconv dx 4', du4)]
    return fwd, bwd


def test_every_tagged_kernel_family_gives_the_bits_of_its_run_time_switch(ctx):
    from univer_ocr_amd.nn import ops
    CP, rt = ctx, ctx.runtime()
    fwd, bwd = _family_cases(CP, ops)
    differ = []
    for name, run in fwd:
        for kind in ((None, 0.0), ('relu', 0.0), ('leaky', 0.01), ('sigmoid', 0.0)):
            tags, switch = _both_dispatches(rt, lambda: run(kind))
            assert not np.isnan(tags).any()
            if not np.array_equal(tags, switch):
                differ.append(f'{name}, act {kind}: rel_linf {rel_linf(tags, switch):.2e}')
    for name, run in bwd:
        for kind in ((None, 0.0), ('leaky', 0.01), ('leaky', 0.3), ('sigmoid', 0.0)):
            tags, switch = _both_dispatches(rt, lambda: run(kind))
            assert not np.isnan(tags).any()
            if not np.array_equal(tags, switch):
                differ.append(f'{name}, mask {kind}: rel_linf {rel_linf(tags, switch):.2e}')
    assert not differ, '\n'.join(differ)


def test_kinds_the_nets_never_use_still_match_the_oracle(ctx):
    """act_dispatch stays 1: these pairs have no tags, so the launcher must fall back to the run-time instantiation."""
    from univer_ocr_amd.nn import ops
    CP, rt = ctx, ctx.runtime()
    xs, wt, g, m, ref_dx = problem(SHAPES[1])
    factor, y = mask_factor(('sigmoid', 0.0), m)
    dx = ops.conv2d_bwd_data(CP.copy(g), CP.copy(wt, np.float32), xs, (1, 1), (2, 2), x_act=CP.copy(y), act='sigmoid')
    per_image(dx, ref_dx * factor, 'Sigmoid mask on the 4 -> 2 layer')
    # a Sigmoid on a stride-2 forward conv (conv_fwd_px) is tagged; a ReLU there is not
    rng = np.random.default_rng(7400)
    x, w4, b4 = rng.standard_normal((2, 9, 21, 1)), rng.standard_normal((5, 5, 1, 4)) * 0.2, rng.standard_normal(4)
    for act, ref_fn in (('relu', O.relu_fwd), ('sigmoid', O.sigmoid_fwd)):
        ref = ref_fn(O.conv2d_fwd(x, w4, b4, (2, 2), (2, 2), 0.25, True))
        yv = ops.conv2d_fwd(CP.copy(x), CP.copy(w4, np.float32), CP.copy(b4, np.float32), (2, 2), (2, 2), 0.25, True,
                            act=act)
        per_image(yv, ref, f'{act} on a stride-2 forward')
    if _experiments(rt):
        b = np.array([0.3, -0.2])
        ref = O.relu_fwd(O.conv2d_fwd(m, wt, b, (1, 1), (2, 2), 0.5, True))
        yv = ops.conv2d_fwd(CP.copy(m), CP.copy(wt, np.float32), CP.copy(b, np.float32), (1, 1), (2, 2), 0.5, True,
                            act='relu')
        per_image(yv, ref, 'ReLU forward')
