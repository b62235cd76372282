"""The depth-tile loop and the epilogue of the float32 MFMA GEMM (univer-ocr_amd/csrc/gemm_mfma.hip) where they carry
state from tile to tile instead of rebuilding it: operand positions that are advanced by block-uniform distances, the
loop that exists once for 16-byte loads and once for element loads, and output addresses made of a wave-uniform part
and one register per lane.  Same style as test_gpu_gemm_configs.py, whose fixture, option helpers and Python copies of
the host rules are used here: MFMA whenever eligible, no shape-specialised kernels, outputs poisoned with NaN, the
float64 oracle, 1e-5 for y and dx and 2e-5 for dw and db.

The shapes are the smallest that reach what can go wrong:
  * 1, 2 and 3 depth tiles per tap, with the taps of the Char net's (5, 3) stride (2, 1) conv and of a padded 3 x 3 conv
    with a padding value; M = 100 / 280 (no multiple of 64, a row tile spans two images); 64 and 8 output columns;
  * backward-data at strides (2, 1) and (2, 2) with w = 64 (whole depth tiles are skipped), unsplit and with slabs of
    3 tiles at 2 tiles per tap (every second slab starts on the odd tile of a tap), with and without the mask;
  * dense layers whose depth ends first, last and mid-group of a 16-byte group and on a tile boundary, at 1 to 3 row
    tiles and 1 to 3 column tiles with ragged edges;
  * every loader in the element-wise loop;
  * the same bits for 64- and 128-row tiles, both block numberings, and a deferred group against separate launches.
"""
import contextlib
import functools

import numpy as np
import pytest

import test_gpu_gemm_configs as G
from oracle import nn_oracle as O
from test_gpu_gemm_configs import ctx  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

TOL_Y, TOL_W = G.TOL_Y, G.TOL_W
UNSPLIT = dict(split_blocks=0, split_min=3)


@contextlib.contextmanager
def options(rt, **opt):
    G.set_gemm_options(rt, {**dict(G.GEMM_DEFAULTS), **opt})
    try:
        yield {**dict(G.GEMM_DEFAULTS), **opt}
    finally:
        G.set_gemm_options(rt, dict(G.GEMM_DEFAULTS))


def ran(CP, gemm, opt, what):
    """last_gemm is what the host rule gives for `gemm` = (M, N, depth, allow_split): the MFMA GEMM ran, as configured"""
    got, exp = CP.runtime().last_gemm(), G.expect_gemm(*gemm, G.cu_count(CP), G.WS_HALF, opt)
    assert got == exp, f'{what} {opt}: last_gemm {got} != host rule {exp}'
    return got


@functools.lru_cache(maxsize=None)
def conv_problem(xs, ks, cout, st, pd, pv):
    """inputs and float64 results of one conv (computed once, read-only)"""
    rng = np.random.default_rng(abs(hash((xs, ks, cout, st, pd))) % (1 << 32))
    X = rng.standard_normal(xs)
    w = rng.standard_normal((*ks, xs[3], cout)) * 0.1
    b = rng.standard_normal(cout)
    y = O.conv2d_fwd(X, w, b, st, pd, pv, True)
    g = rng.standard_normal(y.shape)
    dx, dw, db = O.conv2d_bwd(X, w, g, st, pd, pv, True)
    m, slope = G.mask_of('leaky', rng, xs)
    out = dict(X=X, w=w, b=b, g=g, m=m, y=y, y_nobias=O.conv2d_fwd(X, w, b, st, pd, pv, False), dx=dx, dxm=dx * slope,
               dw=dw, db=db)
    for v in out.values():
        v.setflags(write=False)
    return out


# ---- 1. positions across tap boundaries --------------------------------------------------------------------------------
GEOMETRY = [((5, 3), (2, 1), (0, 1), 0.0), ((3, 3), (1, 1), (1, 1), 0.5)]      # kernel, stride, padding, padding value
IMAGE = (2, 14, 10)


def run_forward(CP, p, xs, ks, cout, st, pd, pv, what):
    from univer_ocr_amd.nn import ops
    Xd, wd, bd = CP.copy(p['X']), CP.copy(p['w']), CP.copy(p['b'])
    gemm = G.conv_gemms(xs, ks, cout, st, pd)[0]
    assert gemm[0] % 64 and (gemm[0] // xs[0]) % 64, gemm       # ragged last row tile; a tile that spans two images
    for opt in (UNSPLIT, {}):
        with options(CP.runtime(), **opt) as full:
            y = ops.conv2d_fwd(Xd, wd, bd, st, pd, pv, True, act='leaky', alpha=0.01)
            ran(CP, gemm, full, what)
            y0 = ops.conv2d_fwd(Xd, wd, bd, st, pd, pv, False)
            G.check(y, O.leaky_relu_fwd(p['y'], 0.01), TOL_Y, f'{what} leaky(y) {opt}')
            G.check(y0, p['y_nobias'], TOL_Y, f'{what} y without bias {opt}')


def run_dgrad(CP, p, xs, ks, cout, st, pd, what, option_sets=(UNSPLIT, {})):
    from univer_ocr_amd.nn import ops
    gd, wd, md = CP.copy(p['g']), CP.copy(p['w']), CP.copy(p['m'])
    gemm = G.conv_gemms(xs, ks, cout, st, pd)[1]
    seen = []
    for opt in option_sets:
        with options(CP.runtime(), **opt) as full:
            dx = ops.conv2d_bwd_data(gd, wd, xs, st, pd)
            if cout % G.BD == 0:
                seen.append(ran(CP, gemm, full, what))
            dxm = ops.conv2d_bwd_data(gd, wd, xs, st, pd, x_act=md, act='leaky', alpha=0.01)
            G.check(dx, p['dx'], TOL_Y, f'{what} dx {opt}')
            G.check(dxm, p['dxm'], TOL_Y, f'{what} masked dx {opt}')
    return seen


@pytest.mark.parametrize('cout', [64, 8])
@pytest.mark.parametrize('geometry', range(len(GEOMETRY)))
@pytest.mark.parametrize('cin', [32, 64, 96])
def test_taps_forward_and_dgrad(cin, geometry, cout, ctx):     # noqa: F811
    """cin / 32 depth tiles per tap in the forward GEMM (and cout / 32 in backward-data), unsplit and split"""
    ks, st, pd, pv = GEOMETRY[geometry]
    xs = IMAGE + (cin,)
    p = conv_problem(xs, ks, cout, st, pd, pv)
    what = f'{xs} {ks} stride {st} -> {cout}'
    run_forward(ctx, p, xs, ks, cout, st, pd, pv, f'fwd {what}')
    run_dgrad(ctx, p, xs, ks, cout, st, pd, f'dgrad {what}')


@pytest.mark.parametrize('geometry', range(len(GEOMETRY)))
@pytest.mark.parametrize('cout', [32, 96])
def test_taps_dgrad_one_and_three_tiles(cout, geometry, ctx):     # noqa: F811
    """backward-data sums over (tap, cout): 1 and 3 depth tiles per tap (2 are in the test above)"""
    ks, st, pd, pv = GEOMETRY[geometry]
    xs = IMAGE + (32,)
    run_dgrad(ctx, conv_problem(xs, ks, cout, st, pd, pv), xs, ks, cout, st, pd, f'dgrad {xs} {ks} stride {st} <- {cout}')


# ---- 2. skipped tiles and slab starts ----------------------------------------------------------------------------------
@pytest.mark.parametrize('st', [(2, 1), (2, 2)])
def test_dgrad_skipped_tiles_and_odd_slab_starts(st, ctx):     # noqa: F811
    """w = 64: the rows of a block lie in one image row, so the tap rows that miss it are stepped over.  30 depth tiles,
    2 per tap; 10 slabs of 3 tiles: slabs 1, 3, ... start on the second tile of a tap."""
    xs, ks, cout, pd = (2, 6, 64, 8), (5, 3), 64, (2, 1)
    M, N, depth, allow = G.conv_gemms(xs, ks, cout, st, pd)[1]
    tiles = G.cdiv(M, 64) * G.cdiv(N, G.BN)
    assert allow and G.cdiv(depth, G.BD) == 30 and G.slab_lengths(depth, 10) == [3] * 10
    forced = dict(gemm_bm=64, split_blocks=10 * tiles, split_min=2)
    seen = run_dgrad(ctx, conv_problem(xs, ks, cout, st, pd, 0.0), xs, ks, cout, st, pd, f'dgrad {xs} stride {st}',
                     (dict(gemm_bm=64, **UNSPLIT), forced))
    assert [s[3] for s in seen] == [1, 10], seen


# ---- 3. ragged depth and the ones column -------------------------------------------------------------------------------
DEPTHS = [31, 32, 33, 95, 100]
MS = [1, 63, 65, 130]
NS = [4, 60, 68, 162]


@functools.lru_cache(maxsize=None)
def dense_ref(m, n_in, n_out):
    rng = np.random.default_rng(m * 1000003 + n_in * 1009 + n_out)
    X, w, g = G.dense_problem(rng, m, n_in, n_out)
    dx, dw = O.dense_bwd(X, w, g)
    out = dict(X=X, w=w, g=g, y=O.dense_fwd(X, w), dx=dx, dw=dw)
    for v in out.values():
        v.setflags(write=False)
    return out


@pytest.mark.parametrize('depth', DEPTHS)
def test_dense_ragged_depth(depth, ctx):     # noqa: F811
    """`depth` stored elements along the summed index of each dense GEMM: forward (n_in = depth, then the ones column),
    dx (n_out = depth) and dw (m = depth; its M = n_in + 1 rows end with the ones row, so M = 1 does not exist: the
    stored rows are 1, 62, 64 and 129), each at M x N from MS x NS, unsplit and with the automatic split."""
    from univer_ocr_amd.nn import ops
    CP = ctx
    for opt in (UNSPLIT, {}):
        with options(CP.runtime(), **opt) as full:
            for a in MS:
                for n in NS:
                    tag = f'depth {depth}, {a} x {n} {opt}'
                    p = dense_ref(a, depth, n)                                      # forward: M = m, N = n_out
                    y = ops.dense_fwd(CP.copy(p['X']), CP.copy(p['w']))
                    ran(CP, (a, n, depth + 1, True), full, f'fwd {tag}')
                    G.check(y, p['y'], TOL_Y, f'y {tag}')
                    p = dense_ref(a, n, depth)                                      # dx: M = m, N = n_in
                    dx = CP.empty((a, n))
                    G.dense_call(CP, CP.copy(p['X']), CP.copy(p['w']), CP.copy(p['g']), dx, None, False)
                    ran(CP, (a, n, depth, True), full, f'dx {tag}')
                    G.check(dx, p['dx'], TOL_Y, f'dx {tag}')
                    n_in = max(1, a - 1)                                            # dw: M = n_in + 1, N = n_out
                    p = dense_ref(depth, n_in, n)
                    dw = CP.empty(p['w'].shape)
                    G.dense_call(CP, CP.copy(p['X']), CP.copy(p['w']), CP.copy(p['g']), None, dw, False)
                    ran(CP, (n_in + 1, n, depth, True), full, f'dw {tag}')
                    G.check(dw, p['dw'], TOL_W, f'dw {tag}')


# ---- 4. the element-wise loop, one case per loader ---------------------------------------------------------------------
def test_every_loader_off_alignment(ctx):     # noqa: F811
    """One operand 4 bytes past a 16-byte boundary puts the whole block into the loop with element loads; the operand
    that is aligned keeps its 16-byte loads there.  Sizes are multiples of 4."""
    from univer_ocr_amd.nn import ops
    CP = ctx
    off = functools.partial(G.misaligned, CP)
    m, n_in, n_out = 65, 100, 68
    p = dense_ref(m, n_in, n_out)
    X, w, g = CP.copy(p['X']), CP.copy(p['w']), CP.copy(p['g'])
    G.check(ops.dense_fwd(off(p['X']), w), p['y'], TOL_Y, 'ARowMajor: dense forward, x off alignment')
    G.check(ops.dense_fwd(X, off(p['w'])), p['y'], TOL_Y, 'BRowMajor: dense forward, w off alignment')
    dx = CP.empty((m, n_in))
    G.dense_call(CP, X, off(p['w']), g, dx, None, False)
    G.check(dx, p['dx'], TOL_Y, 'BDepthContig: dense dx, w off alignment')
    dw = CP.empty(p['w'].shape)
    G.dense_call(CP, off(p['X']), w, g, None, dw, False)
    G.check(dw, p['dw'], TOL_W, 'AColMajor: dense dw, x off alignment')
    (ks, st, pd, pv), xs, cout = GEOMETRY[0], IMAGE + (64,), 64
    c = conv_problem(xs, ks, cout, st, pd, pv)
    Xc, bc, gc = CP.copy(c['X']), CP.copy(c['b']), CP.copy(c['g'])
    fwd, dgrad, wgrad = G.conv_gemms(xs, ks, cout, st, pd)
    y = ops.conv2d_fwd(Xc, off(c['w']), bc, st, pd, pv, True)
    ran(CP, fwd, dict(G.GEMM_DEFAULTS), 'conv forward')
    G.check(y, c['y'], TOL_Y, 'AConvFwd: conv forward, w off alignment')
    dx = ops.conv2d_bwd_data(gc, off(c['w']), xs, st, pd)
    ran(CP, dgrad, dict(G.GEMM_DEFAULTS), 'conv dx')
    G.check(dx, c['dx'], TOL_Y, 'AConvDgrad: conv dx, w off alignment')
    dw, db = CP.empty(c['w'].shape, np.float32), CP.empty((cout,), np.float32)
    ops.conv2d_bwd_weight(Xc, off(c['g']), dw, db, st, pd, pv, True, accumulate=False)
    ran(CP, wgrad, dict(G.GEMM_DEFAULTS), 'conv dw')
    G.check(dw, c['dw'], TOL_W, 'AConvWgrad: conv dw, dy off alignment')
    G.check(db, c['db'], TOL_W, 'AConvWgrad: conv db, dy off alignment')


# ---- 5. the same bits --------------------------------------------------------------------------------------------------
def same_bits(CP, run, gemm, refs, what):
    """run() under 64- and 128-row tiles x both block numberings, unsplit and in 2 slabs: within the tolerance of the
    oracle, and bit for bit the same at one slab count"""
    M, N, depth, allow = gemm
    first = {}
    for bm in (64, 128):
        tiles = G.cdiv(M, bm) * G.cdiv(N, G.BN)
        for split in (dict(UNSPLIT), dict(split_blocks=2 * tiles, split_min=2)):
            for xcd in (0, 1):
                with options(CP.runtime(), gemm_bm=bm, xcd_remap=xcd, **split) as full:
                    outs = [G.host(o) for o in run()]
                    got = ran(CP, gemm, full, what)
                tag = f'{what} bm={bm} xcd_remap={xcd} slabs={got[3]}'
                for o, (ref, tol, name) in zip(outs, refs):
                    G.check(o, ref, tol, f'{name} [{tag}]')
                base = first.setdefault(got[3], (tag, outs))
                for o, o0, (_, _, name) in zip(outs, base[1], refs):
                    assert np.array_equal(o, o0), f'{name}: [{tag}] differs from [{base[0]}]'
    assert set(first) == ({1, 2} if allow and G.cdiv(depth, G.BD) >= 4 else {1}), sorted(first)


BITS_CONV = (IMAGE + (96,), (5, 3), 64, (2, 1), (0, 1), 0.0)
BITS_DENSE = (130, 100, 68)                       # dw sums over 130, forward over 100 + the ones column: ragged depths


def test_same_bits_conv(ctx):     # noqa: F811
    from univer_ocr_amd.nn import ops
    CP = ctx
    xs, ks, cout, st, pd, pv = BITS_CONV
    p = conv_problem(xs, ks, cout, st, pd, pv)
    Xd, wd, bd, gd, md = (CP.copy(p[k]) for k in ('X', 'w', 'b', 'g', 'm'))
    fwd, dgrad, _ = G.conv_gemms(xs, ks, cout, st, pd)
    same_bits(CP, lambda: (ops.conv2d_fwd(Xd, wd, bd, st, pd, pv, True, act='leaky', alpha=0.01),), fwd,
              [(O.leaky_relu_fwd(p['y'], 0.01), TOL_Y, 'leaky(y)')], 'conv forward')
    same_bits(CP, lambda: (ops.conv2d_bwd_data(gd, wd, xs, st, pd, x_act=md, act='leaky', alpha=0.01),), dgrad,
              [(p['dxm'], TOL_Y, 'masked dx')], 'conv dx')


def test_same_bits_dense(ctx):     # noqa: F811
    from univer_ocr_amd.nn import ops
    CP = ctx
    m, n_in, n_out = BITS_DENSE
    p = dense_ref(m, n_in, n_out)
    Xd, wd, gd = CP.copy(p['X']), CP.copy(p['w']), CP.copy(p['g'])
    same_bits(CP, lambda: (ops.dense_fwd(Xd, wd),), (m, n_out, n_in + 1, True), [(p['y'], TOL_Y, 'y')], 'dense forward')

    def dx():
        out = CP.empty((m, n_in))
        G.dense_call(CP, Xd, wd, gd, out, None, False)
        return (out,)

    def dw():
        out = CP.empty(p['w'].shape)
        G.dense_call(CP, Xd, wd, gd, None, out, False)
        return (out,)

    same_bits(CP, dx, (m, n_in, n_out, True), [(p['dx'], TOL_Y, 'dx')], 'dense dx')
    same_bits(CP, dw, (n_in + 1, n_out, m, True), [(p['dw'], TOL_W, 'dw')], 'dense dw')


def test_same_bits_group_and_separate_launches(ctx):     # noqa: F811
    """The conv dw (depth 100) and the dense dw (depth 130) as one deferred group and as two launches, unsplit and at
    the slab counts the group chooses: the same bits."""
    from univer_ocr_amd.nn import ops
    CP = ctx
    rt = CP.runtime()
    xs, ks, cout, st, pd, pv = BITS_CONV
    c = conv_problem(xs, ks, cout, st, pd, pv)
    d = dense_ref(*BITS_DENSE)
    Xc, gc = CP.copy(c['X']), CP.copy(c['g'])
    Xd, wd, gd = CP.copy(d['X']), CP.copy(d['w']), CP.copy(d['g'])
    problems = [G.conv_gemms(xs, ks, cout, st, pd)[2][:3], (BITS_DENSE[1] + 1, BITS_DENSE[2], BITS_DENSE[0])]
    assert problems[0][2] == 100
    cu = G.cu_count(CP)

    def conv_dw():
        dw, db = CP.full(c['w'].shape, 0.5), CP.full((cout,), 0.25)
        ops.conv2d_bwd_weight(Xc, gc, dw, db, st, pd, pv, True, accumulate=True)
        return dw, db

    def dense_dw():
        dw = CP.full(d['w'].shape, 0.5)
        ops.dense_bwd(Xd, wd, gd, dw, accumulate=True, need_dx=False)
        return (dw,)

    split_at = next(v for v in range(2, 1 << 14) if min(G.expect_group(problems, cu, G.WS_HALF, v, 1024, 2)) > 1)
    for group_opt in (dict(UNSPLIT), dict(group_blocks=split_at, split_min=2)):
        splits = G.expect_group(problems, cu, G.WS_HALF, group_opt.get('group_blocks', 0),
                                group_opt.get('split_blocks', 1024), group_opt['split_min'])
        with options(rt, **group_opt):
            with rt.defer_wgrad():
                grouped = [conv_dw(), dense_dw()]
            assert rt.last_gemm_group() == (2, sum(s > 1 for s in splits)) and rt.last_gemm()[3] == max(splits)
            grouped = [[G.host(o) for o in outs] for outs in grouped]
        apart = []
        for job, (M, N, depth), s in zip((conv_dw, dense_dw), problems, splits):
            opt = dict(UNSPLIT) if s == 1 else dict(split_blocks=s * G.cdiv(M, 64) * G.cdiv(N, G.BN), split_min=2)
            with options(rt, gemm_bm=64, **opt):
                apart.append([G.host(o) for o in job()])
                assert rt.last_gemm()[0] == 64 and rt.last_gemm()[3] == s, (rt.last_gemm(), s)
        refs = [(c['dw'] + 0.5, c['db'] + 0.25), (d['dw'] + 0.5,)]
        for outs, outs0, ref, name in zip(grouped, apart, refs, ('conv', 'dense')):
            for o, o0, r in zip(outs, outs0, ref):
                G.check(o, r, TOL_W, f'{name} dw / db in the group, slabs {splits}')
                assert np.array_equal(o, o0), f'{name}: group and separate launch differ at slabs {splits}'
