"""dw / db under channel scaling, bit for bit.

An elementwise bound (elementwise_bound.py) for a weight gradient sums over thousands of positions and is too wide to
tell anything.  Another property is exact instead: scaling input channel ci by 2^a and gradient channel co by 2^b
scales dw[:, :, ci, co] by exactly 2^(a + b) and db[co] by 2^b -- power-of-two scaling commutes with every rounding
(nothing overflows or underflows here), and no kernel's summation order depends on the data.  It holds for a padding
value of 0 and accumulate = False.  A kernel that mixes channels before it rounds (a shared partial sum, an operand
packed with a neighbour's, a reduction across the lanes of different channels) breaks it.

Every family runs twice, uniform and channel-scaled (float32: a, b in [-8, 8]; binary16: [-3, 3], x and dy stay in
the normal range); the bits of the scaled run must equal the uniform run's after the exact rescaling, and the scaled
run is judged against the float64 oracle PER (ci, co) SLICE at the project's 2e-5 (rel_linf of the slice: a small
slice is no longer hidden behind a large one).

  table    the FastConv table configurations with more than one channel at the nets' padding, float32 (default dispatch
           and t32 = 0, tiled = 0) and binary16 (h16 = 1 and 0), pages of 3 x 37 x 141; `Runtime.last_conv` must name
           the family test_gpu_conv_padding.expect_kernel expects
  mfma     the MFMA implicit-GEMM weight gradient (mfma = 2, 3x3, 32 -> 32)
  up4      upconv2x_bwd_weight 4 -> 4 on 2 x 19 x 71, float32 and binary16
  dense    dense_bwd dw (bias row included) at (67, 200) x (200, 70): one element per slice, so x and dy are positive

Well-posedness, by the rule of test_gpu_conv_padding.py: x and dy are negative with probability 1/4 only, so no slice
cancels, and every case takes the first of 20 seeds for which a float32 NumPy restatement of the oracle stays within
a QUARTER of the tolerance on every slice (`test_every_case_has_a_qualifying_seed`, no GPU); a case without one fails.
"""
import functools
from collections import namedtuple

import numpy as np
import pytest

import elementwise_bound as B
from oracle import nn_oracle as O
from test_gpu_conv_padding import DEFAULTS, KERNELS, KID, TABLE, WGRAD, ctx, expect_kernel, make_dims  # noqa: F401

TOL = 2e-5                                      # dw / db (test_gpu_kernels.py, test_gpu_f16.py)
SEEDS = 20
SCALE_EXP = {'float32': 8, 'float16': 3}
OVER_INIT = (7.0, -3.0)                         # what an overwriting call must replace
Case = namedtuple('Case', 'id kind dtype geom opts seed_base')     # opts: ((key, value), ...)


def _cases():
    out = []
    for i, cfg in enumerate(TABLE):
        if cfg.cin == 1 and cfg.cout == 1:
            continue
        geom = (*cfg[:6], *cfg.net_pad)
        out.append(Case(f'32-table{i}', 'conv', 'float32', geom, (), 7000000 + 64 * i))
        out.append(Case(f'32-table{i}-t32_0-tiled0', 'conv', 'float32', geom, (('t32', 0), ('tiled', 0)), 7000000 + 64 * i))
        out.append(Case(f'16-table{i}', 'conv', 'float16', geom, (), 7100000 + 64 * i))
        out.append(Case(f'16-table{i}-h16_0', 'conv', 'float16', geom, (('h16', 0),), 7100000 + 64 * i))
    out.append(Case('32-mfma2', 'conv', 'float32', B.MFMA_GEOM, (('mfma', 2),), 7200000))
    out.append(Case('32-up4', 'up', 'float32', 4, (), 7300000))
    out.append(Case('16-up4', 'up', 'float16', 4, (), 7400000))
    out.append(Case('32-dense', 'dense', 'float32', None, (), 7500000))
    return tuple(out)


CASES = _cases()
CASE_IDS = [c.id for c in CASES]


def dims_of(c):
    return make_dims(*B.SHAPE, *c.geom)


def draw(c, seed):
    """x, dy (uniform magnitudes in [0.25, 1], representable in the storage type) and the channel exponents a, b"""
    rng = np.random.default_rng(seed)

    def tensor(shape, negative=0.25):
        m = rng.uniform(0.25, 1.0, shape) * np.where(rng.random(shape) < negative, -1.0, 1.0)
        return m.astype(B.STORE[c.dtype]).astype(np.float64)

    if c.kind == 'conv':
        d = dims_of(c)
        x, g = tensor((d.n, d.h, d.w, d.cin)), tensor((d.n, d.oh, d.ow, d.cout))
    elif c.kind == 'up':
        n, hl, wl = B.LOW_SHAPE
        x, g = tensor((n, hl, wl, c.geom)), tensor((n, 2 * hl, 2 * wl, c.geom))
    else:
        x, g = tensor((B.DENSE_M, B.DENSE_K), 0.0), tensor((B.DENSE_M, B.DENSE_N), 0.0)
    k = SCALE_EXP[c.dtype]
    return x, g, B.spread(rng, x.shape[-1], k), B.spread(rng, g.shape[-1], k)


def oracle(c, x, g, dt=np.float64):
    """(dw, db) of the uniform inputs by the oracle's code in `dt` arithmetic; dense: dw (K, N) and its bias row"""
    x, g = x.astype(dt), g.astype(dt)
    if c.kind == 'conv':
        d = dims_of(c)
        _, dw, db = O.conv2d_bwd(x, np.zeros((d.kh, d.kw, d.cin, d.cout), dt), g, (d.sh, d.sw), (d.ph, d.pw), dt(0.0), True)
    elif c.kind == 'up':
        _, dw, db = O.conv2d_bwd(O.upsample2d_fwd(x, (2, 2)), np.zeros((5, 5, c.geom, c.geom), dt), g, 1, 2, dt(0.0), True)
    else:
        full = O.dense_bwd(x, np.zeros((B.DENSE_K + 1, B.DENSE_N), dt), g)[1]
        dw, db = full[None, None, :-1], full[-1]
    assert dw.dtype == dt and db.dtype == dt
    return dw, db


def slice_errors(dw, db, ref_dw, ref_db):
    """rel_linf of every (ci, co) slice of dw and of every db[co]"""
    dw, db = np.asarray(dw, dtype=np.float64), np.asarray(db, dtype=np.float64)
    e_w = np.abs(dw - ref_dw).max(axis=(0, 1)) / np.abs(ref_dw).max(axis=(0, 1))
    return np.where(np.isnan(e_w), np.inf, e_w), np.where(np.isnan(db), np.inf, np.abs(db - ref_db) / np.abs(ref_db))


@functools.lru_cache(maxsize=None)
def qualified(c):
    """(seed, x, g, a, b, ref dw, ref db) of the first seed whose float32 restatement keeps every slice within a quarter
    of TOL, or (None, worst figure)"""
    worst = None
    for seed in range(c.seed_base, c.seed_base + SEEDS):
        x, g, a, b = draw(c, seed)
        ref_dw, ref_db = oracle(c, x, g)
        e_w, e_b = slice_errors(*oracle(c, x, g, np.float32), ref_dw, ref_db)
        worst = max(e_w.max(), e_b.max())
        if worst <= TOL / 4:
            return seed, x, g, a, b, ref_dw, ref_db
    return None, worst


@pytest.mark.parametrize('index', range(len(CASES)), ids=CASE_IDS)
def test_every_case_has_a_qualifying_seed(index):
    found = qualified(CASES[index])
    assert found[0] is not None, f'no qualifying seed among {SEEDS}: float32 restatement at {found[1]:.2e}'
    _, x, g, a, b, _, _ = found
    k = SCALE_EXP[CASES[index].dtype]
    assert np.ptp(a) + np.ptp(b) > 0 and max(np.abs(a).max(), np.abs(b).max()) <= k
    if CASES[index].dtype == 'float16':         # the scaled operands stay binary16 normals
        for t, e in ((x, a), (g, b)):
            s = np.abs(t * 2.0 ** e)
            assert B.F16_MIN <= s.min() and s.max() <= B.F16_MAX and np.array_equal(B.r16(s), s)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize('index', range(len(CASES)), ids=CASE_IDS)
def test_channel_scaling_scales_dw_and_db_bit_for_bit(index, ctx):
    from univer_ocr_amd.nn import ops
    CP, rt = ctx, ctx.runtime()
    c = CASES[index]
    found = qualified(c)
    assert found[0] is not None, f'no qualifying seed among {SEEDS}'
    seed, x, g, a, b, ref_dw, ref_db = found
    for key, value in DEFAULTS:
        rt.set_option(key, dict(c.opts).get(key, value))
    CP.set_dtype(c.dtype)
    failures = []

    def run(xs, gs):
        xd, gd = CP.copy(xs), CP.copy(gs)
        if c.kind == 'dense':
            full = CP.full((B.DENSE_K + 1, B.DENSE_N), OVER_INIT[0], np.float32)
            ops.dense_bwd(xd, CP.full(full.shape, 0.0, np.float32), gd, full, accumulate=False, need_dx=False)
            host = CP.asnumpy(full)
            return host[None, None, :-1], host[-1]
        dw, db = CP.full(ref_dw.shape, OVER_INIT[0], np.float32), CP.full(ref_db.shape, OVER_INIT[1], np.float32)
        if c.kind == 'up':
            ops.upconv2x_bwd_weight(xd, gd, dw, db, (2, 2), True, accumulate=False)
        else:
            d = dims_of(c)
            ops.conv2d_bwd_weight(xd, gd, dw, db, (d.sh, d.sw), (d.ph, d.pw), 0.0, True, accumulate=False)
            want = (WGRAD, KID[expect_kernel(WGRAD, c.dtype, d, 0.0, dict(c.opts))])
            if rt.last_conv() != want:
                got = rt.last_conv()
                failures.append(f'last_conv {got} ({KERNELS[got[1]]}) != {want} ({KERNELS[want[1]]})')
        return CP.asnumpy(dw), CP.asnumpy(db)

    dw0, db0 = run(x, g)
    dw1, db1 = run(x * 2.0 ** a, g * 2.0 ** b)
    assert dw0.dtype == np.float32 and db0.dtype == np.float32
    f_w, f_b = (2.0 ** (a[:, None] + b[None, :])).astype(np.float32), (2.0 ** b).astype(np.float32)
    same_w = _bits(dw1) == _bits(dw0 * f_w)
    same_b = _bits(db1) == _bits(db0 * f_b)
    e_w, e_b = slice_errors(dw1, db1, ref_dw * f_w, ref_db * f_b)
    e_w0, e_b0 = slice_errors(dw0, db0, ref_dw, ref_db)
    print(f'{c.id} seed {seed}: dw bits differ in {int((~same_w).sum())} of {same_w.size}, db in {int((~same_b).sum())} of '
          f'{same_b.size}; worst slice rel_linf dw {e_w.max():.2e} (uniform {e_w0.max():.2e}), db {e_b.max():.2e} '
          f'(uniform {e_b0.max():.2e})')
    if not same_w.all():
        ci, co = np.argwhere(~same_w.all(axis=(0, 1)))[0]
        failures.append(f'dw differs in {int((~same_w).sum())} elements after the exact rescaling, first slice ({ci}, {co}): '
                        f'2^{a[ci] + b[co]}')
    if not same_b.all():
        failures.append(f'db differs in channels {np.flatnonzero(~same_b).tolist()} after the exact rescaling')
    if not e_w.max() <= TOL:
        failures.append(f'dw: worst slice rel_linf {e_w.max():.3e} > {TOL:.1e} at {np.unravel_index(e_w.argmax(), e_w.shape)}')
    if not e_b.max() <= TOL:
        failures.append(f'db: worst rel error {e_b.max():.3e} > {TOL:.1e} at {int(e_b.argmax())}')
    assert not failures, '\n'.join(failures)
