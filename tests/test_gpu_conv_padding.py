"""The shape-specialised conv kernels (conv_fast.hip's FastConv table) at paddings the nets never use, against the
float64 oracle.

`uocr_conv2d_fwd / _bwd_data / _bwd_weight` pick a kernel from two ladders (conv_api.hip, then conv_fast.hip).  The
nine table kernels match on kernel size, channels and stride only; everything that shadows them (conv_c16_*,
conv_dgrad_s2, conv_dgrad_c64s2, conv_wgrad_t542, conv_wgrad_s2_tiled, conv_tiled, conv_t32*, conv_h16*) also wants
the net's own padding or a "same" output.  The other conv tests use the nets' padding, so several table kernels never
ran there and the padding-dependent branches of those that did (the aligned float4 row path `load_row_c1`, the packed
store, the clamp-and-select border) saw one padding each.  This module crosses the nine configurations with

  dtype     float32, float16
  padding   the net's own; (0, 0); one component K/2 in either order (the float4 row path under a foreign ph, the
            scalar path at w % 4 == 0); neither component K/2; K - 1; >= K (whole windows in the border)
  size      72 and 44 columns (w % 4 == 0, w % 8 == 0 / 4: for every packed store `ow % PX` / `w % PX` is zero at one
            and non-zero at the other wherever the padding allows both) and 37 (odd); 27 / 18 / 21 rows: the weight
            gradient runs bands of four output rows, the last one short for most paddings; batches of 2 and 3
  pad_value 0, 0.75

and rotates bias, the forward activation (none / relu / leaky / sigmoid) and the dx mask (none / leaky / sigmoid) over
them.  Cases at the NET's padding reach the shadowed table kernels through the options (`t32` = 0, `tiled` = 0,
`h16` = 0).  After every launch `Runtime.last_conv` (uocr_ctx_last_conv) must report what `expect_kernel`, a Python
copy of the two ladders, expects: a later dispatch change cannot quietly turn these into tests of the generic kernel.

References and tolerances are the project's own.  float32 (test_gpu_kernels.py): y / dx / masked dx 1e-5, dw / db
2e-5, accumulated onto 0.5 / 0.25 and overwritten.  binary16 (test_gpu_f16.py): the oracle on the binary16-rounded
x / dy / mask, float32 master weights (rounded to binary16 only where the expected kernel is a conv_h16 one), a
gradient scale of 2^4; stored tensors 1e-3 (TOL_STORE), dw / db 2e-5 (TOL_EXACT).  All rel_linf.  Every array the ops
allocate starts as NaN.

Well-posedness.  rel_linf divides by max |expected|, and a one-channel db is ONE number: a sum of thousands of terms
that, for a zero-mean dy, cancels against the 0.25 it is accumulated onto -- float32 NumPy alone then misses the
float64 oracle by up to 1e-5, half the tolerance, before any kernel has run.  So dy is drawn with mean 0.5 (db cannot
cancel), and every case takes the first of 20 seeds for which a float32 NumPy restatement of ALL its outputs (the
oracle's own code on float32 operands) stays within a QUARTER of that output's tolerance; the factor 4 is room for a
summation order other than NumPy's.  In binary16 mode the restatement is float32 arithmetic on the binary16 operands
before the output is rounded: that rounding is at most 2^-11 = 4.9e-4 of the largest element by itself and is the
kernel's, not the reference's.  The search needs no GPU (`test_every_case_has_a_qualifying_seed`); a case without a
qualifying seed fails, it is never dropped.
"""
import itertools
from collections import namedtuple

import numpy as np
import pytest

from conftest import rel_linf
from oracle import nn_oracle as O

TOL_Y32, TOL_G32 = 1e-5, 2e-5                   # test_gpu_kernels.py
TOL_STORE, TOL_EXACT = 1e-3, 2e-5               # test_gpu_f16.py
GSCALE = 4                                      # binary16: dy carries 2^4 (test_gpu_f16.py)
SEEDS = 20
DEFAULTS = (('max_blocks', 0), ('wgrad_bands', 0), ('pair_band', 0), ('t32', 2), ('h16', 1), ('mfma', 1),
            ('fast_paths', 1), ('tiled', 1))
ACC_INIT, OVER_INIT = (0.5, 0.25), (7.0, -3.0)  # dw, db when accumulating; what an overwriting call must replace

# UOCR_CONV_* (include/univer_hip.h)
KERNELS = ('none', 'generic', 'mfma', 'h16', 'h16_wgrad', 'h16_wgrad_s2', 't32', 't32_wgrad', 'h3', 'tiled',
           'c16_expand', 'c16_reduce', 'c16_wgrad', 'dgrad_s2', 'dgrad_c64s2', 'wgrad_t542', 'wgrad_s2_tiled',
           'table_fast', 'table_px')
KID = {name: i for i, name in enumerate(KERNELS)}
FWD, DGRAD, WGRAD = 0, 1, 2

Dims = namedtuple('Dims', 'n h w cin cout kh kw sh sw ph pw oh ow')
# FAST_CONVS (conv_fast.hip): kernel, channels, stride | fwd.px, dx.px, the pixels per thread of conv_fwd_px and
# conv_dgrad_px (0 = the row names the *_fast kernel instead), and dw.px of conv_wgrad_fast | the net's padding
Cfg = namedtuple('Cfg', 'kh kw cin cout sh sw fpx dpx wpx net_pad')
TABLE = (
    Cfg(3, 3, 1, 16, 1, 1, 0, 4, 1, (1, 1)),    # Monochrome conv_1
    Cfg(3, 3, 16, 1, 1, 1, 4, 2, 1, (1, 1)),    # Monochrome conv_2
    Cfg(5, 5, 1, 1, 2, 2, 4, 0, 4, (2, 2)),     # Paragraph down_1/2
    Cfg(5, 5, 1, 1, 1, 1, 4, 8, 8, (2, 2)),     # Paragraph up_2, up_1, end
    Cfg(5, 5, 1, 4, 2, 2, 4, 0, 1, (2, 2)),     # Line down_1
    Cfg(5, 5, 4, 4, 2, 2, 4, 0, 2, (2, 2)),     # Line down_2
    Cfg(5, 5, 4, 4, 1, 1, 4, 4, 4, (2, 2)),     # Line up_2, up_1
    Cfg(5, 5, 4, 2, 1, 1, 4, 4, 4, (2, 2)),     # Line end
    Cfg(5, 3, 1, 64, 2, 1, 0, 0, 1, (0, 1)),    # Char conv_1
)


def r16(a):
    return np.asarray(a, dtype=np.float64).astype(np.float16).astype(np.float64)


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def make_dims(n, h, w, kh, kw, cin, cout, sh, sw, ph, pw):
    oh, ow = O.conv2d_out_hw(h, w, (kh, kw), (sh, sw), (ph, pw))
    return Dims(n, h, w, cin, cout, kh, kw, sh, sw, ph, pw, oh, ow)


# ---- the two ladders (Python copies of conv_api.hip and of uocr_conv_*_fast in conv_fast.hip) ---------------------------
def table_cfg(d):
    for cfg in TABLE:
        if (d.kh, d.kw, d.cin, d.cout, d.sh, d.sw) == cfg[:6]:
            return cfg
    return None


def _same5x5(d):
    return (d.kh, d.kw, d.sh, d.sw, d.ph, d.pw) == (5, 5, 1, 1, 2, 2) and d.oh == d.h and d.ow == d.w


def _half5x5(d):
    return (d.kh, d.kw, d.sh, d.sw, d.ph, d.pw) == (5, 5, 2, 2, 2, 2) and d.oh == (d.h + 1) // 2 and d.ow == (d.w + 1) // 2


def _c16_same(d, cin, cout):
    return (d.kh, d.kw, d.cin, d.cout, d.sh, d.sw) == (3, 3, cin, cout, 1, 1) and d.oh == d.h and d.ow == d.w


def _mfma(d, which, opt):
    if opt == 0 or d.cout % 4 or d.cin % 4 or (which == 0 and d.cin % 32) or (which == 1 and d.cout % 32):
        return False
    return opt == 2 or (d.cin >= 16 and d.cout >= 16)


def expect_kernel(entry, dtype, d, pad_value=0.0, opts=None, aligned=True):
    """name of the kernel family (KERNELS) the library chooses for a uocr_conv2d_* call under `opts`, in the default
    build (t32: bit 2 only, no h3); aligned: every activation pointer of the call is 16-byte (binary16: 8-byte) aligned"""
    o = dict(DEFAULTS)
    o.update(opts or {})
    is32, is16 = dtype == 'float32', dtype == 'float16'
    fast = bool(o['fast_paths']) and aligned
    ch = (d.cin, d.cout)
    if entry in (FWD, DGRAD):
        if is16 and fast and o['h16'] and d.n <= 65535:
            if _same5x5(d) and (ch in ((4, 2), (4, 4)) or (ch == (1, 1) and entry == FWD)):
                return 'h16'
            if _half5x5(d) and (ch == (4, 4) or (ch == (1, 4) and entry == DGRAD)):
                return 'h16'
        if is32 and fast and d.n <= 65535 and _same5x5(d):
            built = o['t32'] & 2
            if (ch in ((4, 2), (4, 4)) and built & (1 << entry)) or (ch == (1, 1) and built & (8 << entry)):
                return 't32'
    if entry == FWD and (is32 or is16) and fast and o['tiled'] and (d.kh, d.kw, d.cin, d.sh, d.sw) == (5, 5, 4, 1, 1) \
            and d.cout in (2, 4) and d.oh == d.h and d.ow == d.w:
        return 'tiled'
    if entry == WGRAD and is16 and fast and o['h16']:
        if _same5x5(d) and ch in ((4, 2), (1, 1)):
            return 'h16_wgrad'
        if _half5x5(d) and ch in ((4, 4), (1, 4), (1, 1)):
            return 'h16_wgrad_s2'
    cfg = table_cfg(d)
    if (is32 or is16) and fast and cfg is not None:
        s2p2 = (d.kh, d.kw, d.sh, d.sw, d.ph, d.pw) == (5, 5, 2, 2, 2, 2)
        if entry == FWD:
            if is32 and _c16_same(d, 1, 16):
                return 'c16_expand'
            if is32 and _c16_same(d, 16, 1):
                return 'c16_reduce'
            return 'table_px' if cfg.fpx else 'table_fast'
        if entry == DGRAD:
            if is32 and _c16_same(d, 16, 1):
                return 'c16_expand'
            if is32 and _c16_same(d, 1, 16):
                return 'c16_reduce'
            if is32 and (d.kh, d.kw, d.sh, d.sw, d.ph, d.pw) == (5, 3, 2, 1, 0, 1) and ch == (1, 64) and d.h <= 65535 \
                    and d.n <= 65535:
                return 'dgrad_c64s2'
            if s2p2 and ch in ((1, 1), (1, 4), (4, 4)):
                return 'dgrad_s2'
            return 'table_px' if cfg.dpx else 'table_fast'
        if is32 and _c16_same(d, 16, 1) and pad_value == 0.0:
            return 'c16_wgrad'
        if s2p2 and o['tiled'] == 1 and ch == (1, 4):
            return 'wgrad_s2_tiled'
        if (d.kh, d.kw, d.sh, d.sw, d.ph, d.pw) == (5, 5, 1, 1, 2, 2) and ch == (4, 2):
            return 'wgrad_t542'
        return 'table_fast'
    if is32 and _mfma(d, entry, o['mfma']):
        return 'mfma'
    return 'generic'


def branches(entry, dtype, d, pad_value=0.0, opts=None):
    """Which side of the padding-dependent branches a TABLE kernel takes for this call: {'row4': the aligned float4 row
    path of load_row_c1 (None: the instantiation has none), 'packed': the packed store (None: it has none), 'deep': some
    window lies wholly in the border (padding >= K)}; None when another kernel takes the call."""
    k = expect_kernel(entry, dtype, d, pad_value, opts)
    if k not in ('table_fast', 'table_px'):
        return None
    cfg = table_cfg(d)
    row4 = packed = None
    if entry == FWD and cfg.fpx:
        if d.cin == 1 and cfg.fpx % 4 == 0:
            row4 = d.pw == d.kw // 2 and d.w % 4 == 0
        if d.cout == 1 and cfg.fpx % 4 == 0:
            packed = d.ow % cfg.fpx == 0
    elif entry == DGRAD and cfg.dpx:
        if d.cout == 1 and cfg.dpx % 4 == 0:
            row4 = d.pw == d.kw // 2 and d.ow % 4 == 0
        if d.cin == 1 and cfg.dpx % 4 == 0:
            packed = d.w % cfg.dpx == 0
    elif entry == WGRAD and d.cin == 1 and cfg.wpx % 4 == 0:
        row4 = d.pw == d.kw // 2 and d.w % 4 == 0
    return dict(row4=row4, packed=packed, deep=d.ph >= d.kh or d.pw >= d.kw)


# ---- cases ---------------------------------------------------------------------------------------------------------------
SIZES = ((2, 27, 72), (3, 18, 44), (2, 21, 37))
PAD_VALUES = (0.0, 0.75)
ACTS = (None, 'relu', 'leaky', 'sigmoid')
MASKS = (None, 'leaky', 'sigmoid')
ALPHA = 0.01


def paddings(cfg):
    """the net's own; none; one component K/2 (both orders); neither K/2; K - 1; >= K"""
    kh, kw = cfg.kh, cfg.kw
    neither = (0, 2) if (kh, kw) == (3, 3) else (1, 3) if (kh, kw) == (5, 5) else (1, 2)
    out = [cfg.net_pad, (0, 0), (0, kw // 2), (kh // 2, 0), (kh // 2, kw // 2), neither, (kh - 1, kw - 1), (kh + 1, kw)]
    return tuple(dict.fromkeys(out))            # (the net's own may be one of them: kept once, order kept)


def option_sets(dtype, cfg, pad):
    """at the net's padding: also the options that take the shadowing kernels away"""
    if pad != cfg.net_pad:
        return ({},)
    if dtype == 'float32':
        return ({}, {'t32': 0, 'tiled': 0})
    return ({}, {'h16': 0}, {'h16': 0, 'tiled': 0})


Case = namedtuple('Case', 'dtype cfg d pad_value bias act mask opts seed_base aligned', defaults=(True,))
GROUPS = []                                     # (id, cases): one configuration, dtype, padding and option set
for _ci, _cfg in enumerate(TABLE):
    for _dtype in ('float32', 'float16'):
        for _pi, _pad in enumerate(paddings(_cfg)):
            for _oi, _opts in enumerate(option_sets(_dtype, _cfg, _pad)):
                _cases = []
                for _k, ((_n, _h, _w), _pv) in enumerate(itertools.product(SIZES, PAD_VALUES)):
                    _d = make_dims(_n, _h, _w, *_cfg[:6], *_pad)
                    if _d.oh <= 0 or _d.ow <= 0:
                        continue                # (an empty output: the host layer refuses it)
                    _r = _k + _pi + _oi
                    _cases.append(Case(_dtype, _cfg, _d, _pv, _r % 2 == 0, ACTS[_r % 4], MASKS[_r % 3], _opts,
                                       1000000 + 32 * (len(GROUPS) * 8 + _k)))
                _name = f"{_dtype[5:]}-{_cfg.kh}x{_cfg.kw}-{_cfg.cin}to{_cfg.cout}-s{_cfg.sh}{_cfg.sw}-p{_pad[0]}_{_pad[1]}" + \
                        ''.join(f'-{k}{v}' for k, v in _opts.items())
                GROUPS.append((_name, tuple(_cases)))
GROUP_IDS = [name for name, _ in GROUPS]


def all_cases():
    return [c for _, cases in GROUPS for c in cases]


def case_id(c):
    d = c.d
    return f"{c.dtype[5:]} {d.n}x{d.h}x{d.w}x{d.cin}->{d.cout} {d.kh}x{d.kw} s{d.sh}{d.sw} p{d.ph},{d.pw} pv{c.pad_value:g} " \
           f"bias{int(c.bias)} act={c.act} mask={c.mask} {c.opts or ''}"


def kernels_of(c):
    return tuple(expect_kernel(e, c.dtype, c.d, c.pad_value, c.opts, c.aligned) for e in (FWD, DGRAD, WGRAD))


# ---- inputs, the oracle and its float32 restatement ----------------------------------------------------------------------
def act_ref(y, act):
    if act == 'relu':
        return O.relu_fwd(y)
    if act == 'leaky':
        return O.leaky_relu_fwd(y, ALPHA)
    if act == 'sigmoid':
        return O.sigmoid_fwd(y)
    return y


def mask_factor(m, mask):
    if mask == 'leaky':
        return np.where(m >= 0, 1.0, ALPHA)
    if mask == 'sigmoid':
        return m * (1 - m)
    return np.ones_like(m)


def draw(c, seed):
    """Seeded inputs as the existing conv tests draw them (dy with mean 0.5: module docstring), and the operands the
    oracle sees: binary16 mode rounds x / dy / the mask tensor to binary16 and the parameters to float32."""
    d = c.d
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((d.n, d.h, d.w, d.cin))
    w = rng.standard_normal((d.kh, d.kw, d.cin, d.cout)) * 0.2
    b = rng.standard_normal(d.cout)
    g = rng.standard_normal((d.n, d.oh, d.ow, d.cout)) + 0.5
    if c.mask == 'sigmoid':                     # an activation OUTPUT: inside (0, 1)
        m = rng.uniform(0.05, 0.95, x.shape)
    else:                                       # signs independent of x, no zero
        m = np.where(rng.random(x.shape) < 0.5, -1.0, 1.0) * (np.abs(x) + 0.01)
    raw = dict(x=x, w=w, b=b, g=g, m=m)
    if c.dtype == 'float16':
        return raw, dict(x=r16(x), w=f32(w), b=f32(b), g=r16(g), m=r16(m))
    return raw, dict(raw)


def reference(c, o, dt=np.float64):
    """every output of the case from the oracle's code in `dt` arithmetic"""
    kf, kd, _ = kernels_of(c)
    st, pd = (c.d.sh, c.d.sw), (c.d.ph, c.d.pw)
    half = c.dtype == 'float16'
    x, b, g, m = (o[k].astype(dt) for k in ('x', 'b', 'g', 'm'))
    # the conv_h16 kernels take the float32 master weights into the matrix cores rounded to binary16
    w_f = (r16(o['w']) if half and kf == 'h16' else o['w']).astype(dt)
    w_d = (r16(o['w']) if half and kd == 'h16' else o['w']).astype(dt)
    y = O.conv2d_fwd(x, w_f, b, st, pd, dt(c.pad_value), c.bias)
    dx, dw, db = O.conv2d_bwd(x, w_d, g, st, pd, dt(c.pad_value), c.bias)
    k = dt(2.0 ** GSCALE if half else 1.0)
    dw, db = dw / k, db / k
    return dict(y=y, y_act=act_ref(y, c.act), dx=dx, dx_mask=dx * mask_factor(m, c.mask).astype(dt),
                dw_acc=dw + dt(ACC_INIT[0]), db_acc=db + dt(ACC_INIT[1]), dw=dw, db=db)


def tolerances(c):
    if c.dtype == 'float16':
        return dict(y=TOL_STORE, y_act=TOL_STORE, dx=TOL_STORE, dx_mask=TOL_STORE, dw_acc=TOL_EXACT, db_acc=TOL_EXACT,
                    dw=TOL_EXACT, db=TOL_EXACT)
    return dict(y=TOL_Y32, y_act=TOL_Y32, dx=TOL_Y32, dx_mask=TOL_Y32, dw_acc=TOL_G32, db_acc=TOL_G32, dw=TOL_G32,
                db=TOL_G32)


def qualified(c):
    """(seed, raw inputs, float64 reference) of the first seed whose float32 restatement stays within a quarter of
    every tolerance (module docstring), or (None, worst ratios, None)"""
    tol = tolerances(c)
    worst = {}
    for seed in range(c.seed_base, c.seed_base + SEEDS):
        raw, o = draw(c, seed)
        ref = reference(c, o)
        low = reference(c, o, np.float32)
        ratio = {k: rel_linf(low[k], ref[k]) / tol[k] for k in tol}
        if max(ratio.values()) <= 0.25:
            return seed, raw, ref
        worst = ratio
    return None, worst, None


# ---- CPU-only checks -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('part', range(8))
def test_every_case_has_a_qualifying_seed(part):
    """The seed search of the module docstring for every case (in eight parts), on the oracle alone."""
    missing = []
    for c in all_cases()[part::8]:
        seed, worst, _ = qualified(c)
        if seed is None:
            missing.append((case_id(c), worst))
    assert not missing, f'no qualifying seed among {SEEDS}: {missing}'


def test_ladder_copy_on_known_shapes():
    """`expect_kernel` on shapes whose kernel the comments of conv_api.hip / conv_fast.hip state."""
    def k(entry, dtype, shape, pad, pv=0.0, opts=None, aligned=True):
        return expect_kernel(entry, dtype, make_dims(*shape, *pad), pv, opts, aligned)
    # (n, h, w, kh, kw, cin, cout, sh, sw)
    line_end, line_up, para, down1 = (2, 40, 72, 5, 5, 4, 2, 1, 1), (2, 40, 72, 5, 5, 4, 4, 1, 1), \
        (2, 40, 72, 5, 5, 1, 1, 1, 1), (2, 40, 72, 5, 5, 1, 4, 2, 2)
    mono1, mono2, char1 = (2, 21, 35, 3, 3, 1, 16, 1, 1), (2, 21, 35, 3, 3, 16, 1, 1, 1), (2, 32, 70, 5, 3, 1, 64, 2, 1)
    # the nets' own padding: the shadowing kernels
    assert [k(e, 'float32', line_end, (2, 2)) for e in (0, 1, 2)] == ['tiled', 't32', 'wgrad_t542']
    assert [k(e, 'float16', line_end, (2, 2)) for e in (0, 1, 2)] == ['h16', 'h16', 'h16_wgrad']
    assert [k(e, 'float16', line_end, (2, 2), opts={'h16': 0}) for e in (0, 1, 2)] == ['tiled', 'table_px', 'wgrad_t542']
    assert [k(e, 'float32', line_up, (2, 2), opts={'t32': 0, 'tiled': 0}) for e in (0, 1, 2)] == ['table_px'] * 2 + ['table_fast']
    assert [k(e, 'float32', para, (2, 2)) for e in (0, 1, 2)] == ['table_px', 'table_px', 'table_fast']
    assert [k(e, 'float16', para, (2, 2)) for e in (0, 1, 2)] == ['h16', 'table_px', 'h16_wgrad']
    assert [k(e, 'float32', down1, (2, 2)) for e in (0, 1, 2)] == ['table_px', 'dgrad_s2', 'wgrad_s2_tiled']
    assert [k(e, 'float16', down1, (2, 2)) for e in (0, 1, 2)] == ['table_px', 'h16', 'h16_wgrad_s2']
    assert [k(e, 'float32', mono1, (1, 1)) for e in (0, 1, 2)] == ['c16_expand', 'c16_reduce', 'table_fast']
    assert [k(e, 'float32', mono2, (1, 1)) for e in (0, 1, 2)] == ['c16_reduce', 'c16_expand', 'c16_wgrad']
    assert k(2, 'float32', mono2, (1, 1), pv=0.5) == 'table_fast'        # conv_c16_wgrad needs a zero padding value
    assert [k(e, 'float16', mono2, (1, 1)) for e in (0, 1, 2)] == ['table_px', 'table_px', 'table_fast']
    assert [k(e, 'float32', char1, (0, 1)) for e in (0, 1, 2)] == ['table_fast', 'dgrad_c64s2', 'table_fast']
    # any other padding: the table kernels, whatever the options
    for shape in (line_end, line_up, para, down1, mono1, mono2, char1):
        for dtype in ('float32', 'float16'):
            got = [k(e, dtype, shape, (0, 0)) for e in (0, 1, 2)]
            assert set(got) <= {'table_fast', 'table_px'} and got[2] == 'table_fast', (shape, dtype, got)
    assert [k(e, 'float32', mono1, (0, 1)) for e in (0, 1, 2)] == ['table_fast', 'table_px', 'table_fast']
    assert [k(e, 'float32', char1, (2, 1)) for e in (0, 1, 2)] == ['table_fast'] * 3
    # off the table, an unaligned pointer, fast paths off: the generic kernels; 64 channels: the MFMA GEMM
    assert k(0, 'float32', (2, 40, 72, 5, 5, 4, 4, 1, 2), (2, 2)) == 'generic'
    assert k(0, 'float32', line_up, (2, 2), aligned=False) == k(1, 'float32', para, (0, 0), opts={'fast_paths': 0}) == 'generic'
    assert [k(e, 'float32', (2, 14, 10, 5, 3, 64, 64, 2, 1), (0, 1)) for e in (0, 1, 2)] == ['mfma'] * 3
    assert k(2, 'float32', line_up, (2, 2), opts={'mfma': 2, 'fast_paths': 0}) == 'mfma'
    assert k(0, 'float64', line_up, (2, 2)) == 'generic'


def test_cases_reach_every_table_kernel_and_shadowed_kernel():
    """The case list under the ladder copy: every (entry, table configuration, dtype) runs its table kernel at a foreign
    padding; every shadowing kernel of the default library runs at the net's; every forward activation / dx mask meets
    every table forward / backward-data kernel in both dtypes."""
    table, other, acts, masks = set(), set(), set(), set()
    for c in all_cases():
        ci = TABLE.index(c.cfg)
        for e, k in enumerate(kernels_of(c)):
            if k in ('table_fast', 'table_px'):
                table.add((e, ci, c.dtype, k, (c.d.ph, c.d.pw) != c.cfg.net_pad))
                if e == FWD:
                    acts.add((ci, c.dtype, c.act))
                if e == DGRAD:
                    masks.add((ci, c.dtype, c.mask))
            else:
                other.add((e, k, c.dtype))
    for ci, cfg in enumerate(TABLE):
        for dtype in ('float32', 'float16'):
            want = {(FWD, ci, dtype, 'table_px' if cfg.fpx else 'table_fast', True),
                    (DGRAD, ci, dtype, 'table_px' if cfg.dpx else 'table_fast', True),
                    (WGRAD, ci, dtype, 'table_fast', True)}
            assert want <= table, (cfg, dtype, sorted(want - table))
            assert {(ci, dtype, a) for a in ACTS} <= acts, (cfg, dtype)
            assert {(ci, dtype, m) for m in MASKS} <= masks, (cfg, dtype)
    # float32 table kernels that only the options uncover at the net's padding (t32 = 0, tiled = 0), and the binary16 ones
    # of the 4-channel layers (h16 = 0)
    for e, ci, dtype in ((DGRAD, 6, 'float32'), (DGRAD, 7, 'float32'), (WGRAD, 4, 'float32'), (FWD, 6, 'float32'),
                         (FWD, 7, 'float32'), (FWD, 6, 'float16'), (DGRAD, 6, 'float16'), (DGRAD, 7, 'float16'),
                         (WGRAD, 4, 'float16'), (WGRAD, 5, 'float16')):
        assert any(t[:3] == (e, ci, dtype) and not t[4] for t in table), (e, ci, dtype)
    want = {(FWD, 'c16_expand', 'float32'), (DGRAD, 'c16_expand', 'float32'), (FWD, 'c16_reduce', 'float32'),
            (DGRAD, 'c16_reduce', 'float32'), (WGRAD, 'c16_wgrad', 'float32'), (DGRAD, 'dgrad_s2', 'float32'),
            (DGRAD, 'dgrad_s2', 'float16'), (DGRAD, 'dgrad_c64s2', 'float32'), (WGRAD, 'wgrad_t542', 'float32'),
            (WGRAD, 'wgrad_t542', 'float16'), (WGRAD, 'wgrad_s2_tiled', 'float32'), (WGRAD, 'wgrad_s2_tiled', 'float16'),
            (FWD, 'tiled', 'float32'), (FWD, 'tiled', 'float16'), (DGRAD, 't32', 'float32'), (FWD, 'h16', 'float16'),
            (DGRAD, 'h16', 'float16'), (WGRAD, 'h16_wgrad', 'float16'), (WGRAD, 'h16_wgrad_s2', 'float16')}
    assert want <= other, sorted(want - other)
    assert not any(k in ('generic', 'mfma', 'h3', 't32_wgrad') for _, k, _ in other), sorted(other)


def test_cases_reach_both_sides_of_the_padding_dependent_branches():
    """Per (entry, configuration, dtype) that has the branch: the float4 row path taken (also under ph != KH / 2) and
    not taken (also at w % 4 == 0, i.e. because of pw alone); the packed store taken and not taken at w % 4 == 0; windows
    wholly in the border with a non-zero padding value."""
    seen = {}
    for c in all_cases():
        for e in (FWD, DGRAD, WGRAD):
            br = branches(e, c.dtype, c.d, c.pad_value, c.opts)
            if br is None:
                continue
            s = seen.setdefault((e, TABLE.index(c.cfg), c.dtype), set())
            if br['row4'] is not None:
                s.add(('row4', br['row4'], c.d.ph != c.cfg.kh // 2 if br['row4'] else c.d.w % 4 == 0))
            if br['packed'] is not None:
                s.add(('packed', br['packed'], c.d.w % 4 == 0))
            if br['deep']:
                s.add(('deep', c.pad_value != 0.0))
    has_row4 = {(FWD, 2), (FWD, 3), (FWD, 4), (DGRAD, 3), (WGRAD, 2), (WGRAD, 3)}
    has_packed = {(FWD, 1), (FWD, 2), (FWD, 3), (DGRAD, 0), (DGRAD, 3)}
    for e in (FWD, DGRAD, WGRAD):
        for ci in range(len(TABLE)):
            for dtype in ('float32', 'float16'):
                s = seen[(e, ci, dtype)]
                assert {('deep', True), ('deep', False)} <= s, (e, ci, dtype)
                assert ((e, ci) in has_row4) == any(t[0] == 'row4' for t in s), (e, ci)
                assert ((e, ci) in has_packed) == any(t[0] == 'packed' for t in s), (e, ci)
                if (e, ci) in has_row4:
                    assert {('row4', True, True), ('row4', True, False), ('row4', False, True), ('row4', False, False)} <= s, \
                        (e, ci, dtype, sorted(s))
                if (e, ci) in has_packed:           # (3 x 3 1 -> 16 dx packs four pixels: w % 4 alone decides)
                    want = {('packed', True, True), ('packed', False, False)} | \
                        ({('packed', False, True)} if (e, ci) != (DGRAD, 0) else set())
                    assert want <= s, (e, ci, dtype, sorted(s))


# ---- GPU side ------------------------------------------------------------------------------------------------------------
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


class Checker:
    """prints every figure, collects the misses: a group reports all of its cases before it fails"""

    def __init__(self):
        self.failures = []

    def close(self, what, a, ref, tol):
        from univer_ocr_amd.nn import CP
        err = rel_linf(CP.asnumpy(a), ref)
        print(f'    {what}: rel_linf {err:.3e} (bound {tol:.1e})')
        if not err <= tol:
            self.failures.append(f'{what}: rel_linf={err:.3e} > {tol:.1e}')

    def kernel(self, what, rt, entry, name):
        got = rt.last_conv()
        print(f'    {what}: last_conv {got} = {KERNELS[got[1]]}')
        if got != (entry, KID[name]):
            self.failures.append(f'{what}: last_conv {got} ({KERNELS[got[1]]}) != ladder copy {(entry, KID[name])} ({name})')


def run_case(CP, c, chk, vs_generic=False):
    """One case: forward (plain, then with its activation), backward-data (plain, then masked), backward-weight
    (accumulating, then overwriting); `last_conv` after every launch."""
    from univer_ocr_amd.nn import ops
    seed, raw, ref = qualified(c)
    assert seed is not None, f'{case_id(c)}: no qualifying seed among {SEEDS}: {raw}'
    what = f'{case_id(c)} seed {seed}'
    print(f'  {what}')
    rt = CP.runtime()
    for key, value in DEFAULTS:
        rt.set_option(key, c.opts.get(key, value))
    half = c.dtype == 'float16'
    CP.set_dtype(c.dtype)
    tol = tolerances(c)
    kf, kd, kw = kernels_of(c)
    d, st, pd = c.d, (c.d.sh, c.d.sw), (c.d.ph, c.d.pw)
    xd, gd, md = CP.copy(raw['x']), CP.copy(raw['g']), CP.copy(raw['m'])
    wd, bd = CP.copy(raw['w'], np.float32), CP.copy(raw['b'], np.float32)
    if half:
        gd.gscale = GSCALE
    store = np.float16 if half else np.float32
    y = ops.conv2d_fwd(xd, wd, bd, st, pd, c.pad_value, c.bias)
    chk.kernel(f'{what}: fwd', rt, FWD, kf)
    chk.close(f'{what}: y', y, ref['y'], tol['y'])
    assert y.dtype == store and y.shape == (d.n, d.oh, d.ow, d.cout)
    if c.act is not None:
        ya = ops.conv2d_fwd(xd, wd, bd, st, pd, c.pad_value, c.bias, act=c.act, alpha=ALPHA)
        chk.kernel(f'{what}: fwd {c.act}', rt, FWD, kf)
        chk.close(f'{what}: {c.act}(y)', ya, ref['y_act'], tol['y_act'])
    if vs_generic:
        rt.set_option('fast_paths', 0)
        yg = ops.conv2d_fwd(xd, wd, bd, st, pd, c.pad_value, c.bias)
        chk.kernel(f'{what}: fwd, fast_paths = 0', rt, FWD, 'generic')
        rt.set_option('fast_paths', 1)
        chk.close(f'{what}: y against the generic kernel', y, CP.asnumpy(yg).astype(np.float64), TOL_Y32)
    dx = ops.conv2d_bwd_data(gd, wd, xd.shape, st, pd)
    chk.kernel(f'{what}: dgrad', rt, DGRAD, kd)
    chk.close(f'{what}: dx', dx, ref['dx'], tol['dx'])
    assert dx.dtype == store and (not half or dx.gscale == GSCALE)
    if c.mask is not None:
        dxm = ops.conv2d_bwd_data(gd, wd, xd.shape, st, pd, x_act=md, act=c.mask, alpha=ALPHA)
        chk.kernel(f'{what}: dgrad {c.mask} mask', rt, DGRAD, kd)
        chk.close(f'{what}: dx * {c.mask} mask', dxm, ref['dx_mask'], tol['dx_mask'])
    for accumulate, init, names in ((True, ACC_INIT, ('dw_acc', 'db_acc')), (False, OVER_INIT, ('dw', 'db'))):
        dw, db = CP.full(raw['w'].shape, init[0], np.float32), CP.full(raw['b'].shape, init[1], np.float32)
        ops.conv2d_bwd_weight(xd, gd, dw, db, st, pd, c.pad_value, c.bias, accumulate=accumulate)
        chk.kernel(f'{what}: wgrad accumulate={accumulate}', rt, WGRAD, kw)
        chk.close(f'{what}: {names[0]}', dw, ref[names[0]], tol[names[0]])
        if c.bias:
            chk.close(f'{what}: {names[1]}', db, ref[names[1]], tol[names[1]])
        else:                                   # a switched-off bias: unchanged when accumulating, 0 when overwriting
            chk.close(f'{what}: {names[1]} (no bias)', db, np.full(d.cout, init[1] if accumulate else 0.0), 0.0)


@pytest.mark.gpu
def test_last_conv_is_zero_before_the_first_conv():
    """A fresh context of its own reports (0, 0)."""
    import ctypes as C
    from univer_ocr_amd.hip import lib as hiplib
    lib = hiplib.get_lib()
    handle = C.c_void_p()
    assert lib.uocr_ctx_create(0, 0, C.byref(handle)) == 0
    try:
        entry, kernel = C.c_int(-1), C.c_int(-1)
        assert lib.uocr_ctx_last_conv(handle, C.byref(entry), C.byref(kernel)) == 0
        assert (entry.value, kernel.value) == (0, 0)
        assert lib.uocr_ctx_last_conv(handle, None, C.byref(kernel)) != 0        # (a null pointer is refused)
    finally:
        lib.uocr_ctx_destroy(handle)
    assert hiplib.CONV_KERNELS == KERNELS


@pytest.mark.gpu
@pytest.mark.parametrize('index', range(len(GROUPS)), ids=GROUP_IDS)
def test_table_kernels_against_oracle(index, ctx):
    """One configuration, dtype, padding and option set: three sizes x two padding values, every output against the
    oracle, the kernel of every launch against the ladder copy; the first float32 case also against the generic kernel."""
    chk = Checker()
    for k, c in enumerate(GROUPS[index][1]):
        run_case(ctx, c, chk, vs_generic=k == 0 and c.dtype == 'float32')
    assert not chk.failures, '\n'.join(chk.failures)


@pytest.mark.gpu
def test_refused_call_leaves_last_conv(ctx):
    """An activation code outside the enum is refused before the dispatch: last_conv keeps the previous call's."""
    from univer_ocr_amd.hip.lib import HipError
    from univer_ocr_amd.nn import ops
    CP = ctx
    rt = CP.runtime()
    x, g = CP.copy(np.full((2, 9, 12, 1), 0.5)), CP.copy(np.full((2, 5, 8, 1), 0.5))
    w, b = CP.copy(np.full((5, 5, 1, 1), 0.1)), CP.copy(np.full((1,), 0.1))
    ops.conv2d_bwd_data(g, w, x.shape, (1, 1), (0, 0))
    before = rt.last_conv()
    assert before == (DGRAD, KID['table_px'])
    y = CP.empty((2, 5, 8, 1))
    dims = make_dims(2, 9, 12, 5, 5, 1, 1, 1, 1, 0, 0)
    with pytest.raises(HipError, match='act'):
        rt.call('uocr_conv2d_fwd', x.code, x.ptr, w.ptr, b.ptr, y.ptr, *dims, 0.0, 1, 9, 0.0)
    with pytest.raises(HipError, match='oh'):
        rt.call('uocr_conv2d_bwd_weight', x.code, x.ptr, g.ptr, w.ptr, b.ptr, *dims._replace(oh=6), 0.0, 1, 0)
    assert rt.last_conv() == before


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['float32', 'float16'])
def test_deferred_weight_gradient_notes_its_kernel(dtype, ctx):
    """Inside a deferred weight-gradient group the table kernel's finish is only recorded: the call still notes its
    kernel, and dw / db are right after the flush (Line end at padding (0, 0) and, conv_wgrad_t542, at the net's)."""
    from univer_ocr_amd.nn import ops
    CP = ctx
    rt = CP.runtime()
    chk = Checker()
    for pad, opts, name in (((0, 0), {}, 'table_fast'), ((2, 2), {'h16': 0}, 'wgrad_t542')):
        c = Case(dtype, TABLE[7], make_dims(2, 27, 72, *TABLE[7][:6], *pad), 0.75, True, None, None, opts, 3000000)
        assert kernels_of(c)[2] == name
        seed, raw, ref = qualified(c)
        assert seed is not None
        for key, value in DEFAULTS:
            rt.set_option(key, opts.get(key, value))
        CP.set_dtype(dtype)
        xd, gd = CP.copy(raw['x']), CP.copy(raw['g'])
        if dtype == 'float16':
            gd.gscale = GSCALE
        dw, db = CP.full(raw['w'].shape, ACC_INIT[0], np.float32), CP.full(raw['b'].shape, ACC_INIT[1], np.float32)
        with rt.defer_wgrad():
            ops.conv2d_bwd_weight(xd, gd, dw, db, (1, 1), pad, 0.75, True, accumulate=True)
            chk.kernel(f'deferred {case_id(c)}', rt, WGRAD, name)
        tol = tolerances(c)
        chk.close('dw after the flush', dw, ref['dw_acc'], tol['dw_acc'])
        chk.close('db after the flush', db, ref['db_acc'], tol['db_acc'])
    assert not chk.failures, '\n'.join(chk.failures)


UNALIGNED = ((6, (2, 2)), (3, (0, 2)), (5, (1, 3)))      # (TABLE index, padding): Line up at the net's padding, two foreign


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['float32', 'float16'])
@pytest.mark.parametrize('which', range(len(UNALIGNED)))
def test_unaligned_pointers_fall_to_the_generic_kernel(which, dtype, ctx):
    """Direct calls with ONE activation pointer moved by one element (a view into a larger allocation: x of the forward,
    dx of the backward-data, dy of the backward-weight): no vector kernel may take the call."""
    from univer_ocr_amd.nn import gpu
    CP = ctx
    rt = CP.runtime()
    ci, pad = UNALIGNED[which]
    c = Case(dtype, TABLE[ci], make_dims(2, 21, 40, *TABLE[ci][:6], *pad), 0.75, True, None, None, {}, 4000000 + 32 * which,
             aligned=False)
    assert kernels_of(c) == ('generic',) * 3
    seed, raw, ref = qualified(c)
    assert seed is not None
    CP.set_dtype(dtype)
    half = dtype == 'float16'
    d, tol = c.d, tolerances(c)

    def shifted(host):
        """a device copy of `host` that starts one element into its allocation (NaN on either side)"""
        flat = np.concatenate(([np.nan], np.asarray(host, dtype=np.float64).ravel(), [np.nan] * 7))
        big = CP.copy(flat)
        view = gpu.DeviceArray(big.t[1:1 + host.size].view(*host.shape))
        assert view.ptr % (8 if half else 16) != 0 and view.ptr == big.ptr + big.t.element_size()
        return big, view

    chk = Checker()
    code = CP.copy(raw['x']).code
    gcode = code | (GSCALE << 8) if half else code
    wd, bd = CP.copy(raw['w'], np.float32), CP.copy(raw['b'], np.float32)
    # forward: x unaligned
    _, xv = shifted(raw['x'])
    y = CP.empty(ref['y'].shape)
    rt.call('uocr_conv2d_fwd', code, xv.ptr, wd.ptr, bd.ptr, y.ptr, *d, c.pad_value, 1, 0, 0.0)
    chk.kernel('fwd, x + 1', rt, FWD, 'generic')
    chk.close('y', y, ref['y'], tol['y'])
    # backward-data: dx unaligned (its neighbours in the allocation must stay NaN)
    gd = CP.copy(raw['g'])
    big, dxv = shifted(np.zeros(raw['x'].shape))
    rt.call('uocr_conv2d_bwd_data', gcode, gd.ptr, wd.ptr, dxv.ptr, *d, None, 0, 0.0)
    chk.kernel('dgrad, dx + 1', rt, DGRAD, 'generic')
    chk.close('dx', dxv, ref['dx'], tol['dx'])
    host = CP.asnumpy(big)
    assert np.isnan(host[0]) and np.all(np.isnan(host[1 + raw['x'].size:]))
    # backward-weight: dy unaligned
    xd = CP.copy(raw['x'])
    _, gv = shifted(raw['g'])
    dw, db = CP.full(raw['w'].shape, ACC_INIT[0], np.float32), CP.full(raw['b'].shape, ACC_INIT[1], np.float32)
    rt.call('uocr_conv2d_bwd_weight', gcode, xd.ptr, gv.ptr, dw.ptr, db.ptr, *d, c.pad_value, 1, 1)
    chk.kernel('wgrad, dy + 1', rt, WGRAD, 'generic')
    chk.close('dw', dw, ref['dw_acc'], tol['dw_acc'])
    chk.close('db', db, ref['db_acc'], tol['db_acc'])
    assert not chk.failures, '\n'.join(chk.failures)
