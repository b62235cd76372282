"""Every launch form of the conv-pair strip kernels (uocr_conv_pair_fwd / _bwd; conv_pair_strip.hip float32,
conv_pair_strip_h.hip binary16) against the float64 oracle run layer by layer.

What selects the code of these kernels is mostly the page WIDTH: waves per cooperative block and the edge columns they
hand each other, the unmasked MODE 0 (w == 64 * waves, zero padding value), overlapping column blocks past 512
columns, binary16 strips of 64 columns every 62 with four strips per block, the cooperative / independent-wave
binary16 backward.  Then the rows (steps in batches of three, bands raised to four rows, one recomputed row between
bands), the flags, and the options "pair_g" / "pair_pf" that pick other instantiations.  The sections below sweep each
of them; after every launch `Runtime.last_pair` (uocr_ctx_last_pair) must report what a Python copy of the host rules
(`expect_pair`) expects, so that a forced option that does nothing cannot pass unnoticed, and a CPU-only check
(`test_shapes_reach_every_form`) keeps a later edit of a shape list from emptying a class.

References and tolerances are the project's own: float32 exactly as test_gpu_kernels.test_conv_pair_kernels_against_oracle
(y 1e-5, dx / dw / db 2e-5); binary16 as checker (1) of test_gpu_f16.test_conv_pair_f16 -- the oracle with the kernels'
operand roundings (weights, a1, d_a1 to binary16), the backward from the STORED y -- stored tensors 1e-3, dw1 / dw2 /
db2 2e-4, db1 4e-3; all rel_linf.  Every array the ops allocate starts as NaN.

Well-posedness.  The backward is discontinuous in z1, the pre-activation of conv_1: where the kernel's float32 z1 and
the oracle's float64 z1 differ in sign, the LeakyReLU slope flips between 1 and alpha, and dx and the gradients move by
far more than any tolerance.  With up to ~4 x 10^6 values of z1 per case and several hundred cases this happens for
some seed.  So every case draws its inputs from the first seed of base, base + 1, ..., base + 19 for which the ORACLE
has no position with |z1| < 2^-20 * (sum_k |x_k w1_k| + |b1|).  The bound exceeds the worst-case error of the
kernel's z1: float32 rounding of the 10-term sum (10 * 2^-24 of that quantity) plus, in float32 mode, the rounding of
the float64 inputs to float32 (2 * 2^-24 more); in binary16 mode the rounded oracle has the kernel's operands exactly
and the sums are float32 on both sides.  It is derived, not tuned.  If none of the twenty seeds qualifies the test
fails; it never skips and never leaves a position out.  Not applied for alpha = 1 (no discontinuity).  The search
needs no GPU: `test_every_case_has_a_qualifying_seed` runs it for every parametrised case.  The expected number of
positions inside the bound is ~1.3e-6 per value of z1, i.e. ~5.5 for the 4.2 x 10^6 values of a benchmarked size: there
5 to 8 of 2000 seeds qualified, so the two cases of section 7 carry a `base` that an offline run of the same
search found (SEED_BASE); every other case takes its base from its position in the lists.

A second condition, also on the oracle alone, concerns the only ONE-element output.  rel_linf divides by max |expected|;
for db2 accumulated into 2.0 the expected value is 2.0 + db2, and a seed whose db2 is close to -2.0 turns the float32
rounding of the kernel's partial sums -- which is relative to the sum itself -- into an arbitrarily large relative
error (first GPU run of this module: float32 2 x 5 x 130, db2 = -2.0086, expected -0.0086, absolute error 2.7e-6 on a
sum of 1300 terms with sum |term| = 153: rel_linf 3.1e-4).  A seed is passed over when |2.0 + db2| < max(2.0, |db2|) / 4,
i.e. when cancellation would tighten the 2e-5 / 2e-4 of the existing tests by more than a factor 4.  The multi-element
outputs take their norm over 16 to 2 x 10^5 elements and need no such condition.
"""
import numpy as np
import pytest

from conftest import rel_linf
from oracle import nn_oracle as O

TOL_Y32, TOL_G32 = 1e-5, 2e-5                   # test_gpu_kernels.py
TOL_STORE, TOL_SUM16, TOL_DB1_16 = 1e-3, 2e-4, 4e-3   # test_gpu_f16.py, test_gpu_work_split.py
SEEDS = 20
DEFAULTS = (('pair_band', 0), ('pair_g', 4), ('pair_pf', -1), ('max_blocks', 0), ('wgrad_bands', 0), ('t32', 2),
            ('h16', 1), ('mfma', 1), ('fast_paths', 1), ('tiled', 1))
ACC_INIT = (0.5, 0.25, -0.5, 2.0)               # dw1, db1, dw2, db2 when accumulating (test_gpu_kernels.py)
OVER_INIT = (7.0, -3.0, 5.0, -1.0)              # ... and what an overwriting call must replace


def r16(a):
    return np.asarray(a, dtype=np.float64).astype(np.float16).astype(np.float64)


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def cdiv(a, b):
    return (a + b - 1) // b


# ---- the host rules (independent Python copies of pair_block_geometry, pair_bands_per_cu, pair_wave_geometry and
# pair_bands_rounds of conv_pair_strip.h, and of how the five launchers combine them) ------------------------------------
def block_geometry(w, g=4, max_waves=8):
    """cooperative block: waves, computed columns, column blocks (overlapping by two columns)"""
    cols = 16 * g
    nw = min(max_waves, cdiv(w, cols))
    bwc = nw * cols
    nbx = 1 if w <= bwc else 1 + cdiv(w - bwc, bwc - 2)
    return nw, bwc, nbx


def floor4_bands(h, bands, band_opt):
    """bands of the cooperative kernels: raised to 4 rows, never above h"""
    if band_opt > 0:
        bands = cdiv(h, band_opt)
    band_h = min(h, max(4, cdiv(h, bands)))
    return cdiv(h, band_h), band_h


def wave_geometry(w, g=4):
    """independent waves: strips of 16 g columns every 16 g - 2, four strips per block"""
    cols = 16 * g
    nstrips = 1 if w <= cols else 1 + cdiv(w - cols, cols - 2)
    nw = min(4, nstrips)
    return nstrips, nw, cdiv(nstrips, nw)


def wave_bands(n, h, blocks_x, resident, band_opt):
    """bands of the independent-wave kernels: whole rounds of what is resident at once"""
    bands, best = 1, 1e30
    for b in range(1, max(1, h // 8) + 1):
        bh = cdiv(h, b)
        blocks = blocks_x * cdiv(h, bh) * n
        cost = float(cdiv(blocks, resident) * (bh + 2))
        if cost < best * 0.999:
            best, bands = cost, cdiv(h, bh)
    if band_opt > 0:
        bands = cdiv(h, band_opt)
    band_h = cdiv(h, bands)
    return cdiv(h, band_h), band_h


def expect_pair(which, dtype, n, h, w, pad1, opts, cu):
    """((kernel, g, mode, pf, nw, blocks_x, bands, band_h), details) the host code chooses for the forward
    (`which` = 'fwd') or the backward ('bwd'); details: nbx / nstrips / live strips of the last block / rows of the
    last band.  Whether dx is wanted changes the kernel instantiation and the LDS size, none of these."""
    band, g_opt, pf_opt = opts.get('pair_band', 0), opts.get('pair_g', 4), opts.get('pair_pf', -1)
    det = {}
    if dtype == 'float32':
        g, max_waves = (2, 16) if which == 'bwd' and g_opt == 2 else (4, 8)
        nw, bwc, nbx = block_geometry(w, g, max_waves)
        mode = 0 if nbx == 1 and w == bwc and pad1 == 0.0 else 1
        per = cu if which == 'bwd' else 2 * cu
        bands, band_h = floor4_bands(h, max(1, cdiv(per, n * nbx)), band)
        pf = (0 if pf_opt == 0 else 2 if pf_opt == 2 else 1) if which == 'fwd' else 0
        out = (1 if which == 'fwd' else 2, g, mode, pf, nw, nbx, bands, band_h)
        det['nbx'] = nbx
    elif which == 'fwd':
        nstrips, nw, bx = wave_geometry(w)
        bands, band_h = wave_bands(n, h, bx, 4 * cu, band)
        out = (3, 4, 0, 0 if pf_opt == 0 else 1 if pf_opt == 1 else 2, nw, bx, bands, band_h)
        det.update(nstrips=nstrips, last_live=nstrips - 4 * (bx - 1))
    else:
        nw, bwc, _ = block_geometry(w)
        if w > bwc:
            g = 2 if g_opt == 2 else 4
            nstrips, nw, bx = wave_geometry(w, g)
            bands, band_h = wave_bands(n, h, bx, (2 if g == 4 else 4) * cu, band)
            out = (5, g, 0, 0, nw, bx, bands, band_h)
            det.update(nstrips=nstrips, last_live=nstrips - 4 * (bx - 1))
        else:
            bands, band_h = floor4_bands(h, max(1, cdiv(cu, n)), band)
            out = (4, 4, 0 if w == bwc and pad1 == 0.0 else 1, 0, nw, 1, bands, band_h)
    det['last_band'] = h - (out[6] - 1) * out[7]
    return out, det


# ---- cases ---------------------------------------------------------------------------------------------------------------
def case(dtype, n, h, w, pad1=0.0, bias1=True, bias2=True, sigmoid=True, alpha=0.01, need_dx=True, accumulate=True,
         gscale=6, deferred=False):
    return dict(dtype=dtype, n=n, h=h, w=w, pad1=pad1, bias1=bias1, bias2=bias2, sigmoid=sigmoid, alpha=alpha,
                need_dx=need_dx, accumulate=accumulate, gscale=gscale, deferred=deferred)


AUTO = ({},)

# 2. width sweep: n = 2, h = 7, auto bands; pad1 in {0, 0.25} because the mode depends on it
W32 = (1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193, 320, 383, 384, 385, 447, 448, 449, 511, 512, 513, 514,
       515, 575, 576, 577, 1021, 1022, 1023, 1024, 1531, 1532, 1533)
W16 = (1, 3, 63, 64, 65, 66, 126, 127, 128, 188, 189, 190, 250, 251, 252, 312, 313, 374, 375, 436, 437, 498, 499, 511,
       512, 513, 560, 561, 622, 623, 684, 685, 808, 809, 1024)
W16_PLAIN = (192, 256, 320, 384, 448)           # the unmasked cooperative backward with 3 - 7 waves (pad1 = 0 only)
WIDTHS = [('w32', case('float32', 2, 7, w, pad), AUTO) for w in W32 for pad in (0.0, 0.25)] + \
         [('w16', case('float16', 2, 7, w, pad), AUTO) for w in W16 for pad in (0.0, 0.25)] + \
         [('w16', case('float16', 2, 7, w, 0.0), AUTO) for w in W16_PLAIN] + \
         [('w16', case('float16', 2, 12, 2048, pad), AUTO) for pad in (0.0, 0.25)]     # the high-res page width

# 3. height x band sweep: one wave, plain, ragged with three waves, two float32 column blocks / ten binary16 strips
ROWS = [('rows', case(dt, 2, h, w), tuple({'pair_band': b} for b in sorted({0, 4, 5, 6, 7, h})))
        for dt in ('float32', 'float16') for w in (40, 128, 130, 600) for h in range(1, 14)]
# The host evens the bands out (band_h = ceil(h / ceil(h / pair_band))), so a last band of r rows at a band height b
# needs h >= (b - r) b + r: up to h = 13 that gives b = 4 and (5, 3) only.  The smallest heights for the rest:
TALL = (17, 21, 26, 31, 37, 43)                 # (5, 2); (5, 1), (6, 3); (6, 2); (6, 1), (7, 3); (7, 2); (7, 1)
ROWS += [('rows', case(dt, 2, h, w), tuple({'pair_band': b} for b in (5, 6, 7)))
         for dt in ('float32', 'float16') for w in (40, 600) for h in TALL]

# 4. flags, pairwise: at a narrow, a plain and a multi-block shape per dtype
FLAG_SHAPES = ((9, 40), (9, 256), (9, 600))
FLAG_SETS = (
    dict(bias1=True, bias2=False),                                           # a switched-off bias, accumulating: unchanged
    dict(bias1=False, bias2=True, accumulate=False),                         # ... overwriting: 0
    dict(bias1=False, bias2=False),
    dict(bias1=True, bias2=False, accumulate=False, sigmoid=False),
    dict(bias1=False, bias2=True, pad1=0.25, alpha=0.3),
    dict(accumulate=False, gscale=3),
    dict(sigmoid=False, need_dx=False, pad1=0.25),
    dict(sigmoid=False, alpha=0.3, pad1=-0.5, gscale=9),
    dict(alpha=0.0, need_dx=False, pad1=0.25, accumulate=False),
    dict(alpha=0.0, sigmoid=False),
    dict(alpha=1.0, pad1=-0.5, sigmoid=False),
    dict(alpha=1.0, need_dx=False),
    dict(alpha=0.3, gscale=3, pad1=0.25),
    dict(need_dx=False, pad1=-0.5),
)
FLAGS = [('flags', case(dt, 2, h, w, **fl), AUTO) for dt in ('float32', 'float16') for h, w in FLAG_SHAPES
         for fl in FLAG_SETS] + \
        [('flags', case(dt, 2, 9, 600, deferred=True, **fl), AUTO) for dt in ('float32', 'float16')
         for fl in (dict(), dict(bias1=False, accumulate=False, need_dx=False, pad1=0.25))]

# 5. forced forms
G2 = ({}, {'pair_g': 2})
PFS = ({}, {'pair_pf': 0}, {'pair_pf': 1}, {'pair_pf': 2}, {'pair_pf': -1})
FORCED_G = [('g2', case('float32', 2, 7, w, pad), G2)
            for w, pad in ((31, 0.0), (32, 0.0), (32, 0.25), (33, 0.0), (480, 0.0), (481, 0.0), (512, 0.0), (513, 0.0),
                           (513, 0.25), (1023, 0.0))] + \
           [('g2', case('float16', 2, 7, w, pad), G2)
            for w, pad in ((300, 0.0), (512, 0.0), (513, 0.0), (562, 0.25), (1024, 0.0))]
FORCED_PF = [('pf', case(dt, 2, 7, w, pad), PFS) for dt in ('float32', 'float16')
             for w, pad in ((256, 0.0), (130, 0.0), (600, 0.25))]

# 6. batch
BATCH = [('batch', case(dt, 1, 9, 130), AUTO) for dt in ('float32', 'float16')] + \
        [('batch', case(dt, 70, 9, 40), AUTO) for dt in ('float32', 'float16')] + \
        [('batch', case(dt, 4096, 1, 1), AUTO) for dt in ('float32', 'float16')] + \
        [('batch', case(dt, 12800, 1, 1, deferred=True), AUTO) for dt in ('float32', 'float16')] + \
        [('batch', case(dt, 70, 45, 17), AUTO) for dt in ('float32', 'float16')]
# (12800 blocks: 26 MB of partials, beside the 24 MB deferred region.  70 x 45: the auto band rule above its floor.)

# 7. the benchmarked sizes
BENCHED = [('benched', case('float32', 2, 256, 512), AUTO), ('benched', case('float16', 2, 64, 2048), AUTO)]

SECTIONS = {'widths': WIDTHS, 'rows': ROWS, 'flags': FLAGS, 'forced_g': FORCED_G, 'forced_pf': FORCED_PF,
            'batch': BATCH, 'benched': BENCHED}
# first seed tried by a case: its position in the lists, 32 apart -- except where the offline search had to go further
SEED_BASE = {('benched', 0): 700340, ('benched', 1): 700830}


def seed_base(section, index):
    return SEED_BASE.get((section, index), 100000 * (1 + list(SECTIONS).index(section)) + 32 * index)


def all_jobs():
    return [(name, i, job) for name, jobs in SECTIONS.items() for i, job in enumerate(jobs)]


def job_id(job):
    c = job[1]
    flags = ''.join(('' if c['bias1'] else '-b1', '' if c['bias2'] else '-b2', '' if c['sigmoid'] else '-lin',
                     '' if c['need_dx'] else '-nodx', '' if c['accumulate'] else '-over',
                     '' if c['alpha'] == 0.01 else f"-a{c['alpha']:g}", '' if c['gscale'] == 6 else f"-s{c['gscale']}",
                     '-defer' if c['deferred'] else ''))
    return f"{c['dtype'][5:]}-{c['n']}x{c['h']}x{c['w']}-pad{c['pad1']:g}{flags}"


# ---- inputs and the oracle -----------------------------------------------------------------------------------------------
def draw(c, seed):
    """Seeded inputs as the existing pair tests draw them, and the operands the oracle sees."""
    rng = np.random.default_rng(seed)
    shape = (c['n'], c['h'], c['w'], 1)
    half = c['dtype'] == 'float16'
    x = rng.random(shape) if half else rng.standard_normal(shape)
    w1 = rng.standard_normal((3, 3, 1, 16)) * 0.4
    b1 = rng.standard_normal(16) * (0.1 if half else 0.3)
    w2 = rng.standard_normal((3, 3, 16, 1)) * 0.2
    b2 = rng.standard_normal(1) * (0.1 if half else 1.0)
    g = rng.standard_normal(shape)
    d = dict(x=x, w1=w1, b1=b1, w2=w2, b2=b2, g=g)
    if half:                                    # binary16 x / dy, float32 master weights rounded to binary16 as operands
        d['o'] = dict(x=r16(x), w1=r16(f32(w1)), b1=f32(b1), w2=r16(f32(w2)), b2=f32(b2), g=r16(g))
    else:
        d['o'] = dict(x=x, w1=w1, b1=b1, w2=w2, b2=b2, g=g)
    return d


def forward_ref(c, d):
    o = d['o']
    half = c['dtype'] == 'float16'
    z1 = O.conv2d_fwd(o['x'], o['w1'], o['b1'], 1, 1, c['pad1'], c['bias1'])
    a1 = O.leaky_relu_fwd(z1, c['alpha'])
    if half:
        a1 = r16(a1)
    z2 = O.conv2d_fwd(a1, o['w2'], o['b2'], 1, 1, 0.0, c['bias2'])
    return dict(z1=z1, a1=a1, z2=z2, y=O.sigmoid_fwd(z2) if c['sigmoid'] else z2)


def well_posed(c, d, ref):
    """no z1 of the oracle within 2^-20 * (sum |x w1| + |b1|) of zero (module docstring)"""
    if c['alpha'] == 1.0:
        return True
    o = d['o']
    mag = O.conv2d_fwd(np.abs(o['x']), np.abs(o['w1']), np.abs(o['b1']), 1, 1, abs(c['pad1']), c['bias1'])
    return not bool(np.any(np.abs(ref['z1']) < 2.0 ** -20 * mag))


def db2_cancels(c, d, ref):
    """the one-element db2, accumulated into ACC_INIT, loses more than a factor 4 to cancellation (module docstring)"""
    if not (c['bias2'] and c['accumulate']):
        return False
    o, y = d['o'], ref['y']
    db2 = float(np.sum(o['g'] * y * (1 - y) if c['sigmoid'] else o['g']))
    if c['dtype'] == 'float16':
        db2 /= 2.0 ** c['gscale']
    return abs(ACC_INIT[3] + db2) < 0.25 * max(abs(ACC_INIT[3]), abs(db2))


def qualified(c, base):
    """(seed, inputs, forward reference) of the first qualifying seed, or (None, None, None)"""
    for seed in range(base, base + SEEDS):
        d = draw(c, seed)
        ref = forward_ref(c, d)
        if well_posed(c, d, ref) and not db2_cancels(c, d, ref):
            return seed, d, ref
    return None, None, None


def backward_ref(c, d, ref, y_stored=None):
    """dx, dw1, db1, dw2, db2; binary16: from the stored y, d_z2 and d_a1 rounded to binary16, gradients / 2^gscale"""
    o = d['o']
    half = c['dtype'] == 'float16'
    if not c['sigmoid']:
        gz2 = o['g']
    elif half:
        gz2 = r16(o['g'] * y_stored * (1 - y_stored))
    else:
        gz2 = O.sigmoid_bwd(ref['z2'], o['g'])
    ga1, dw2, db2 = O.conv2d_bwd(ref['a1'], o['w2'], gz2, 1, 1, 0.0, c['bias2'])
    gz1 = O.leaky_relu_bwd(ref['z1'], ga1, c['alpha'])
    if half:
        gz1 = r16(gz1)
    dx, dw1, db1 = O.conv2d_bwd(o['x'], o['w1'], gz1, 1, 1, c['pad1'], c['bias1'])
    k = 2.0 ** c['gscale'] if half else 1.0
    return dx, dw1 / k, db1 / k, dw2 / k, db2 / k


# ---- CPU-only checks -----------------------------------------------------------------------------------------------------
def test_every_case_has_a_qualifying_seed():
    """The seed search of the module docstring for every parametrised case, on the oracle alone.  (The two benchmarked
    sizes are searched by test_benched_cases_qualify: a few seconds each.)"""
    missing = [f'{name}[{i}] {job_id(job)}' for name, i, job in all_jobs() if name != 'benched'
               and qualified(job[1], seed_base(name, i))[0] is None]
    assert not missing, f'no qualifying seed among {SEEDS}: {missing}'


def test_benched_cases_qualify():
    for i, job in enumerate(BENCHED):
        assert qualified(job[1], seed_base('benched', i))[0] is not None, job_id(job)


def reached_forms(cu):
    """every (tuple, details) the host rules choose over all parametrised launches on a device with `cu` compute units"""
    out = []
    for _, _, (_, c, opt_sets) in all_jobs():
        for opts in opt_sets:
            for which in ('fwd', 'bwd'):
                out.append(expect_pair(which, c['dtype'], c['n'], c['h'], c['w'], c['pad1'], opts, cu))
    return out


@pytest.mark.parametrize('cu', [256, 64])
def test_shapes_reach_every_form(cu):
    """The Python host rules over all parametrised shapes: together they reach every class of launch form."""
    forms = reached_forms(cu)
    by_kernel = {k: [(t, d) for t, d in forms if t[0] == k] for k in range(1, 6)}
    every_nw = {(nw, mode) for nw in range(1, 9) for mode in (0, 1)}
    summary = []

    def reach(what, got, want):
        assert set(want) <= set(got), f'cu={cu}: {what}: not reached {sorted(set(want) - set(got))}'
        summary.append(f'{what}: {sorted(set(got))}')

    # float32: every number of waves in both modes, forward and backward; column blocks; G = 2 up to 16 waves
    reach('float32 forward (waves, mode)', {(t[4], t[2]) for t, _ in by_kernel[1]}, every_nw)
    reach('float32 backward G=4 (waves, mode)', {(t[4], t[2]) for t, _ in by_kernel[2] if t[1] == 4}, every_nw)
    reach('float32 backward G=2 (waves, mode)', {(t[4], t[2]) for t, _ in by_kernel[2] if t[1] == 2},
          {(1, 0), (1, 1), (2, 1), (15, 0), (16, 0), (16, 1)})
    reach('float32 forward column blocks', {d['nbx'] for _, d in by_kernel[1]}, {1, 2, 3})
    reach('float32 backward column blocks', {d['nbx'] for t, d in by_kernel[2] if t[1] == 4}, {1, 2, 3})
    reach('float32 backward G=2 column blocks', {d['nbx'] for t, d in by_kernel[2] if t[1] == 2}, {1, 2, 3})
    # binary16 forward: strips, live strips of a last block behind other blocks
    reach('binary16 forward strips', {d['nstrips'] for _, d in by_kernel[3]}, range(1, 10))
    reach('binary16 forward live strips of the last of several blocks',
          {d['last_live'] for t, d in by_kernel[3] if t[5] > 1}, {1, 2, 3, 4})
    # binary16 backward: both families; the cooperative one with every number of waves in both modes
    assert by_kernel[4] and by_kernel[5]
    reach('binary16 cooperative backward (waves, mode)', {(t[4], t[2]) for t, _ in by_kernel[4]}, every_nw)
    reach('binary16 independent-wave backward G=4 live strips of the last block',
          {d['last_live'] for t, d in by_kernel[5] if t[1] == 4 and t[5] > 1}, {1, 2, 3, 4})
    reach('binary16 independent-wave backward G', {t[1] for t, _ in by_kernel[5]}, {2, 4})
    reach('float32 backward G', {t[1] for t, _ in by_kernel[2]}, {2, 4})
    assert {t[1] for k in (1, 3, 4) for t, _ in by_kernel[k]} == {4}
    # prefetch forms of both forwards
    reach('float32 forward prefetch forms', {t[3] for t, _ in by_kernel[1]}, {0, 1, 2})
    reach('binary16 forward prefetch forms', {t[3] for t, _ in by_kernel[3]}, {0, 1, 2})
    # rows: last bands of 1, 2 and 3 rows at band heights 4 - 7, for every kernel
    short = {(bh, last) for bh in (4, 5, 6, 7) for last in (1, 2, 3)}
    for k in range(1, 6):
        reach(f'kernel {k} (band height, rows of the last band)',
              {(t[7], d['last_band']) for t, d in by_kernel[k] if t[6] > 1 and d['last_band'] <= 3}, short)
        reach(f'kernel {k} single-band heights', {t[7] for t, _ in by_kernel[k] if t[6] == 1}, range(1, 14))
    print(f'\nlaunch forms reached with {cu} compute units ({len(forms)} launches):\n  ' + '\n  '.join(summary))


def test_host_rule_copies_on_known_shapes():
    """The Python rules on shapes whose geometry the kernel comments state: 512 columns = 8 waves, one block, MODE 0;
    1024 x 2048 binary16 = 33 strips in 9 blocks; band heights below 4 are raised to 4, never above h."""
    assert expect_pair('bwd', 'float32', 32, 256, 512, 0.0, {}, 256)[0] == (2, 4, 0, 0, 8, 1, 8, 32)
    assert expect_pair('fwd', 'float32', 32, 256, 512, 0.25, {}, 256)[0] == (1, 4, 1, 1, 8, 1, 16, 16)
    assert expect_pair('fwd', 'float16', 8, 1024, 2048, 0.0, {}, 256)[0][:6] == (3, 4, 0, 2, 4, 9)
    assert expect_pair('bwd', 'float16', 8, 1024, 2048, 0.0, {'pair_g': 2}, 256)[0][:6] == (5, 2, 0, 0, 4, 18)
    assert expect_pair('bwd', 'float16', 2, 9, 512, 0.0, {'pair_g': 2}, 256)[0][:6] == (4, 4, 0, 0, 8, 1)
    assert expect_pair('bwd', 'float32', 2, 9, 40, 0.0, {'pair_band': 1}, 256)[0][6:] == (3, 4)
    assert expect_pair('bwd', 'float32', 2, 3, 40, 0.0, {'pair_band': 7}, 256)[0][6:] == (1, 3)
    assert expect_pair('bwd', 'float32', 2, 7, 1533, 0.0, {}, 256)[1]['nbx'] == 4


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


def check(a, ref, tol, what):
    from univer_ocr_amd.nn import CP
    err = rel_linf(CP.asnumpy(a), ref)
    print(f'    {what}: rel_linf {err:.3e} (bound {tol:.1e})')
    assert err <= tol, f'{what}: rel_linf={err:.3e} > {tol:.1e}'


def run_job(CP, section, index, same_y=False):
    """One case under each of its option sets: forward, `last_pair`, y; backward, `last_pair`, dx / dw1 / db1 / dw2 /
    db2.  same_y: every option set's y must equal the first set's bit for bit.  Returns the host copies of y."""
    from univer_ocr_amd.hip import lib as hiplib
    from univer_ocr_amd.nn import ops
    _, c, opt_sets = SECTIONS[section][index]
    seed, d, ref = qualified(c, seed_base(section, index))
    assert seed is not None, f'{job_id(SECTIONS[section][index])}: no qualifying seed among {SEEDS}'
    rt = CP.runtime()
    cu = rt.device_info()['cu_count']
    half = c['dtype'] == 'float16'
    CP.set_dtype(c['dtype'])
    xd, gd = CP.copy(d['x']), CP.copy(d['g'])
    if half:
        gd.gscale = c['gscale']
    w1d, b1d, w2d, b2d = (CP.copy(d[k], np.float32) for k in ('w1', 'b1', 'w2', 'b2'))
    act2 = hiplib.ACT_SIGMOID if c['sigmoid'] else hiplib.ACT_NONE
    geo = (c['dtype'], c['n'], c['h'], c['w'], c['pad1'])
    tol_y, tol_dx = (TOL_STORE, TOL_STORE) if half else (TOL_Y32, TOL_G32)
    ys = []
    for opts in opt_sets:
        what = f'{job_id(SECTIONS[section][index])} seed {seed} {opts}'
        print(f'  {what}')
        for key in ('pair_band', 'pair_g', 'pair_pf'):
            rt.set_option(key, opts.get(key, dict(DEFAULTS)[key]))
        y = ops.conv_pair_fwd(xd, w1d, b1d, w2d, b2d, c['pad1'], c['bias1'], c['bias2'], c['alpha'], act2)
        got, exp = rt.last_pair(), expect_pair('fwd', *geo, opts, cu)[0]
        assert got == exp, f'{what}: forward last_pair {got} != host rule {exp}'
        assert got[1] == 4, 'the forward kernels exist for G = 4 only'
        check(y, ref['y'], tol_y, 'y')
        yh = CP.asnumpy(y)
        assert yh.dtype == (np.float16 if half else np.float32)
        ys.append(yh)
        if same_y:
            assert np.array_equal(yh, ys[0]), f'{what}: y differs from the auto form ' \
                f'(max |diff| {np.nanmax(np.abs(yh.astype(np.float64) - ys[0])):.3e})'
        refs = backward_ref(c, d, ref, yh.astype(np.float64))
        init = ACC_INIT if c['accumulate'] else OVER_INIT
        grads = [CP.full(d[k].shape, v, np.float32) for k, v in zip(('w1', 'b1', 'w2', 'b2'), init)]

        def bwd():
            return ops.conv_pair_bwd(xd, y, gd, w1d, b1d, w2d, *grads, c['pad1'], c['bias1'], c['bias2'], c['alpha'],
                                     act2, need_dx=c['need_dx'], accumulate=c['accumulate'])
        if c['deferred']:
            with rt.defer_wgrad():
                dx = bwd()
        else:
            dx = bwd()
        got, exp = rt.last_pair(), expect_pair('bwd', *geo, opts, cu)[0]
        assert got == exp, f'{what}: backward last_pair {got} != host rule {exp}'
        if half and c['w'] <= 512:
            assert got[:2] == (4, 4), 'up to 512 columns the binary16 backward is the cooperative block with G = 4'
        if c['need_dx']:
            assert dx.dtype == (np.float16 if half else np.float32) and (not half or dx.gscale == c['gscale'])
            check(dx, refs[0], tol_dx, 'dx')
        else:
            assert dx is None
        for name, got_g, r, v, live in zip(('dw1', 'db1', 'dw2', 'db2'), grads, refs[1:], init,
                                           (True, c['bias1'], True, c['bias2'])):
            # a switched-off bias: `live ? s : 0` -- unchanged when accumulating, 0 when overwriting, exactly
            expect = (r if live else np.zeros_like(r)) + (v if c['accumulate'] else 0.0)
            tol = TOL_G32 if not half else TOL_DB1_16 if name == 'db1' else TOL_SUM16
            check(got_g, expect, tol if live else 0.0, name)
    return ys


def ids(section):
    return [job_id(job) for job in SECTIONS[section]]


@pytest.mark.gpu
def test_last_pair_is_zero_before_the_first_pair_launch():
    """A fresh context of its own reports all zeros."""
    import ctypes as C
    from univer_ocr_amd.hip import lib as hiplib
    lib = hiplib.get_lib()
    handle = C.c_void_p()
    assert lib.uocr_ctx_create(0, 0, C.byref(handle)) == 0
    try:
        v = [C.c_int(-1) for _ in range(8)]
        assert lib.uocr_ctx_last_pair(handle, *[C.byref(x) for x in v]) == 0
        assert tuple(x.value for x in v) == (0,) * 8
        assert lib.uocr_ctx_last_pair(handle, None, *[C.byref(x) for x in v[1:]]) != 0      # (a null pointer is refused)
    finally:
        lib.uocr_ctx_destroy(handle)


@pytest.mark.gpu
@pytest.mark.parametrize('index', range(len(WIDTHS)), ids=ids('widths'))
def test_width_sweep(index, ctx):
    """Section 2: widths at every wave seam, block seam and strip seam; all six outputs."""
    run_job(ctx, 'widths', index)


@pytest.mark.gpu
@pytest.mark.parametrize('index', range(len(ROWS)), ids=ids('rows'))
def test_height_band_sweep(index, ctx):
    """Section 3: h = 1 ... 13 under pair_band 0, 4, 5, 6, 7, h; `bands` and `band_h` of last_pair follow the rules
    "raised to 4", "never above h" and the binary16 cost search."""
    run_job(ctx, 'rows', index)


@pytest.mark.gpu
@pytest.mark.parametrize('index', range(len(FLAGS)), ids=ids('flags'))
def test_flags(index, ctx):
    """Section 4: bias pairs, act2, need_dx, accumulate / overwrite, alpha 0 / 0.01 / 0.3 / 1, pad1 0 / 0.25 / -0.5,
    binary16 gradient scales 3 / 6 / 9, a deferred weight-gradient group."""
    run_job(ctx, 'flags', index)


@pytest.mark.gpu
@pytest.mark.parametrize('index', range(len(FORCED_G)), ids=ids('forced_g'))
def test_forced_g2(index, ctx):
    """Section 5: pair_g = 2 (32 columns per wave, up to 16 waves; binary16: independent waves of 32 columns).  Both
    forwards and the binary16 backward up to 512 columns must report that G = 4 ran (asserted in run_job)."""
    run_job(ctx, 'forced_g', index)


@pytest.mark.gpu
@pytest.mark.parametrize('index', range(len(FORCED_PF)), ids=ids('forced_pf'))
def test_forced_prefetch_forms(index, ctx):
    """Section 5: pair_pf = 0, 1, 2, -1 on both forwards.  The forms differ only in when a row's loads are issued:
    the arithmetic and its order are the same, so y must equal the auto form's bit for bit."""
    run_job(ctx, 'forced_pf', index, same_y=True)


@pytest.mark.gpu
@pytest.mark.parametrize('index', range(len(BATCH)), ids=ids('batch'))
def test_batch_sizes(index, ctx):
    """Section 6: one image; 70 images (9 rows: auto bands at their floor of 4 rows; 45 rows: the auto rule above its
    floor, 6 rows per band forward and 12 backward on 256 compute units); 4096 and 12800 images of 1 x 1 (grid z
    far past one wave of blocks; 8 MB of partials, and 26 MB inside a deferred group: beside its 24 MB region)."""
    run_job(ctx, 'batch', index)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['float32', 'float16'])
def test_batch_limit_fails_loudly(dtype, ctx):
    """n = 65536 is refused with the library's error by both entry points and leaves last_pair as it was."""
    from univer_ocr_amd.hip.lib import HipError
    from univer_ocr_amd.nn import ops
    CP = ctx
    CP.set_dtype(dtype)
    rt = CP.runtime()
    small = CP.copy(np.full((2, 4, 8, 1), 0.5))
    p = [CP.copy(np.full(s, 0.1), np.float32) for s in ((3, 3, 1, 16), (16,), (3, 3, 16, 1), (1,))]
    ops.conv_pair_fwd(small, *p)
    before = rt.last_pair()
    assert before[0] == (1 if dtype == 'float32' else 3)
    x = CP.copy(np.full((65536, 1, 1, 1), 0.5))
    with pytest.raises(HipError, match='n <= 65535'):
        ops.conv_pair_fwd(x, *p)
    assert rt.last_pair() == before
    grads = [CP.full(a.shape, 0.5, np.float32) for a in p]
    with pytest.raises(HipError, match='n <= 65535'):
        ops.conv_pair_bwd(x, x, x, p[0], p[1], p[2], *grads)
    assert rt.last_pair() == before
    for got in grads:
        assert np.all(CP.asnumpy(got) == 0.5)


@pytest.mark.gpu
@pytest.mark.parametrize('index', range(len(BENCHED)), ids=ids('benched'))
def test_benchmarked_sizes(index, ctx):
    """Section 7: float32 2 x 256 x 512 and binary16 2 x 64 x 2048, all six outputs against the oracle."""
    run_job(ctx, 'benched', index)
