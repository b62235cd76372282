"""An elementwise error bound for the conv / dense kernels, inputs whose magnitude varies by region, and the case table
the host checks (test_elementwise_bound_host.py) and the GPU tests (test_gpu_elementwise.py) share.

The bound.  A float32 sum of n products, in any order, with or without FMA, misses the exact sum by at most
gamma(n) * sum |x_i * w_i|, gamma(n) = n u / (1 - n u), u = 2^-24 (Higham, Accuracy and Stability of Numerical
Algorithms, 2nd ed., section 3.1: every term passes through at most n roundings, product included).  The sum of the
absolute products, S, is the oracle's own operation on the absolute values of its operands.  Per output element

    tol = store_u * |ref| + (operand_u + gamma(n + 8)) * S + floor

  n          products per output element;
  + 8        roundings that act on a term already counted in S: the bias add, a LeakyReLU scaling and its float32
             alpha, a mask factor, and the float32 sums of taps that conv_up.hip forms per output phase (at most
             2 x 2 taps of a 5x5 kernel fall on one low-resolution pixel: three additions);
  store_u    2^-11, the unit roundoff of binary16, where the output is stored in binary16 (else 0);
  floor      2^-25, half the spacing 2^-24 of the binary16 subnormals: the absolute error of that store below the
             normal range, which cancellation can reach although every S is normal (else 0);
  operand_u  2^-11 where the kernel rounds an operand to binary16 that the oracle keeps in float32: the master weights
             in conv_h16*.hip, the phase-summed weights of the binary16 upconv, the weights and a1 of the binary16 conv
             pair (else 0).  A rounded operand changes each product by at most 2^-11 of its magnitude.

Nothing here is measured and nothing is multiplied by a safety factor.  The reference is the float64 oracle on the
exact operands: every input is drawn representable in the storage type, so no input rounding enters.

The conv pair composes the bound through both layers (PairProblem.tolerances).

Inputs.  Magnitudes uniform in [0.25, 1] with a random sign (no zeros, no subnormals), times 2^e with e the sum of a
per-image, a per-8-row-band, a per-24-column-strip and a per-channel exponent.  8 and 24 do not divide the 16 / 32 /
64 tile edges of the kernels, so region borders fall on tile borders and inside tiles.  float32: |e| <= 9 + 8 + 10 + 6
= 33.  binary16: image, band and channel 1 each, and the strips all that the normal range [2^-14, 65504] leaves (8, |e|
<= 11, weights without a channel exponent: `fit16`); `Problem.check_ranges` asserts that every stored input and every S
lies in that range.
"""
import functools
from collections import namedtuple

import numpy as np

from oracle import nn_oracle as O
from test_gpu_conv_padding import DGRAD, FWD, TABLE, expect_kernel, make_dims

U32 = 2.0 ** -24                # unit roundoff of binary32: 24 significant bits, round to nearest
U16 = 2.0 ** -11                # unit roundoff of binary16: 11 significant bits
FLOOR16 = 2.0 ** -25            # half the spacing 2^-24 of the binary16 subnormals
SLACK = 8                       # see the module docstring: bias, LeakyReLU and its alpha, mask, <= 3 phase-weight adds
F16_MIN, F16_MAX = 2.0 ** -14, 65504.0          # binary16: smallest normal number, largest finite number
ALLOW = {'float32': 1e-5, 'float16': 1e-3}     # the suite's rel_linf allowance for y / dx (test_gpu_kernels / _f16)
ALPHA = 0.01                    # the LeakyReLU slope of the nets (and of the other conv tests)
BAND, STRIP = 8, 24             # rows per band, columns per strip: neither divides every tile edge (16 / 32 / 64)
# largest |exponent| per kind of region.  float32: the sum, 33, keeps products of two such tensors and a weight far
# inside binary32's range (2^-126 .. 2^127).  binary16: the default below; the cases of the table take theirs from fit16
EXPONENTS = {'float32': dict(image=9, band=8, strip=10, channel=6),
             'float16': dict(image=1, band=1, strip=6, channel=1)}
# weights: 2^WEIGHT_SHIFT * [0.25, 1] * 2^(e_in + e_out), each |e| <= WEIGHT_EXP (binary16: no channel exponent and the
# shift of fit16: the normal range has no room for either)
WEIGHT_SHIFT = {'float32': -2, 'float16': -2}
WEIGHT_EXP = {'float32': 2, 'float16': 0}
BIAS_SHIFT = {'float32': -12, 'float16': -10}   # a bias that dominates the small regions only (binary16: S >= 2^-12 there)
SHAPE, LOW_SHAPE = (3, 37, 141), (2, 19, 71)    # pages; low-resolution upconv inputs: several tiles, ragged last ones
STORE = {'float32': np.float32, 'float16': np.float16}


def gamma(n, u=U32):
    assert n * u < 1
    return n * u / (1 - n * u)


def tolerance(ref, s, n, store16=False, operand16=False):
    """the elementwise tolerance of the module docstring"""
    return (U16 if store16 else 0.0) * np.abs(ref) + ((U16 if operand16 else 0.0) + gamma(n + SLACK)) * s + \
        (FLOOR16 if store16 else 0.0)


def r16(a):
    return np.asarray(a, dtype=np.float64).astype(np.float16).astype(np.float64)


def cdiv(a, b):
    return -(-a // b)


# ---- inputs --------------------------------------------------------------------------------------------------------------
def signed_unit(rng, shape, dtype):
    """magnitudes uniform in [0.25, 1], random sign, representable in the storage type"""
    m = rng.uniform(0.25, 1.0, shape) * np.where(rng.random(shape) < 0.5, -1.0, 1.0)
    return m.astype(STORE[dtype]).astype(np.float64)


def spread(rng, count, limit):
    """`count` exponents in [-limit, limit]; with two or more, both ends occur once and the others lie in [-limit, 0]:
    the few large regions set max |ref|, most elements lie far below it"""
    e = rng.integers(-limit, (limit if count == 1 else 0) + 1, count)
    if count >= 2:
        i, j = rng.choice(count, 2, replace=False)
        e[i], e[j] = limit, -limit
    return e


def region_exponents(rng, shape, r):
    n, h, w, c = shape
    return (spread(rng, n, r['image'])[:, None, None, None] +
            spread(rng, cdiv(h, BAND), r['band'])[np.arange(h) // BAND][None, :, None, None] +
            spread(rng, cdiv(w, STRIP), r['strip'])[np.arange(w) // STRIP][None, None, :, None] +
            spread(rng, c, r['channel'])[None, None, None, :])


def scaled_input(rng, shape, dtype, limits=None, shift=0):
    """an (n, h, w, c) activation tensor of the module docstring; limits: the largest |exponent| per kind of region
    (EXPONENTS[dtype] unless given); shift: one more exponent for the whole tensor"""
    limits = EXPONENTS[dtype] if limits is None else limits
    e = region_exponents(rng, shape, limits)
    assert np.abs(e).max() <= sum(limits.values())
    return signed_unit(rng, shape, dtype) * 2.0 ** (e + shift)


def scaled_weights(rng, shape, dtype, shift=None):
    """float32 parameters (kh, kw, cin, cout) whose magnitude varies by input and output channel"""
    k = WEIGHT_EXP[dtype]
    e = spread(rng, shape[2], k)[:, None] + spread(rng, shape[3], k)[None, :] + (WEIGHT_SHIFT[dtype] if shift is None else shift)
    return signed_unit(rng, shape, 'float32') * 2.0 ** e


def scaled_bias(rng, cout, dtype):
    return signed_unit(rng, (cout,), 'float32') * 2.0 ** (spread(rng, cout, WEIGHT_EXP[dtype]) + BIAS_SHIFT[dtype])


def leaky(y, dt):
    if dt is np.float64:
        return O.leaky_relu_fwd(y, ALPHA)
    return np.where(y >= 0, y, y * dt(ALPHA)).astype(dt)


def slope_of(m, dt=np.float64):
    return np.where(m >= 0, dt(1.0), dt(ALPHA)).astype(dt)


# ---- problems ------------------------------------------------------------------------------------------------------------
# One problem = one set of operands and every output judged on it.  `run(q, dt)`: the oracle's code on the operands q in
# `dt` arithmetic -> {output: array}.  `tolerances(operand16)`: {output: elementwise tolerance}; operand16 = the outputs
# whose kernel rounds an operand to binary16.
class Problem:
    weights = ('w',)

    def __init__(self, name, dtype, seed, fit=None):
        self.name, self.dtype, self.seed = name, dtype, seed
        self.half = dtype == 'float16'
        # fit (binary16, see fit16): (exponent limits, shift of the weights, shift of dy / of the second weights)
        self.limits, self.wshift, self.gshift = (None, None, 0) if fit is None else fit

    def in_range(self):
        try:
            self.check_ranges()
        except AssertionError:
            return False
        return True

    @functools.cached_property
    def q(self):
        q = self.draw(np.random.default_rng(self.seed))
        for a in q.values():
            a.setflags(write=False)
        return q

    @functools.cached_property
    def ref(self):
        out = self.run(self.q, np.float64)
        for a in out.values():
            a.setflags(write=False)
        return out

    @functools.cached_property
    def sums(self):
        """{output: (S, n)}"""
        return self.abs_sums()

    def cast(self, q, dt):
        return {k: np.asarray(v).astype(dt) for k, v in q.items()}

    def restated(self, store=True):
        """float32 NumPy restatement; store: a binary16 output is rounded once to binary16"""
        out = self.run(self.cast(self.q, np.float32), np.float32)
        assert all(a.dtype == np.float32 for a in out.values()), {k: a.dtype for k, a in out.items()}
        return {k: (r16(a) if self.half and store else a.astype(np.float64)) for k, a in out.items()}

    def store_part(self, name):
        """the part of the tolerance of output `name` that belongs to the binary16 store alone"""
        return U16 * np.abs(self.ref[name]) + FLOOR16 if self.half else np.zeros(self.ref[name].shape)

    def with_rounded_weights(self):
        """mutation: the weights rounded to binary16, everything else exact"""
        q = dict(self.q)
        for k in self.weights:
            q[k] = r16(q[k])
        return self.run(q, np.float64)

    def tolerances(self, operand16=()):
        out = {}
        for k, (s, n) in self.sums.items():
            if k == 'y_leaky':
                # where y lies below minus its own arithmetic bound the kernel's y is negative too, and the epilogue
                # scales value and error alike by alpha (its rounding is one of the + 8); elsewhere the full S stands
                arith = ((U16 if k in operand16 else 0.0) + gamma(n + SLACK)) * s
                s = np.where(self.ref['y'] < -arith, ALPHA * s, s)
            out[k] = tolerance(self.ref[k], s, n, self.half, k in operand16)
        return out

    def judged(self, name):
        """boolean mask of the elements of output `name` that are judged (all, but for the pair's dx)"""
        return np.ones(self.ref[name].shape, bool)

    def check_ranges(self):
        """binary16: every stored input and every S inside the normal range"""
        if not self.half:
            return
        for k in self.stored:
            a = np.abs(self.q[k])
            assert F16_MIN <= a.min() and a.max() <= F16_MAX, (self.name, k, a.min(), a.max())
            assert np.array_equal(r16(self.q[k]), self.q[k]), (self.name, k)
        for k, (s, _) in self.sums.items():
            if k.endswith('_leaky'):            # y_leaky, dx_leaky: S is y's / dx's, asserted here, times a slope of 1 or
                continue                        # alpha; alpha S may be subnormal, and the floor term covers that store
            assert F16_MIN <= s.min() and s.max() <= F16_MAX, (self.name, k, s.min(), s.max())


class ConvProblem(Problem):
    stored = ('x', 'g', 'm')

    def __init__(self, name, dtype, seed, geom, shape=SHAPE, pad_value=0.0, bias=True, fit=None):
        super().__init__(name, dtype, seed, fit)
        kh, kw, cin, cout, sh, sw, ph, pw = geom
        self.d = make_dims(*shape, kh, kw, cin, cout, sh, sw, ph, pw)
        self.pad_value, self.bias = pad_value, bias

    def draw(self, rng):
        d = self.d
        return dict(x=scaled_input(rng, (d.n, d.h, d.w, d.cin), self.dtype, self.limits),
                    w=scaled_weights(rng, (d.kh, d.kw, d.cin, d.cout), self.dtype, self.wshift),
                    b=scaled_bias(rng, d.cout, self.dtype),
                    g=scaled_input(rng, (d.n, d.oh, d.ow, d.cout), self.dtype, self.limits, self.gshift),
                    m=signed_unit(rng, (d.n, d.h, d.w, d.cin), self.dtype))

    def _conv(self, x, w, b, g, pv):
        d = self.d
        st, pd = (d.sh, d.sw), (d.ph, d.pw)
        y = O.conv2d_fwd(x, w, b, st, pd, pv, self.bias)
        dx = O.conv2d_bwd(x, w, g, st, pd, pv, self.bias)[0]
        return y, dx

    def run(self, q, dt):
        y, dx = self._conv(q['x'], q['w'], q['b'], q['g'], dt(self.pad_value))
        return dict(y=y, y_leaky=leaky(y, dt), dx=dx, dx_leaky=dx * slope_of(q['m'], dt))

    def abs_sums(self):
        d, a = self.d, {k: np.abs(v) for k, v in self.q.items()}
        sy, sdx = self._conv(a['x'], a['w'], a['b'], a['g'], abs(self.pad_value))
        ny = d.kh * d.kw * d.cin
        ndx = cdiv(d.kh, d.sh) * cdiv(d.kw, d.sw) * d.cout       # the taps that can reach one input pixel
        return dict(y=(sy, ny), y_leaky=(sy, ny), dx=(sdx, ndx), dx_leaky=(sdx * slope_of(self.q['m']), ndx))


class UpProblem(Problem):
    """Upsample2D(2) + conv 5x5 (padding 2, padding value 0) on the low-resolution tensor"""
    stored = ('x', 'g', 'm')

    def __init__(self, name, dtype, seed, ch, shape=LOW_SHAPE, fit=None):
        super().__init__(name, dtype, seed, fit)
        self.ch, self.shape = ch, shape

    def draw(self, rng):
        n, hl, wl = self.shape
        ch = self.ch
        return dict(x=scaled_input(rng, (n, hl, wl, ch), self.dtype, self.limits),
                    w=scaled_weights(rng, (5, 5, ch, ch), self.dtype, self.wshift), b=scaled_bias(rng, ch, self.dtype),
                    g=scaled_input(rng, (n, 2 * hl, 2 * wl, ch), self.dtype, self.limits, self.gshift),
                    m=signed_unit(rng, (n, hl, wl, ch), self.dtype))

    @staticmethod
    def _up(x, w, b, g):
        up = O.upsample2d_fwd(x, (2, 2))
        y = O.conv2d_fwd(up, w, b, 1, 2, 0.0, True)
        dx = O.upsample2d_bwd(O.conv2d_bwd(up, w, g, 1, 2, 0.0, True)[0], (2, 2))
        return y, dx

    def run(self, q, dt):
        y, dx = self._up(q['x'], q['w'], q['b'], q['g'])
        return dict(y=y, y_leaky=leaky(y, dt), dx=dx, dx_leaky=dx * slope_of(q['m'], dt))

    def abs_sums(self):
        a = {k: np.abs(v) for k, v in self.q.items()}
        sy, sdx = self._up(a['x'], a['w'], a['b'], a['g'])
        ny, ndx = 25 * self.ch, 4 * 25 * self.ch                 # dx: the 2 x 2 high-resolution pixels of one source pixel
        return dict(y=(sy, ny), y_leaky=(sy, ny), dx=(sdx, ndx), dx_leaky=(sdx * slope_of(self.q['m']), ndx))


class PairProblem(Problem):
    """conv3x3(1 -> 16) + LeakyReLU + conv3x3(16 -> 1), act2 none: y, and (float32) dx"""
    stored = ('x', 'g')
    weights = ('w1', 'w2')

    def __init__(self, name, dtype, seed, shape=SHAPE, fit=None):
        super().__init__(name, dtype, seed, fit)
        self.shape = shape
        self.pad1 = 0.0 if self.half else 0.25

    def draw(self, rng):
        n, h, w = self.shape
        w2shift = None if self.wshift is None else self.gshift        # (binary16 has no dx here: the slot is free)
        return dict(x=scaled_input(rng, (n, h, w, 1), self.dtype, self.limits),
                    w1=scaled_weights(rng, (3, 3, 1, 16), self.dtype, self.wshift), b1=scaled_bias(rng, 16, self.dtype),
                    w2=scaled_weights(rng, (3, 3, 16, 1), self.dtype, w2shift), b2=scaled_bias(rng, 1, self.dtype),
                    g=scaled_input(rng, (n, h, w, 1), self.dtype, self.limits))

    def _layers(self, q, dt):
        z1 = O.conv2d_fwd(q['x'], q['w1'], q['b1'], 1, 1, dt(self.pad1), True)
        a1 = leaky(z1, dt)
        return z1, a1, O.conv2d_fwd(a1, q['w2'], q['b2'], 1, 1, dt(0.0), True)

    def run(self, q, dt):
        z1, a1, z2 = self._layers(q, dt)
        out = dict(y=z2)
        if not self.half:
            ga1 = O.conv2d_bwd(a1, q['w2'], q['g'], 1, 1, dt(0.0), True)[0]
            out['dx'] = O.conv2d_bwd(q['x'], q['w1'], ga1 * slope_of(z1, dt), 1, 1, dt(self.pad1), True)[0]
        return out

    abs_sums = None

    @functools.cached_property
    def _composed(self):
        """The bound through both layers, for operand16 False and True.
        forward:  E1 = (op + gamma(9 + 8)) S1 bounds z1; LeakyReLU is 1-Lipschitz, so E1 bounds a1 too, and an a1
                  rounded to binary16 adds op (|a1| + E1).  The second conv sees a1 + e, |e| <= Ea1: the error it inherits is
                  conv(Ea1, |w2|), its own is (op + gamma(144 + 8)) conv(|a1| + Ea1, |w2|, |b2|).
        backward: Ega = gamma(9 + 8) Sga bounds ga1 = dgrad(dy, w2); where the slope of z1 is decided (|z1| > E1) the
                  mask scales ga1 and Ega alike; dx inherits dgrad(Egz, |w1|) and adds gamma(144 + 8) dgrad(|gz1| + Egz,
                  |w1|).  Pixels whose 3x3 field holds an undecided z1 are not judged."""
        q, a = self.q, {k: np.abs(v) for k, v in self.q.items()}
        z1, a1, z2 = self._layers(q, np.float64)
        s1 = O.conv2d_fwd(a['x'], a['w1'], a['b1'], 1, 1, abs(self.pad1), True)
        out = {}
        for op in (False, True):
            opu = U16 if op else 0.0
            e1 = (opu + gamma(9 + SLACK)) * s1
            ea1 = e1 + opu * (np.abs(a1) + e1)
            hi = np.abs(a1) + ea1
            zero = np.zeros(1)
            e2 = O.conv2d_fwd(ea1, a['w2'], zero, 1, 1, 0.0, False) + \
                (opu + gamma(144 + SLACK)) * O.conv2d_fwd(hi, a['w2'], a['b2'], 1, 1, 0.0, True)
            tol = dict(y=(U16 * np.abs(z2) + FLOOR16 if self.half else 0.0) + e2)
            judged = None
            if not self.half:
                undecided = (np.abs(z1) <= e1).any(axis=3, keepdims=True).astype(np.float64)
                judged = O.conv2d_fwd(undecided, np.ones((3, 3, 1, 1)), zero, 1, 1, 0.0, False) == 0
                sl = slope_of(z1)
                sga = O.conv2d_bwd(a1, a['w2'], a['g'], 1, 1, 0.0, True)[0]
                ega = gamma(9 + SLACK) * sga
                gz1 = O.conv2d_bwd(a1, q['w2'], q['g'], 1, 1, 0.0, True)[0] * sl
                egz = ega * sl
                tol['dx'] = O.conv2d_bwd(a['x'], a['w1'], egz, 1, 1, 0.0, True)[0] + \
                    gamma(144 + SLACK) * O.conv2d_bwd(a['x'], a['w1'], np.abs(gz1) + egz, 1, 1, 0.0, True)[0]
            out[op] = tol, judged, s1
        return out

    def tolerances(self, operand16=()):
        return self._composed[bool(operand16)][0]

    def judged(self, name):
        return self._composed[False][1] if name == 'dx' else np.ones(self.ref[name].shape, bool)

    def check_ranges(self):
        if not self.half:
            return
        for k in self.stored:
            a = np.abs(self.q[k])
            assert F16_MIN <= a.min() and a.max() <= F16_MAX and np.array_equal(r16(self.q[k]), self.q[k]), (self.name, k)
        a = {k: np.abs(v) for k, v in self.q.items()}
        s1 = self._composed[True][2]
        s2 = O.conv2d_fwd(leaky(s1, np.float64), a['w2'], a['b2'], 1, 1, 0.0, True)
        for s in (s1, s2):
            assert F16_MIN <= s.min() and s.max() <= F16_MAX, (self.name, s.min(), s.max())


DENSE_M, DENSE_K, DENSE_N = 67, 200, 70
WIN_SHAPE, WIN_WIDTH = (1, 5, 67, 5), 8          # 5 rows x 8 columns x 5 channels = 200 inputs per window, 67 windows


def dense_weights(rng):
    """(K + 1, N), bias row last; rows carry 2^[-6, 6], columns 2^[-10, 10]"""
    e = spread(rng, DENSE_K + 1, 6)[:, None] + spread(rng, DENSE_N, 10)[None, :]
    return signed_unit(rng, (DENSE_K + 1, DENSE_N), 'float32') * 2.0 ** e


class DenseProblem(Problem):
    """y = [x, 1] . w and dx = dy . w^T; the rows of x / dy carry 2^[-16, 16] (with the weights: |e| <= 32)"""
    stored = ()

    def draw(self, rng):
        rows = lambda cols: signed_unit(rng, (DENSE_M, cols), 'float32') * 2.0 ** spread(rng, DENSE_M, 16)[:, None]
        return dict(x=rows(DENSE_K), w=dense_weights(rng), g=rows(DENSE_N))

    def run(self, q, dt):
        return dict(y=O.dense_fwd(q['x'], q['w']), dx=O.dense_bwd(q['x'], q['w'], q['g'])[0])

    def abs_sums(self):
        out = self.run({k: np.abs(v) for k, v in self.q.items()}, np.float64)
        return dict(y=(out['y'], DENSE_K), dx=(out['dx'], DENSE_N))


class WindowsProblem(Problem):
    """fixed-width windows + flatten + dense as one implicit GEMM (ops.windows_dense_*)"""
    stored = ()

    def draw(self, rng):
        return dict(x=scaled_input(rng, WIN_SHAPE, 'float32'), w=dense_weights(rng),
                    g=signed_unit(rng, (DENSE_M, DENSE_N), 'float32') * 2.0 ** spread(rng, DENSE_M, 16)[:, None])

    def run(self, q, dt):
        rows = O.fixed_width_fwd(q['x'], WIN_WIDTH).astype(dt).reshape(DENSE_M, DENSE_K)
        dwin = O.dense_bwd(rows, q['w'], q['g'])[0].reshape(DENSE_M, WIN_SHAPE[1], WIN_WIDTH, WIN_SHAPE[3])
        return dict(y=O.dense_fwd(rows, q['w']), dx=O.fixed_width_bwd(dwin, WIN_SHAPE, WIN_WIDTH).astype(dt))

    def abs_sums(self):
        out = self.run({k: np.abs(v) for k, v in self.q.items()}, np.float64)
        return dict(y=(out['y'], DENSE_K), dx=(out['dx'], WIN_WIDTH * DENSE_N))    # a pixel lies in 8 windows of 70 outputs


# ---- the case table --------------------------------------------------------------------------------------------------------
# Case: a problem, the options it runs under, the outputs judged and (ops on the conv entry points) the kernel family
# `Runtime.last_conv` must report per output.
Case = namedtuple('Case', 'id problem opts outputs kernels operand16')
MFMA_GEOM = (3, 3, 32, 32, 1, 1, 1, 1)
GENERIC_GEOM = (4, 4, 6, 7, 2, 1, 1, 2)
CONV_OUTPUTS = ('y', 'y_leaky', 'dx', 'dx_leaky')
SEEDS = dict(table=9000, mfma=9100, generic=9200, up=9310, pair=9400, dense=9500, windows=9600)


def fit16(make):
    """binary16: the problem with the widest spread between strips whose stored inputs and S all lie in the normal range.
    The range 2^-14 .. 65504 is 2^30 wide.  An S spans (most products / fewest products of an element, 2 .. 5) x 2^2 (unit
    magnitudes of x) x 2^2 (of w) x 2^(2 E), E the sum of the four exponent limits, so E <= 11 can fit: image, band and
    channel keep 1 each and the strips get E - 3.  The weights and dy (for the pair: the second weights) take the
    power of two that centres y's and dx's S in the range; both shifts and E are found by trying, widest E first."""
    for total in (11, 10, 9):
        for wshift in range(2, -9, -1):
            for gshift in range(4, -9, -1):
                p = make((dict(image=1, band=1, strip=total - 3, channel=1), wshift, gshift))
                if p.in_range():
                    return p
    raise AssertionError('no exponent budget fits binary16')


@functools.lru_cache(maxsize=None)
def problem(kind, dtype, key):
    seed = SEEDS[kind] + (0 if dtype == 'float32' else 5000)
    fitted = fit16 if dtype == 'float16' else (lambda make: make(None))
    if kind == 'table':
        cfg = TABLE[key]
        # even rows of the table: a padding value and no bias; odd rows: a bias and zero padding
        return fitted(lambda fit: ConvProblem(f'table{key}', dtype, seed + key, (*cfg[:6], *cfg.net_pad),
                                              pad_value=0.25 if key % 2 == 0 else 0.0, bias=key % 2 == 1, fit=fit))
    if kind == 'mfma':
        return ConvProblem('mfma', dtype, seed, MFMA_GEOM, pad_value=0.0, bias=True)
    if kind == 'generic':
        return ConvProblem('generic', dtype, seed, GENERIC_GEOM, pad_value=0.25, bias=True)
    if kind == 'up':
        return fitted(lambda fit: UpProblem(f'up{key}', dtype, seed + key, key, fit=fit))
    if kind == 'pair':
        return fitted(lambda fit: PairProblem('pair', dtype, seed, fit=fit))
    if kind == 'dense':
        return DenseProblem('dense', dtype, seed)
    assert kind == 'windows'
    return WindowsProblem('windows', dtype, seed)


def _conv_case(p, opts, tag):
    kf, kd = (expect_kernel(e, p.dtype, p.d, p.pad_value, opts) for e in (FWD, DGRAD))
    kernels = dict(y=kf, y_leaky=kf, dx=kd, dx_leaky=kd)
    operand16 = tuple(k for k, v in kernels.items() if p.half and v == 'h16')
    return Case(f'{p.dtype[5:]}-{p.name}{tag}', p, opts, CONV_OUTPUTS, kernels, operand16)


def _cases():
    out = []
    for i in range(len(TABLE)):
        out.append(_conv_case(problem('table', 'float32', i), {}, ''))
        out.append(_conv_case(problem('table', 'float32', i), {'t32': 0, 'tiled': 0}, '-t32_0-tiled0'))
    out.append(_conv_case(problem('mfma', 'float32', 0), {'mfma': 2}, '-mfma2'))
    out.append(_conv_case(problem('generic', 'float32', 0), {}, ''))
    for ch in (4, 1):
        out.append(Case(f'32-up{ch}', problem('up', 'float32', ch), {}, CONV_OUTPUTS, {}, ()))
    out.append(Case('32-pair', problem('pair', 'float32', 0), {}, ('y', 'dx'), {}, ()))
    out.append(Case('32-dense', problem('dense', 'float32', 0), {}, ('y', 'dx'), {}, ()))
    d = make_dims(WIN_SHAPE[0], WIN_SHAPE[1], WIN_SHAPE[2], WIN_SHAPE[1], WIN_WIDTH, WIN_SHAPE[3], DENSE_N, 1, 1, 0,
                  WIN_WIDTH // 2)._replace(oh=1, ow=WIN_SHAPE[2])
    out.append(Case('32-windows', problem('windows', 'float32', 0), {}, ('y', 'dx'),
                    dict(y=expect_kernel(FWD, 'float32', d), dx=expect_kernel(DGRAD, 'float32', d)), ()))
    for i in range(len(TABLE)):
        out.append(_conv_case(problem('table', 'float16', i), {}, ''))
        out.append(_conv_case(problem('table', 'float16', i), {'h16': 0}, '-h16_0'))
    # the 4-channel binary16 upconv runs on conv_h16.hip with the phase-summed weights rounded to binary16
    out.append(Case('16-up4', problem('up', 'float16', 4), {}, CONV_OUTPUTS, {}, CONV_OUTPUTS))
    out.append(Case('16-up4-h16_0', problem('up', 'float16', 4), {'h16': 0}, CONV_OUTPUTS, {}, ()))
    out.append(Case('16-up1', problem('up', 'float16', 1), {}, CONV_OUTPUTS, {}, ()))
    out.append(Case('16-pair', problem('pair', 'float16', 0), {}, ('y',), {}, ('y',)))
    return tuple(out)


CASES = _cases()
CASE_IDS = [c.id for c in CASES]


# ---- mutations -------------------------------------------------------------------------------------------------------------
def constant_leak(a, ref, dtype):
    """a tenth of the rel_linf allowance, times max |ref|, added to every element"""
    return a + 0.1 * ALLOW[dtype] * np.abs(ref).max()


def sliding_residue(a, axis, k=5):
    """What a float32 running sum over k neighbours along `axis` (add the entering element, subtract the leaving one) has
    drifted from the same sum taken directly, per position: the residue a rolling register carries from a large region
    into a small one.  The walk starts at the end of the axis whose half holds the largest magnitude, so that it passes
    the large region first whatever the order of the strips."""
    p = np.moveaxis(np.asarray(a, dtype=np.float32), axis, -1)
    flip = np.abs(p).max(axis=tuple(range(p.ndim - 1))).argmax() >= p.shape[-1] / 2
    if flip:
        p = p[..., ::-1]
    p = np.concatenate([np.zeros(p.shape[:-1] + (k // 2,), np.float32), p, np.zeros(p.shape[:-1] + (k // 2,), np.float32)], -1)
    n = p.shape[-1] - (k - 1)
    out = np.zeros(p.shape[:-1] + (n,), np.float64)
    run = None
    for x in range(n):
        direct = p[..., x]
        for j in range(1, k):
            direct = direct + p[..., x + j]
        run = direct if x == 0 else (run + p[..., x + k - 1]) - p[..., x - 1]
        out[..., x] = run.astype(np.float64) - direct.astype(np.float64)
    return np.moveaxis(out[..., ::-1] if flip else out, -1, axis)


def sliding_axis(p, name):
    """the axis along which the regions of output `name` change"""
    if isinstance(p, DenseProblem):
        return 1 if name == 'y' else 0           # columns of w scale y's columns; rows of dy scale dx's rows
    if isinstance(p, WindowsProblem):
        return 0 if name == 'y' else 2           # y: (windows, outputs), one row per page column
    return 2


def worst_ratio(got, ref, tol, judged=None):
    """largest |got - ref| / tol over the judged elements (NaN counts as infinite)"""
    r = np.abs(np.asarray(got, dtype=np.float64) - ref) / tol
    r = np.where(np.isnan(r), np.inf, r)
    if judged is not None:
        r = r[np.broadcast_to(judged, r.shape)]
    return float(r.max())

