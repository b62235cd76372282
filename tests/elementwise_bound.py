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

Nothing here is measured and nothing is multiplied by a safety factor -- but for k, the error of expf in the Sigmoid
bound, which is measured (see "Sigmoid epilogues" below).  The reference is the float64 oracle on the
exact operands: every input is drawn representable in the storage type, so no input rounding enters.

The conv pair composes the bound through both layers (PairProblem.tolerances).  Three further bounds are derived where
their code stands: Sigmoid epilogues (SigmoidProblem), the Sigmoid derivative taken from a stored output
(FromOutputProblem) and the dx of the pair with every pixel judged (PairDxProblem).  The binary16 pair's weight
gradients, and the dx of its wave kernel, are judged against the kernel's own rounding points with every binary16
rounding as an interval (Pair16Steps, PairWaveDxProblem).

Inputs.  Magnitudes uniform in [0.25, 1] with a random sign (no zeros, no subnormals), times 2^e with e the sum of a
per-image, a per-8-row-band, a per-24-column-strip and a per-channel exponent.  8 and 24 do not divide the 16 / 32 /
64 tile edges of the kernels, so region borders fall on tile borders and inside tiles.  float32: |e| <= 9 + 8 + 10 + 6
= 33.  binary16: image, band and channel 1 each, and the strips all that the normal range [2^-14, 65504] leaves (8, |e|
<= 11, weights without a channel exponent: `fit16`); `Problem.check_ranges` asserts that every stored input and every S
lies in that range.

The weight gradients (dw, db) have a module of their own on top of this one, elementwise_wgrad.py: smaller pages (gamma
grows with the pixels a weight gradient sums), tol = gamma(n + 8) S + u32 |init + ref|.
"""
import copy
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
    scale = {}                      # {operand: one more exponent for the whole tensor} (`rescaled`)

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
        for k, e in self.scale.items():
            q[k] = q[k] * 2.0 ** e
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

    def bias_term(self):
        return self.q['b'] if self.bias else 0.0

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

    def bias_term(self):
        return self.q['b']

    def abs_sums(self):
        a = {k: np.abs(v) for k, v in self.q.items()}
        sy, sdx = self._up(a['x'], a['w'], a['b'], a['g'])
        ny, ndx = 25 * self.ch, 4 * 25 * self.ch                 # dx: the 2 x 2 high-resolution pixels of one source pixel
        return dict(y=(sy, ny), y_leaky=(sy, ny), dx=(sdx, ndx), dx_leaky=(sdx * slope_of(self.q['m']), ndx))


class PairProblem(Problem):
    """conv3x3(1 -> 16) + LeakyReLU + conv3x3(16 -> 1), act2 none: y, and (float32) dx"""
    stored = ('x', 'g')
    weights = ('w1', 'w2')

    def __init__(self, name, dtype, seed, shape=SHAPE, fit=None, pad1=None):
        super().__init__(name, dtype, seed, fit)
        self.shape = shape
        self.pad1 = (0.0 if self.half else 0.25) if pad1 is None else pad1

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

    def bias_term(self):
        return self.q['b2']

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
            out[op] = tol, judged, s1, e2
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


class PairFaintProblem(PairProblem):
    """binary16 inputs for the pair's dx with every pixel judged.  A LeakyReLU slope the kernel may take otherwise than the
    oracle (w1 is rounded) moves a dx pixel by up to (1 - alpha) |ga1 w1|; that stays far below max |dx| only if dy is small
    wherever slopes are contested.  Here dy carries the exponents of x NEGATED (large where the page is faint; the
    brightest exponent of the 5 x 5 neighbourhood, which is what reaches z1 and ga1 of a pixel), and b1 is 2^[B1_SHIFT
    - 2, B1_SHIFT]: where |x| 9 max |w1| stays below it z1 has the sign of b1 and no rounding of w1 decides a slope; in
    the brighter regions z1 cancels as anywhere.  Powers of two: x 2^[-13, 11] (strips 2^(+-8)), w1 2^-3 and w2 2^-5
    times [0.25, 1] and 2^(+-2) per channel (few channels carry a dx pixel: with sixteen alike the sum of 144 terms
    averages a wrong d_a1 away), dy 2^(2 - e)."""
    W1_SHIFT, W2_SHIFT, B1_SHIFT, G_SHIFT = -3, -5, 5, 2
    LIMITS = dict(image=1, band=1, strip=8, channel=1)

    def draw(self, rng):
        n, h, w = self.shape
        e = region_exponents(rng, (n, h, w, 1), self.LIMITS)
        pad = np.pad(e, ((0, 0), (2, 2), (2, 2), (0, 0)), mode='edge')
        near = np.max([pad[:, i:i + h, j:j + w] for i in range(5) for j in range(5)], axis=0)
        return dict(x=signed_unit(rng, (n, h, w, 1), self.dtype) * 2.0 ** e,
                    w1=scaled_weights(rng, (3, 3, 1, 16), 'float32', self.W1_SHIFT),
                    b1=signed_unit(rng, (16,), 'float32') * 2.0 ** self.B1_SHIFT,
                    w2=scaled_weights(rng, (3, 3, 16, 1), 'float32', self.W2_SHIFT), b2=scaled_bias(rng, 1, self.dtype),
                    g=signed_unit(rng, (n, h, w, 1), self.dtype) * 2.0 ** (self.G_SHIFT - near))


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

    def bias_term(self):
        return 0.0                               # the bias is a row of w and scales with it

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


# ---- Sigmoid epilogues -------------------------------------------------------------------------------------------------------
# y = Sigmoid(v) after a linear kernel.  The kernel's pre-activation v^ lies within E = (operand_u + gamma(n + 8)) S of
# the oracle's v (the bound above; for the pair the composed one); it then evaluates 1.f / (1.f + expf(-v^)).
#
#   tol = E sigma'(max(0, |v| - E)) + sigma ((1 - sigma) k u + 2 u) + 2^-126 [+ 2^-11 |ref| + 2^-25, binary16 store]
#
#   inherited  |sigma(v^) - sigma(v)| <= |v^ - v| max sigma' over [v - E, v + E]; sigma' = sigma (1 - sigma) <= 1/4 is even
#              and decreases in |v|, so its largest value on the interval is the one at the point nearest 0;
#   own        e = expf(-v^) (1 + d1), |d1| <= k u; d = (1 + e)(1 + d2), y = (1 / d)(1 + d3), |d2|, |d3| <= u.  To first
#              order y = sigma (1 - (1 - sigma) d1 - d2 + d3) since e / (1 + e) = 1 - sigma: sigma ((1 - sigma) k u + 2 u);
#   floor      2^-126, the smallest normal float32: for v^ < -88.72 expf(-v^) is inf and the result exactly 0, and a
#              result below the normal range may be flushed;
#   k          SIGMOID_K.  build.sh passes no fast-math flag, so expf is the library's; a ROCm installation carries no
#              table of the ULP errors of HIP's maths functions, so k is measured: tools/bench_sigmoid_ulp.py evaluates
#              uocr_act_fwd(SIGMOID) -- the same expression with the same expf, no conv kernel -- on 2^23 + 1 equidistant
#              and 2^23 random v in [-90, 90] and 2^23 v of all magnitudes 2^-21 .. 1 against float64: the largest relative
#              error of the Sigmoid is 2.61 u (at v = -16.74); k = ceil(2 x 2.61) = 6, the factor 2 for the inputs the grid
#              misses.  (That figure holds the two roundings after expf too, so k is on the safe side by up to 4.)
#              The binary16 kernels (conv_h16.hip, conv_pair_strip_h.hip) and the float32 strip kernel take v_exp_f32 of
#              -v^ log2 e and v_rcp_f32 instead (1 ulp = 2 u each, and the scaled argument moves e by <= 2 |v^| u < E): they
#              are judged by the same bound.
#
# Inputs.  The operands of the linear problem, with the last weights (w; the pair: w2) times the power of two 2^d that
# `sigmoid_shift` finds by trying: the regions keep their spread, so v is of order one in some and saturates either way in
# others (SigmoidProblem.check_inputs states what the host test asserts).
SIGMOID_K = 6
TINY32 = 2.0 ** -126            # smallest normal float32
V_INF32 = -88.72                # below this expf(-v) is inf in float32 (ln(2^128) = 88.7228)
TINY16 = 2.0 ** -24             # smallest binary16 subnormal


def sigmoid(v, dt=np.float64):
    """float64: the oracle's Sigmoid, evaluated without cancellation on either side; float32: the kernels' expression"""
    if dt is np.float64:
        e = np.exp(-np.abs(np.asarray(v, dtype=np.float64)))
        return np.where(np.asarray(v) >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
    assert v.dtype == np.float32
    with np.errstate(over='ignore'):
        return (np.float32(1) / (np.float32(1) + np.exp(-v))).astype(np.float32)


def sigmoid_tolerance(v, e, store16=False, k=None):
    """the tolerance of Sigmoid(v^), |v^ - v| <= e, derived above"""
    k = SIGMOID_K if k is None else k
    s, c = sigmoid(v), sigmoid(-np.asarray(v, dtype=np.float64))         # sigma and 1 - sigma
    m = np.maximum(0.0, np.abs(v) - e)
    tol = e * sigmoid(m) * sigmoid(-m) + s * (c * k * U32 + 2 * U32) + TINY32
    return tol + (U16 * s + FLOOR16 if store16 else 0.0)


def sigmoid_score(v):
    """the smallest of the three shares the inputs must reach, each over its requirement (>= 1: all reached)"""
    return min(np.mean(np.abs(v) <= 4) / 0.30, np.mean(v >= 20) / 0.05, np.mean(v <= -20) / 0.05)


def sigmoid_shift(linear, bias, half, lo=-40, hi=40):
    """the exponent d in [lo, hi] for which v = 2^d linear + bias spreads best over the Sigmoid (largest sigmoid_score)
    among those where some v makes the float32 expf overflow (binary16: where some output lies below the subnormals)"""
    best = None
    for d in range(lo, hi + 1):
        v = 2.0 ** d * linear + bias
        if v.min() >= (np.log(TINY16) if half else V_INF32):
            continue
        score = sigmoid_score(v)
        if best is None or score > best[0]:
            best = score, d
    assert best is not None and best[0] >= 1.0, best
    return best[1]


def rescaled(p, scale):
    """a copy of problem `p` whose operands named in `scale` carry that exponent more"""
    c = copy.copy(p)
    for k in ('q', 'ref', 'sums', '_composed'):
        c.__dict__.pop(k, None)
    c.scale = dict(scale)
    return c


class SigmoidProblem(Problem):
    """y_sigmoid = Sigmoid(y of `base` with its last weights times 2^d): `inner` is that linear problem"""

    def __init__(self, base):
        super().__init__(base.name + '-sigmoid', base.dtype, base.seed)
        self.base = base
        self.last = 'w2' if isinstance(base, PairProblem) else 'w'

    @functools.cached_property
    def shift(self):
        p = self.base
        bias = p.bias_term()
        lo, hi = -40, 40
        if self.half:           # a binary16 kernel may round the weights: they stay in the normal range
            a = np.abs(p.q[self.last])
            lo, hi = int(np.ceil(np.log2(F16_MIN / a.min()))), int(np.floor(np.log2(F16_MAX / a.max())))
        return sigmoid_shift(p.ref['y'] - bias, bias, self.half, lo, hi)

    @functools.cached_property
    def inner(self):
        return rescaled(self.base, {self.last: self.shift})

    @property
    def q(self):
        return self.inner.q

    @property
    def v(self):
        return self.inner.ref['y']

    @functools.cached_property
    def ref(self):
        out = dict(y_sigmoid=sigmoid(self.v))
        out['y_sigmoid'].setflags(write=False)
        return out

    def restated(self, store=True, act=sigmoid):
        """float32 restatement: the linear problem's, then `act` (the kernels' expression unless a mutant is given)"""
        p = self.inner
        v = p.run(p.cast(p.q, np.float32), np.float32)['y']
        y = act(v, np.float32)
        assert v.dtype == np.float32 and y.dtype == np.float32
        return dict(y_sigmoid=r16(y) if self.half and store else y.astype(np.float64))

    def pre_error(self, operand16=()):
        """E: the bound of the linear kernel on v"""
        op = 'y_sigmoid' in operand16
        if isinstance(self.inner, PairProblem):
            return self.inner._composed[op][3]
        s, n = self.inner.sums['y']
        return ((U16 if op else 0.0) + gamma(n + SLACK)) * s

    def tolerances(self, operand16=(), store=True):
        """store=False: without the terms of the binary16 store"""
        return dict(y_sigmoid=sigmoid_tolerance(self.v, self.pre_error(operand16), self.half and store))

    def check_ranges(self):
        """binary16: the stored inputs and the weights a kernel may round lie in the normal range (v is never stored)"""
        if not self.half:
            return
        p = self.inner
        for k in p.stored + (self.last,):
            a = np.abs(p.q[k])
            assert F16_MIN <= a.min() and a.max() <= F16_MAX, (self.name, k, a.min(), a.max())
        for k in p.stored:
            assert np.array_equal(r16(p.q[k]), p.q[k]), (self.name, k)
        if isinstance(p, PairProblem):
            s1 = p._composed[True][2]
            assert F16_MIN <= s1.min() and s1.max() <= F16_MAX, (self.name, s1.min(), s1.max())

    def check_inputs(self):
        """what the Sigmoid inputs must offer; returns the figures"""
        v = self.v
        mid, hi, lo = float(np.mean(np.abs(v) <= 4)), float(np.mean(v >= 20)), float(np.mean(v <= -20))
        assert mid >= 0.30 and hi >= 0.05 and lo >= 0.05, (self.name, mid, hi, lo)
        if self.half:
            assert self.ref['y_sigmoid'].min() < TINY16, (self.name, v.min())
        else:
            assert v.min() < V_INF32, (self.name, v.min())
        # the regions keep their spread: the operands are the linear problem's but for one power of two, and over the
        # regions along the axis the magnitudes vary on (strips; rows or columns of a GEMM) the median |v| is of order one
        # in one and saturates in another
        for k, a in self.base.q.items():
            assert np.array_equal(self.q[k], a * 2.0 ** (self.shift if k == self.last else 0)), (self.name, k)
        med = self.region_medians()
        assert med.min() <= 4 and med.max() >= 20, (self.name, med)
        return dict(mid=mid, high=hi, low=lo, vmin=float(v.min()), vmax=float(v.max()), shift=self.shift,
                    median_min=float(med.min()), median_max=float(med.max()))

    def region_medians(self):
        """median |v| per region: per (image, band, strip) of x, taken to the output's geometry; dense: per column of w"""
        a = np.abs(self.v)
        if a.ndim == 2:
            return np.median(a, axis=0)
        x = self.q['x'].shape
        rows, cols = (max(1, round(r * a.shape[i] / x[i])) for i, r in ((1, BAND), (2, STRIP)))
        return np.array([np.median(a[n, i:i + rows, j:j + cols]) for n in range(a.shape[0])
                         for i in range(0, a.shape[1], rows) for j in range(0, a.shape[2], cols)])


# ---- the Sigmoid derivative taken from the output ---------------------------------------------------------------------------
# uocr_act_bwd_from_output and uocr_seg_loss(out_act = SIGMOID) multiply by y (1 - y) of a STORED y.  The reference is
# the same expression in float64 on that same y, so nothing is inherited:
#
#   act_bwd_from_output   dx = dy y (1 - y):   tol = 3 u |ref| + 2^-126 [+ 2^-11 |ref| + 2^-25]
#                         one float32 subtraction and two products: (1 + d)^3, and a result below the normal range may
#                         be flushed (y = 0 and y = 1 give exactly 0 on both sides);
#   seg_loss              grad = (ca g + cb) y (1 - y) 2^k with the oracle's Dice / Jaccard coefficients ca, cb per (image,
#                         channel) and k the power of two of a binary16 gradient.  seg_grad_vec_kernel rounds ca and cb to
#                         float32 (one rounding each) and applies them with one FMA:
#                         tol = 3 u |ref| + u (|ca g| + |cb| + |ca g + cb|) y (1 - y) 2^k + 2^-126 [+ store terms].
#                         The generic kernel (c = 3, or a size that is no multiple of 16 bytes) works in float64 and is
#                         judged by the same bound.
#
# Inputs: y uniform in (0, 1), representable, but for one element in eight, which is (in turn) exactly 0, exactly 1,
# within 2^-12 of 0 and within 2^-12 of 1 (binary16 has no number strictly between 1 - 2^-11 and 1: there the last kind
# is 1 - 2^-11, its nearest); labels 0 / 1; dy: magnitudes [0.25, 1] 2^[-8, 8] per element.
SEG_SHAPES = ((2, 64, 130), (3, 37, 141))       # hw c elem: a multiple of 16 for c elem = 2 .. 16; only for c elem = 16
SEG_EPS = 1e-8                                  # the oracle's EPS_LOSS


def sigmoid_outputs(rng, shape, dtype):
    """stored Sigmoid outputs with the edge values of the comment above"""
    y = rng.uniform(0.0, 1.0, shape).astype(STORE[dtype]).astype(np.float64)
    y = np.clip(y, 2.0 ** -14, 1.0 - U16)               # (the edges come from the list below alone)
    near = 2.0 ** -12 * rng.uniform(0.25, 1.0, shape)
    below_one = 1.0 - near if dtype == 'float32' else np.full(shape, 1.0 - U16)
    kind = rng.integers(0, 32, shape)
    y = np.select([kind == 0, kind == 1, kind == 2, kind == 3], [0.0, 1.0, near, below_one], y)
    return y.astype(STORE[dtype]).astype(np.float64)


class FromOutputProblem(Problem):
    """dx = dy y (1 - y) (kind 'act') or the Dice / Jaccard gradient times y (1 - y) (kind 'dice' / 'jaccard')"""

    def __init__(self, kind, dtype, seed, shape, c):
        super().__init__(f'{kind}-{shape[1]}x{shape[2]}x{c}', dtype, seed)
        self.kind, self.shape = kind, (*shape, c)

    def draw(self, rng):
        q = dict(y=sigmoid_outputs(rng, self.shape, self.dtype))
        if self.kind == 'act':
            q['dy'] = (signed_unit(rng, self.shape, self.dtype) * 2.0 ** rng.integers(-8, 9, self.shape))
        else:
            q['gt'] = (rng.random(self.shape) < 0.3).astype(np.float64)
        return q

    @property
    def gscale(self):
        """log2 of the factor of a binary16 loss gradient (ops.f16_grad_scale_log2)"""
        if self.kind == 'act' or not self.half:
            return 0
        return max(0, min(24, int(np.floor(np.log2(self.shape[1] * self.shape[2]))) - 4))

    def coefficients(self, q, dt=np.float64):
        """(ca, cb): the loss gradient is ca gt + cb, per (image, channel); float64 as both kernels compute them"""
        y, g = np.asarray(q['y'], dtype=np.float64), np.asarray(q['gt'], dtype=np.float64)
        num = (y * g).sum(axis=(1, 2), keepdims=True) + SEG_EPS
        if self.kind == 'dice':
            den = y.sum(axis=(1, 2), keepdims=True) + g.sum(axis=(1, 2), keepdims=True) + 2 * SEG_EPS
            ca, cb = -2.0 / den, 2.0 * num / den ** 2
        else:
            den = y.sum(axis=(1, 2), keepdims=True) + g.sum(axis=(1, 2), keepdims=True) - num + 2 * SEG_EPS
            ca, cb = -(den + num) / den ** 2, num / den ** 2
        return (ca * 2.0 ** self.gscale).astype(dt), (cb * 2.0 ** self.gscale).astype(dt)

    def run(self, q, dt, slope=None):
        """slope: what a mutant takes for y (1 - y)"""
        y = q['y']
        slope = y * (dt(1) - y) if slope is None else slope(y)
        if self.kind == 'act':
            return dict(dx=q['dy'] * slope)
        if dt is np.float64:
            loss = O.dice_loss if self.kind == 'dice' else O.jaccard_loss
            return dict(dx=loss(q['y'], q['gt'])[1] * slope * 2.0 ** self.gscale)
        ca, cb = self.coefficients(q, dt)
        return dict(dx=(ca * q['gt'] + cb) * slope)          # (NumPy rounds the product: one rounding more than the FMA)

    def tolerances(self, operand16=(), store=True):
        ref, y = np.abs(self.ref['dx']), self.q['y']
        tol = 3 * U32 * ref + TINY32
        if self.kind != 'act':
            ca, cb = self.coefficients(self.q)
            tol = tol + U32 * (np.abs(ca * self.q['gt']) + np.abs(cb) + np.abs(ca * self.q['gt'] + cb)) * y * (1.0 - y)
        return dict(dx=tol + (U16 * ref + FLOOR16 if self.half and store else 0.0))

    def mutated(self):
        """the float32 restatement with y (1 - y) from a y rounded once more to binary16 -- binary16 tensors, whose y is
        binary16 already: with 1 - y rounded to binary16 -- stored"""
        h = lambda a: a.astype(np.float16).astype(np.float32)
        slope = (lambda y: y * h(np.float32(1) - y)) if self.half else (lambda y: h(y) * (np.float32(1) - h(y)))
        out = self.run(self.cast(self.q, np.float32), np.float32, slope)['dx']
        assert out.dtype == np.float32
        return r16(out) if self.half else out.astype(np.float64)

    def check_inputs(self):
        y = self.q['y']
        assert np.array_equal(y.astype(STORE[self.dtype]).astype(np.float64), y) and y.min() == 0.0 and y.max() == 1.0
        assert ((y > 0) & (y <= 2.0 ** -12)).any() and ((y < 1) & (1 - y <= (U16 if self.half else 2.0 ** -12))).any()
        if self.kind == 'act':
            return
        n, h, w, c = self.shape
        size = h * w * c * (2 if self.half else 4)
        assert h * w <= 64 * 130 and set(np.unique(self.q['gt'])) == {0.0, 1.0}
        return size % 16 == 0 and c in (1, 2, 4)             # whether seg_grad_vec_kernel takes the call

    def check_ranges(self):
        pass


# ---- dx of the conv pair with every pixel judged ------------------------------------------------------------------------------
# pair_strip_bwd_h_kernel (conv_pair_strip_h.hip; one block of waves spans pages up to 512 columns) rounds to binary16:
# w1 and w2 (the MFMA's B operands), g = dy y (1 - y) where act2 is a Sigmoid (one rounding of the float32 product), d_a1
# = ga1 * slope (once, into the transpose scratch) and dx (the store).  b1 is NOT rounded: it is the float32 accumulator
# the first MFMA starts from (the "ones" copy of the x ring serves db1 alone).  a1 is rounded too but enters dw2 only.
# The slope is the sign of the kernel's float32 z1.
#
#   z1'   = conv(x, r16(w1)) + b1 in exact arithmetic: the kernel's z1 up to float32 accumulation, e1' = gamma(9 + 8) S1',
#           S1' = conv(|x|, |r16(w1)|, |b1|).  A slope is DECIDED where |z1'| > e1'.
#   ref   = the oracle with the exact weights.  Where the decided slope equals the oracle's the composed bound stands:
#           Ega = (op_n + gamma(9 + 8) [+ 3 u]) Sga [+ 2^-25 sum |w2|] bounds ga1 = dgrad(g, w2), op_n = 2^-11 per rounded
#           operand (w2; g under a Sigmoid, whose float32 product y (1 - y) dy is the + 3 u and whose binary16 rounding
#           below the normal range the 2^-25); Egz = slope Ega + op (|gz1| + slope Ega) + 2^-25 (d_a1 rounded once);
#           tol = dgrad(Egz, |w1|) + (op + gamma(144 + 8)) dgrad(|gz1| + Egz, |w1|) + store terms.
#   flips   where z1' is undecided, or decided with another slope than the oracle's z1, the kernel may take the other
#           slope: d_a1 moves by at most (1 - alpha)(|ga1| + Ega), and every dx pixel that (position, channel) reaches gains
#           (1 - alpha)(|ga1| + Ega) |w1[tap]|.  No pixel is left out; test_elementwise_bound_host.py caps the widened
#           pixels at 5 % and their tolerance at 1/16 of what rel_linf allows.
# float32 (op = 0: z1' = z1, only undecided slopes widen) is judged by the same rule, beside the exclusion rule above.
# Pages wider than 512 columns run pair_wave_bwd_h_kernel, which takes LeakyReLU on packed binary16 (z1 and ga1 rounded
# first, alpha rounded to binary16, a binary16 product): other rounding points, judged by another rule -- "The binary16
# pair at its own roundings" below (PairWaveDxProblem).
PAIR_SHAPES = (SHAPE, (2, 21, 128), (2, 19, 71))     # 141, 71: ragged (MODE 1); 128 = two whole waves (MODE 0 at pad1 = 0)


class PairDxProblem(Problem):
    """dx of conv_pair_bwd on the operands of `base` (a PairProblem); sig: act2 is a Sigmoid and the kernel reads the stored
    output `yout`"""
    stored = ('x', 'g', 'yout')

    def __init__(self, base, sig):
        super().__init__(f'{base.name}-dx' + ('-sigmoid' if sig else ''), base.dtype, base.seed)
        self.base, self.sig, self.pad1 = base, sig, base.pad1

    def dgrad(self, g, w, pad=0.0):
        """gradient of a 3x3 conv (padding 1) with respect to its input (the input enters through its shape alone)"""
        return O.conv2d_bwd(np.zeros(g.shape[:3] + (w.shape[2],), g.dtype), w, g, 1, 1, g.dtype.type(pad), True)[0]

    @functools.cached_property
    def q(self):
        b = self.base
        q = dict(b.q)
        # yout is data to the backward kernel: under a Sigmoid stored outputs with the edge values of sigmoid_outputs
        # (0, 1 and their neighbours), else the stored output of the layers (never read)
        out = sigmoid_outputs(np.random.default_rng(self.seed + 7), q['x'].shape, self.dtype) if self.sig \
            else b._layers(q, np.float64)[2]
        q['yout'] = out.astype(STORE[self.dtype]).astype(np.float64)
        for a in q.values():
            a.setflags(write=False)
        return q

    def g_eff(self, q, dt, rnd=lambda a: a):
        if not self.sig:
            return q['g']
        return rnd(q['g'] * (q['yout'] * (dt(1) - q['yout'])))

    def run(self, q, dt):
        """the oracle: exact weights, the slope of its own z1"""
        z1 = O.conv2d_fwd(q['x'], q['w1'], q['b1'], 1, 1, dt(self.pad1), True)
        ga1 = self.dgrad(self.g_eff(q, dt), q['w2'])
        return dict(dx=self.dgrad(ga1 * slope_of(z1, dt), q['w1']))

    def kernel_steps(self, q, dt, mutate=None):
        """the kernel's rounding points in `dt` arithmetic -> (z1', ga1', d_a1', dx'); mutate(stage, value) -> value lets a
        mutant change 'slope', 'd_a1' or 'dx'"""
        mutate = mutate or (lambda stage, value: value)
        rnd = (lambda a: a.astype(np.float16).astype(dt)) if self.half else (lambda a: a)
        w1, w2 = rnd(q['w1']), rnd(q['w2'])
        z1 = O.conv2d_fwd(q['x'], w1, q['b1'], 1, 1, dt(self.pad1), True)
        ga1 = self.dgrad(self.g_eff(q, dt, rnd), w2)
        d = mutate('d_a1', rnd(ga1 * mutate('slope', slope_of(z1, dt))))
        return z1, ga1, d, mutate('dx', self.dgrad(d, w1))

    def restated(self, store=True, mutate=None):
        dx = self.kernel_steps(self.cast(self.q, np.float32), np.float32, mutate)[3]
        assert dx.dtype == np.float32
        return dict(dx=r16(dx) if self.half and store else dx.astype(np.float64))

    @functools.cached_property
    def parts(self):
        q, a = self.q, {k: np.abs(v) for k, v in self.q.items()}
        op = U16 if self.half else 0.0
        z1 = O.conv2d_fwd(q['x'], q['w1'], q['b1'], 1, 1, self.pad1, True)
        z1p = self.kernel_steps(q, np.float64)[0]
        w1r = np.abs(r16(q['w1'])) if self.half else a['w1']
        e1p = gamma(9 + SLACK) * O.conv2d_fwd(a['x'], w1r, a['b1'], 1, 1, abs(self.pad1), True)
        decided = np.abs(z1p) > e1p
        flip = ~decided | (slope_of(z1p) != slope_of(z1))
        g = self.g_eff(q, np.float64)
        ga1, sga = self.dgrad(g, q['w2']), self.dgrad(np.abs(g), a['w2'])
        ega = (op * (2 if self.sig else 1) + gamma(9 + SLACK) + (3 * U32 if self.sig else 0.0)) * sga
        if self.sig and self.half:
            ega = ega + FLOOR16 * self.dgrad(np.ones(g.shape), a['w2'])
        sl = slope_of(z1)
        gz1 = np.abs(ga1 * sl)
        egz = ega * sl + op * (gz1 + ega * sl) + (FLOOR16 if self.half else 0.0)
        tol = self.dgrad(egz, a['w1']) + (op + gamma(144 + SLACK)) * self.dgrad(gz1 + egz, a['w1']) + TINY32
        widen = self.dgrad(flip * (1.0 - ALPHA) * (np.abs(ga1) + ega), a['w1'])
        return dict(z1=z1, z1p=z1p, e1p=e1p, decided=decided, flip=flip, ga1=ga1, ega=ega, base_tol=tol, widen=widen)

    def tolerances(self, operand16=(), store=True):
        t = self.parts
        return dict(dx=t['base_tol'] + t['widen'] + (self.store_part('dx') if store else 0.0))

    @property
    def widened(self):
        return self.parts['widen'] > 0

    def check_ranges(self):
        if not self.half:
            return
        for k in self.stored:
            a = np.abs(self.q[k])
            assert np.array_equal(r16(self.q[k]), self.q[k]) and a.max() <= F16_MAX, (self.name, k)
            assert k == 'yout' or F16_MIN <= a.min(), (self.name, k, a.min())
        self.base.check_ranges()
        a = {k: np.abs(v) for k, v in self.q.items()}
        sdx = self.dgrad(self.dgrad(a['g'], a['w2']), a['w1'])
        assert sdx.max() <= F16_MAX, (self.name, sdx.max())


# ---- the binary16 pair at its own roundings: roundings as intervals ----------------------------------------------------------
# The composed bounds above compare with an oracle that rounds nowhere, so every binary16 rounding costs 2^-11 of an
# operand: too loose for the weight gradients, and not the wave kernel's arithmetic at all.  Here the reference is the
# KERNEL'S OWN sequence of roundings, restated stage by stage in float64 on the stored binary16 x, dy, yout and the
# float32 parameters (Pair16Steps), and a binary16 rounding of a value the kernel computes in float32 is an INTERVAL:
#
#   a float32-computed value has an exact-arithmetic value v' and a derived bound e:
#     z1   z' = conv(x, r16(w1)) + b1 (padding value r16(pad1)), e = gamma(9 + 8) conv(|x|, |r16(w1)|, |b1|, |r16(pad1)|);
#     g    act2 none: dy itself.  Sigmoid: g' = dy (y (1 - y)) (exact in float64: 11 x 24 x 11 bits), e = 3 u32 |g'| for
#          `gf * (yf * (1.f - yf))`;
#     s    = dgrad(g, r16(w2)): with g in [g_lo, g_hi] the exact value lies in dgrad(mid, r16(w2)) -+ dgrad(rad, |r16(w2)|),
#          and e = gamma(9 + 8) dgrad(max(|g_lo|, |g_hi|), |r16(w2)|) on top;
#   where the kernel rounds it to binary16 the restatement carries [r16(v' - e), r16(v' + e)]: rounding, a product with a
#   non-negative constant and LeakyReLU are monotone, so the endpoints bound every outcome.  At most positions the
#   endpoints coincide -- the kernel's value is KNOWN, bit for bit -- elsewhere the element is contested and the interval
#   one binary16 step wide.  A slope is contested where the two endpoints of z take different slopes; d_a1 then takes the
#   hull over both.  The reference is the restatement at the nominal values (e = 0).
#
# The two kernels round at different points (conv_pair_strip_h.hip):
#   strip  pair_strip_bwd_h_kernel (one cooperative block, width <= 512): `slope = z >= 0.f ? 1.f : alpha` on the float32
#          z (line 233), a = z * slope and d = s * slope in float32 with the float32 alpha, ONE rounding of each product
#          (pack4h, lines 247-249).  (The float32 rounding of the product before it is one of the + 8.)
#   wave   pair_wave_bwd_h_kernel (independent waves, width > 512), lines 538-607: zb = cvt2h(z) and sb = cvt2h(s) FIRST;
#          the slope is the SIGN BIT of zb (neg_halves: a z that rounds to -0 takes alpha); a1 = zb * slope16 and d = sb *
#          slope16 are binary16 products (mul2h) with alpha16 = (_Float16)alpha -- 0.010002, not 0.01.
#   both   w1, w2 `(_Float16)`; z1 a float32 MFMA started from the float32 b1; pad1 enters as half_bits(pad1); g =
#          half_bits(gf * (yf * (1.f - yf))) under a Sigmoid; dw1 / dw2 / db1 are float32 MFMA sums of products of two
#          binary16 numbers (exact in float32; db1 through the ones column of the x ring), db2 a float32 fdot2 sum, the
#          unscale by 2^-k is exact.  Hence, n = N H W, wgrad / dgrad the oracle's operators, width = hi - lo, max = the
#          larger endpoint magnitude:
#   dw2    tol = wgrad(width(a1), |g|max) + wgrad(|a1|max, width(g)) + gamma(n + 8) wgrad(|a1|max, |g|max)
#   dw1    tol = wgrad(|x|, width(d_a1)) + gamma(n + 8) wgrad(|x|, |d_a1|max), |r16(pad1)| in the border; db1: ones for x
#   db2    tol = sum width(g) + gamma(n + 8) sum |g|max
#   dx     (wave kernel; the strip kernel's dx keeps PairDxProblem) ref = dgrad(d_a1, r16(w1)) at the nominal values,
#          tol = dgrad(width(d_a1), |r16(w1)|) + gamma(144 + 8) dgrad(|d_a1|max, |r16(w1)|) + 2^-11 |ref| + 2^-25
# Nothing is measured, no term carries a safety factor, no element is left out.  (binary16 arithmetic keeps subnormals
# on gfx950 -- the kernels are built without a flush flag -- and r16 rounds into them as the hardware does.)
#
# Inputs (PairSpreadProblem).  dw1 / db1 scale with |w2[ch]|, dw2 with |w1[ch]| and |b1[ch]|: w1 (b1 follows its channel,
# |b1| ~ 2 |w1|: many channels keep one sign of z1 over the page, so few slopes are contested) and w2 carry per-channel
# exponents 2^(+-5) (`channel_spread`: both ends occur, as neighbours), x mild region exponents (image, strip: 1 each) and dy the same
# NEGATED.  dy is stored times the largest 2^k under which dy, d_a1 and dx all stay finite (k > 0 is asserted); x, 2^k
# dy, r16(w1), r16(w2) lie in the normal range, and so do the magnitude sums of a1, d_a1 and dx (act2 none; a Sigmoid
# scales g by y (1 - y) down to exactly 0, there only the upper end is asserted).
#
# Host figures for dx (test_elementwise_bound_host.py; elementwise_wgrad.py has those of the weight gradients): the float32
# restatement is itself a correct kernel and takes the other endpoint of a few contested roundings (6 and 65 of 6 471 and 4 526
# at (2, 11, 600)); there its error IS the widening, up to 0.81 of that pixel's tolerance.  Beyond what the widening explains it uses
# at most 0.011 of the rest (asserted <= 0.5); rounded once to binary16 it reaches 0.87 .. 0.96 of the whole (the store:
# asserted <= 1).  The widening exceeds the arithmetic and store terms on 0.6 .. 3.0 % of the pixels (cap 5 %).  The strip
# kernel's slope-and-product rule and an unrounded alpha are rejected at 1.1 .. 10 and 1.1 .. 11 tolerances.
# On the MI355X the largest err / tol of the wave kernel's dx was 0.955 at (2, 11, 600) and 0.935 at (1, 3, 560), equal to
# the stored host restatement's to three digits, under every band and pair_g setting, with and without accumulation.
A16, A32 = float(np.float16(ALPHA)), float(np.float32(ALPHA))    # alpha as the wave kernel / the strip kernel multiplies by it
PAIR16_LIMITS = dict(image=1, band=0, strip=1, channel=0)
WIDEN_CAP = 0.05                                # share of an output's elements whose widening may exceed the arithmetic part
PAIR16_CH = 5                                   # largest |channel exponent| of w1 (and b1) and of w2
PAIR16_W1_SHIFT, PAIR16_W2_SHIFT = 5, -7        # w1 2^[-2, 10] (a1 keeps alpha |z1| normal), r16(w2) 2^[-14, -2]


def wgrad(x, g, ksize, stride=1, padding=0, pad_value=0.0, bias=True):
    """(dw, db) of the oracle's conv for input x and output gradient g (the weights enter through their shape alone)"""
    w = np.zeros((*ksize, x.shape[3], g.shape[3]), x.dtype)
    return O.conv2d_bwd(x, w, g, stride, padding, x.dtype.type(pad_value), bias)[1:]


def dgrad3(g, w, pad=0.0):
    """gradient of a 3x3 conv (padding 1) with respect to its input (the input enters through its shape alone)"""
    return O.conv2d_bwd(np.zeros(g.shape[:3] + (w.shape[2],), g.dtype), w, g, 1, 1, g.dtype.type(pad), True)[0]


def h16(a, dt):
    return np.asarray(a).astype(np.float16).astype(dt)


def pair16_leaky(kernel, z, dt):
    """(a1, the positions that take alpha) as kernel `kernel` derives them from its float32 z, in `dt` arithmetic"""
    if kernel == 'wave':
        zb = h16(z, dt)
        neg = np.signbit(zb)
        return np.where(neg, h16(zb * dt(A16), dt), zb), neg
    neg = ~(z >= 0)
    return h16(np.where(neg, z * dt(A32), z).astype(dt), dt), neg


def pair16_masked(kernel, s, neg, dt, alpha=None):
    """d_a1 from the kernel's float32 s = dgrad(g, w2); alpha: what a mutant of the wave kernel multiplies by"""
    if kernel == 'wave':
        sb = h16(s, dt)
        return np.where(neg, h16((sb * dt(A16 if alpha is None else alpha)).astype(dt), dt), sb)
    return h16(np.where(neg, s * dt(A32), s).astype(dt), dt)


def channel_spread(rng, count, limit):
    """`spread` with the channel of the smallest exponent moved right behind the one of the largest: one pair of
    neighbouring channels differs by 2^(2 limit), whatever the seed"""
    e = spread(rng, count, limit)
    i, j = int(np.argmax(e)), int(np.argmin(e))
    k = (i + 1) % count
    e[j], e[k] = e[k], e[j]
    return e


class PairSpreadProblem(Problem):
    """binary16 inputs of the pair whose CHANNELS differ by many powers of two (the comment above)"""
    stored = ('x', 'g')

    def __init__(self, name, seed, shape, pad1):
        super().__init__(name, 'float16', seed)
        self.shape, self.pad1 = shape, pad1

    def draw(self, rng):
        n, h, w = self.shape
        e = region_exponents(rng, (n, h, w, 1), PAIR16_LIMITS)
        c1, c2 = channel_spread(rng, 16, PAIR16_CH), channel_spread(rng, 16, PAIR16_CH)
        return dict(x=signed_unit(rng, (n, h, w, 1), 'float16') * 2.0 ** e,
                    w1=signed_unit(rng, (3, 3, 1, 16), 'float32') * 2.0 ** (c1 + PAIR16_W1_SHIFT),
                    b1=signed_unit(rng, (16,), 'float32') * 2.0 ** (c1 + PAIR16_W1_SHIFT + 1),
                    w2=signed_unit(rng, (3, 3, 16, 1), 'float32') * 2.0 ** (c2[:, None] + PAIR16_W2_SHIFT),
                    b2=scaled_bias(rng, 1, 'float16'),
                    g=signed_unit(rng, (n, h, w, 1), 'float16') * 2.0 ** -e)


class Interval(namedtuple('Interval', 'lo nom hi')):
    """what a stage of the kernel may hold: its endpoints and the nominal value (lo <= nom <= hi)"""
    @property
    def width(self):
        return self.hi - self.lo

    @property
    def mag(self):
        return np.maximum(np.abs(self.lo), np.abs(self.hi))


class Pair16Steps:
    """conv_pair_bwd in binary16 on the operands of `base`, restated at the rounding points of `kernel` ('strip' or
    'wave'): the intervals, the reference (nominal values), the tolerances and a float32 restatement, for dw1, db1, dw2,
    db2 (unscaled by 2^-k) and dx (as stored: times 2^k).  sig: act2 is a Sigmoid, the kernel reads `yout`."""

    def __init__(self, base, sig, kernel):
        assert kernel in ('strip', 'wave') and base.half
        self.base, self.sig, self.kernel, self.pad1 = base, sig, kernel, base.pad1
        self.name = f'{base.name}-{kernel}' + ('-sigmoid' if sig else '')
        self.pv = float(r16(base.pad1))

    @functools.cached_property
    def yout(self):
        """the stored output: under a Sigmoid with the edge values of sigmoid_outputs (0, 1 and their neighbours); else
        never read"""
        y = sigmoid_outputs(np.random.default_rng(self.base.seed + 7), self.base.q['x'].shape, 'float16')
        y.setflags(write=False)
        return y

    @functools.cached_property
    def gscale(self):
        """log2 of the factor dy is stored with: the largest under which dy, d_a1 and dx stay finite (act2 none decides: a
        Sigmoid only shrinks g)"""
        q = self.base.q
        g = np.abs(q['g'])
        sd = dgrad3(g, np.abs(r16(q['w2']))) * np.where(self._z.hi >= 0, 1.0, max(A16, A32))
        sdx = dgrad3(sd, np.abs(r16(q['w1'])))
        return int(np.floor(np.log2(F16_MAX / max(g.max(), sd.max(), sdx.max()))))

    @functools.cached_property
    def g_dev(self):
        return self.base.q['g'] * 2.0 ** self.gscale

    @functools.cached_property
    def _z(self):
        q = self.base.q
        w1r = r16(q['w1'])
        z = O.conv2d_fwd(q['x'], w1r, q['b1'], 1, 1, self.pv, True)
        e = gamma(9 + SLACK) * O.conv2d_fwd(np.abs(q['x']), np.abs(w1r), np.abs(q['b1']), 1, 1, abs(self.pv), True)
        return Interval(z - e, z, z + e)

    @functools.cached_property
    def iv(self):
        """{stage: Interval} for g, s, a1, d (= d_a1), and `neg`: the positions that take alpha at (lo, nom, hi) of z"""
        q, z = self.base.q, self._z
        w2r = r16(q['w2'])
        if self.sig:
            ge = self.g_dev * (self.yout * (1.0 - self.yout))
            eg = 3 * U32 * np.abs(ge)
            g = Interval(r16(ge - eg), r16(ge), r16(ge + eg))
        else:
            g = Interval(self.g_dev, self.g_dev, self.g_dev)
        es = gamma(9 + SLACK) * dgrad3(g.mag, np.abs(w2r))
        mid, rad = dgrad3(0.5 * (g.lo + g.hi), w2r), dgrad3(0.5 * g.width, np.abs(w2r)) + es
        s = Interval(mid - rad, dgrad3(g.nom, w2r), mid + rad)
        (a_lo, n_lo), (a_nom, n_nom), (a_hi, n_hi) = (pair16_leaky(self.kernel, v, np.float64) for v in z)
        m = lambda v, neg: pair16_masked(self.kernel, v, neg, np.float64)
        d = Interval(np.minimum(m(s.lo, n_lo), m(s.lo, n_hi)), m(s.nom, n_nom), np.maximum(m(s.hi, n_lo), m(s.hi, n_hi)))
        out = dict(z=z, g=g, s=s, a1=Interval(a_lo, a_nom, a_hi), d=d, neg=Interval(n_lo, n_nom, n_hi))
        for t in (g, s, out['a1'], d):
            assert np.all(t.lo <= t.nom) and np.all(t.nom <= t.hi)
        return out

    def _outputs(self, x, a1, g, d, w1r, unscale, dt):
        dw2, db2 = wgrad(a1, g, (3, 3), 1, 1, 0.0, True)
        dw1, db1 = wgrad(x, d, (3, 3), 1, 1, self.pv, True)
        out = dict(dw1=dw1, db1=db1, dw2=dw2, db2=db2)
        out = {k: v * dt(unscale) for k, v in out.items()}
        out['dx'] = dgrad3(d, w1r)
        return out

    @functools.cached_property
    def ref(self):
        """the restatement at the nominal values, float64"""
        q, t = self.base.q, self.iv
        out = self._outputs(q['x'], t['a1'].nom, t['g'].nom, t['d'].nom, r16(q['w1']), 2.0 ** -self.gscale, np.float64)
        for a in out.values():
            a.setflags(write=False)
        return out

    @functools.cached_property
    def parts(self):
        """{output: (arithmetic part, widening)}: gamma(..) of the magnitude sums, and the width(..) terms"""
        q, t = self.base.q, self.iv
        ax, w1a = np.abs(q['x']), np.abs(r16(q['w1']))
        n = ax.shape[0] * ax.shape[1] * ax.shape[2]
        gam, un = gamma(n + SLACK), 2.0 ** -self.gscale
        a1, g, d = t['a1'], t['g'], t['d']
        s2 = wgrad(a1.mag, g.mag, (3, 3), 1, 1)
        w2a, w2g = wgrad(a1.width, g.mag, (3, 3), 1, 1), wgrad(a1.mag, g.width, (3, 3), 1, 1)
        s1 = wgrad(ax, d.mag, (3, 3), 1, 1, abs(self.pv))
        w1 = wgrad(ax, d.width, (3, 3), 1, 1, abs(self.pv))
        return dict(dw1=(gam * s1[0] * un, w1[0] * un), db1=(gam * s1[1] * un, w1[1] * un),
                    dw2=(gam * s2[0] * un, (w2a[0] + w2g[0]) * un),
                    db2=(gam * g.mag.sum(axis=(0, 1, 2)) * un, g.width.sum(axis=(0, 1, 2)) * un),
                    dx=(gamma(144 + SLACK) * dgrad3(d.mag, w1a), dgrad3(d.width, w1a)))

    def tolerances(self, store=True):
        out = {k: a + w for k, (a, w) in self.parts.items()}
        if store:
            out['dx'] = out['dx'] + U16 * np.abs(self.ref['dx']) + FLOOR16
        return out

    @property
    def terms(self):
        x = self.base.q['x'].shape
        return x[0] * x[1] * x[2]

    def halo_column(self):
        """a column that two strips compute: the first computed column of the wave kernel's second strip (owned by the
        first); the cooperative kernel has no halo: the first column of its second wave"""
        w = self.base.shape[2]
        return 62 if self.kernel == 'wave' else 64 if w > 64 else w // 2

    def overlap_row(self):
        """a row that two bands compute (the first row of the second band: the first band computes its d_a1 for dx), or
        None where the page has one row.  Three rows: bands of two rows (pair_band 2); else bands of four"""
        h = self.base.shape[1]
        return None if h == 1 else 2 if h < 5 else 4

    def restated(self, mutant=None, store=True, dt=np.float32):
        """the float32 NumPy restatement (dt: in another arithmetic) -> {output: float64 array}; mutant: 'strip rule' (the other kernel's slope and
        product rule), 'alpha32' (the wave kernel's d_a1 with the unrounded alpha), 'halo' / 'row' (halo_column /
        overlap_row summed twice into all four weight gradients)"""
        f = dt
        q = {k: np.asarray(v).astype(f) for k, v in self.base.q.items()}
        w1r, w2r = h16(q['w1'], f), h16(q['w2'], f)
        z = O.conv2d_fwd(q['x'], w1r, q['b1'], 1, 1, f(self.pv), True)
        g = self.g_dev.astype(f)
        if self.sig:
            y = self.yout.astype(f)
            g = h16(g * (y * (f(1) - y)), f)
        s = dgrad3(g, w2r)
        kernel = 'strip' if mutant == 'strip rule' else self.kernel
        a1, neg = pair16_leaky(kernel, z, f)
        d = pair16_masked(kernel, s, neg, f, A32 if mutant == 'alpha32' else None)
        un = f(2.0 ** -self.gscale)
        out = self._outputs(q['x'], a1, g, d, w1r, un, f)
        if mutant in ('halo', 'row'):
            keep = np.zeros(z.shape[:3] + (1,), f)
            if mutant == 'halo':
                keep[:, :, self.halo_column()] = 1
            else:
                keep[:, self.overlap_row()] = 1
            twice = self._outputs(q['x'], a1 * keep, g, d * keep, w1r, un, f)
            twice['db2'] = (g * keep).sum(axis=(0, 1, 2)) * un
            for k in ('dw1', 'db1', 'dw2', 'db2'):
                out[k] = out[k] + twice[k]
        assert all(a.dtype == f for a in out.values()), {k: a.dtype for k, a in out.items()}
        out = {k: a.astype(np.float64) for k, a in out.items()}
        if store:
            out['dx'] = r16(out['dx'])
        return out

    def room(self, got, name, store=False):
        """(err / tol, (err - widening) / (tol - widening)), largest element each, of `got` for output `name`.  The float32
        restatement is itself a correct kernel and may take the OTHER endpoint of a contested rounding: its error is then
        that element's widening, which is the whole tolerance where little else enters (a dx pixel: 144 terms, gamma(152)).
        The second figure takes out what the contested roundings explain and asks how much of the REST the arithmetic
        uses; store: with the binary16 store terms of dx"""
        tol = self.tolerances(store)[name]
        err, widen = np.abs(got - self.ref[name]), self.parts[name][1]
        live = tol > 0
        assert np.all(err[~live] == 0)
        beyond = np.maximum(err - widen, 0.0)[live] / (tol - widen)[live]
        return float((err[live] / tol[live]).max()), float(beyond.max())

    def widened_share(self, name):
        """share of the elements of `name` whose widening exceeds the arithmetic part (dx: with its store terms, which
        every pixel is allowed whatever it sums)"""
        a, w = self.parts[name]
        if name == 'dx':
            a = a + U16 * np.abs(self.ref['dx']) + FLOOR16
        return float(np.mean(w > a))

    def shares(self):
        """the contested shares: a1, d_a1 (endpoints differ) and the slopes (the endpoints of z take different ones)"""
        t = self.iv
        return dict(a1=float(np.mean(t['a1'].lo != t['a1'].hi)), d_a1=float(np.mean(t['d'].lo != t['d'].hi)),
                    slopes=float(np.mean(t['neg'].lo != t['neg'].hi)), g=float(np.mean(t['g'].lo != t['g'].hi)))

    def check_ranges(self):
        """x, 2^k dy, r16(w1), r16(w2) representable and normal, k > 0; a1, d_a1 and dx finite over their intervals and
        (act2 none) their magnitude sums normal"""
        q, t = self.base.q, self.iv
        assert 0 < self.gscale <= 24, (self.name, self.gscale)
        for k, a in (('x', q['x']), ('g', self.g_dev), ('w1', r16(q['w1'])), ('w2', r16(q['w2']))):
            assert F16_MIN <= np.abs(a).min() and np.abs(a).max() <= F16_MAX, (self.name, k, np.abs(a).min(), np.abs(a).max())
            assert k in ('w1', 'w2') or np.array_equal(r16(a), a), (self.name, k)
        assert np.array_equal(r16(self.yout), self.yout) and r16(self.pad1) == self.pad1
        w1a, w2a = np.abs(r16(q['w1'])), np.abs(r16(q['w2']))
        slope = np.where(t['neg'].nom, min(A16, A32), 1.0)
        s1 = O.conv2d_fwd(np.abs(q['x']), w1a, np.abs(q['b1']), 1, 1, abs(self.pv), True) * slope
        sd = dgrad3(np.abs(self.g_dev), w2a) * slope
        sdx = dgrad3(sd, w1a)
        for k, s, top in (('a1', s1, t['a1'].mag), ('d_a1', sd, t['d'].mag), ('dx', sdx, dgrad3(t['d'].mag, w1a))):
            assert top.max() <= F16_MAX, (self.name, k, top.max())
            assert F16_MIN <= s.min(), (self.name, k, s.min())


class PairWaveDxProblem(Problem):
    """dx of pair_wave_bwd_h_kernel (binary16, pages wider than 512 columns) at its own roundings, every pixel judged
    (Pair16Steps with kernel 'wave').  dx is judged as stored: times 2^k."""
    stored = ('x', 'g', 'yout')

    def __init__(self, steps):
        assert steps.kernel == 'wave'
        super().__init__(steps.name + '-dx', 'float16', steps.base.seed)
        self.steps, self.base, self.sig, self.pad1 = steps, steps.base, steps.sig, steps.pad1

    @functools.cached_property
    def q(self):
        q = dict(self.base.q, yout=self.steps.yout)
        for a in q.values():
            a.setflags(write=False)
        return q

    @property
    def gscale(self):
        return self.steps.gscale

    def device(self, key):
        return self.steps.g_dev if key == 'g' else self.q[key]

    @property
    def ref(self):
        return dict(dx=self.steps.ref['dx'])

    @property
    def parts(self):
        return dict(dx=self.steps.parts['dx'])

    def restated(self, store=True, mutant=None):
        return dict(dx=self.steps.restated(mutant, store)['dx'])

    def tolerances(self, operand16=(), store=True):
        return dict(dx=self.steps.tolerances(store)['dx'])

    def check_ranges(self):
        self.steps.check_ranges()


# Seeds.  The seed decides which channels neighbour each other, where the regions lie and which d_a1 sit next to a rounding
# border: a property of the inputs, found without any kernel.  Every binary16-pair problem takes the first of
# PAIR16_TRIES seeds under which (a) check_ranges holds and on no output more than WIDEN_CAP (5 %) of the elements have a
# widening above their arithmetic part (one contested slope in a channel of large w2 does that to a whole channel of
# dw1 / db1), (b) for the wave kernel, its restatement with the STRIP
# kernel's slope-and-product rule and with the unrounded alpha in d_a1 each exceed the tolerance on some output -- both
# move d_a1 by 2.1e-4 of itself where the slope is alpha (alpha16 / alpha = 1.000214) or by a binary16 step at single
# positions, which gamma(n + 8) S of a weight gradient hides at these n by construction (the sum of n products may err by
# more), so they show on dx, whose pixels sum 144 terms -- and (c) what the caller asks on top (elementwise_wgrad: the
# leak mutant reaches VISIBLE tolerances on dw1 and dw2).  Without such a seed the last one stands and
# test_elementwise_bound_host.py fails.
PAIR16_SEED0, PAIR16_TRIES, PAIR16_SEED_STEP = 21000, 10, 20000
WAVE_RULE_MUTANTS = ('strip rule', 'alpha32')


def pair16_mutant_ratios(st, mutant):
    """{output: largest err / tol} of the restatement of `st` under `mutant`, dx judged as stored.  In float64: the mutant's
    own error alone, and the same figure on every machine (a float32 matrix product sums in the library's order; the seed
    search must not depend on it)"""
    tol, got = st.tolerances(), st.restated(mutant, dt=np.float64)
    out = {}
    for k in tol:                   # (a page of one row: the outer tap rows of dw2 are exactly 0 with a tolerance of 0)
        err = np.abs(got[k] - st.ref[k])
        out[k] = float(np.where(tol[k] > 0, err / np.where(tol[k] > 0, tol[k], 1.0), np.where(err == 0, 0.0, np.inf)).max())
    return out


def pair16_acceptable(st):
    try:
        st.check_ranges()
    except AssertionError:
        return False
    if any(st.widened_share(k) > WIDEN_CAP for k in st.parts):
        return False
    return st.kernel != 'wave' or all(max(pair16_mutant_ratios(st, m).values()) > 1.0 for m in WAVE_RULE_MUTANTS)


@functools.lru_cache(maxsize=None)
def pair16_steps(shape, pad1, sig, kernel, extra=None):
    tag = f'pair16-{shape[0]}x{shape[1]}x{shape[2]}-pad{pad1:g}'
    seed = PAIR16_SEED0 + 100 * shape[2] + 10 * shape[1] + shape[0] + (5 if pad1 else 0) + (50000 if sig else 0)
    for j in range(PAIR16_TRIES):
        st = Pair16Steps(PairSpreadProblem(tag, seed + j * PAIR16_SEED_STEP, shape, pad1), sig, kernel)
        if pair16_acceptable(st) and (extra is None or extra(st)):
            break
    return st


# dx of the wave kernel: ten strips with a ragged last one, several images and bands; whole strips (front<2>).  The
# problems are built when a test asks for them (the seed search costs seconds): the table holds their keys.
PAIR_WAVE_DX_KEYS = tuple((shape, pad1, sig) for shape, pad1 in (((2, 11, 600), 0.25), ((1, 3, 560), 0.0)) for sig in (False, True))
PAIR_WAVE_DX_IDS = [f'16-pair16-{s[0]}x{s[1]}x{s[2]}-pad{pad1:g}-wave' + ('-sigmoid' if sig else '') + '-dx'
                    for s, pad1, sig in PAIR_WAVE_DX_KEYS]


@functools.lru_cache(maxsize=None)
def pair_wave_dx_case(index):
    shape, pad1, sig = PAIR_WAVE_DX_KEYS[index]
    p = PairWaveDxProblem(pair16_steps(shape, pad1, sig, 'wave'))
    assert '16-' + p.name == PAIR_WAVE_DX_IDS[index]
    return Case('16-' + p.name, p, {}, ('dx',), {}, ())


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
    seed = SEEDS.get(kind, 0) + (0 if dtype == 'float32' else 5000)
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
    if kind == 'pair_faint':                 # key: (index into PAIR_SHAPES, pad1)
        i, pad1 = key
        assert dtype == 'float16'
        return PairFaintProblem(f'pair{PAIR_SHAPES[i][2]}-pad{pad1:g}', dtype, PAIR_FAINT_SEEDS[key], PAIR_SHAPES[i], None, pad1)
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


@functools.lru_cache(maxsize=None)
def sigmoid_problem(base):
    return SigmoidProblem(base)


def _sigmoid_cases():
    """y_sigmoid for every conv, upconv and pair case of CASES (same options, same kernels), and for dense_fwd"""
    out = []
    for c in CASES:
        if not isinstance(c.problem, (ConvProblem, UpProblem, PairProblem, DenseProblem)):
            continue
        kernels = {'y_sigmoid': c.kernels['y']} if 'y' in c.kernels else {}
        out.append(Case(c.id + '-sigmoid', sigmoid_problem(c.problem), c.opts, ('y_sigmoid',), kernels,
                        ('y_sigmoid',) if 'y' in c.operand16 else ()))
    return tuple(out)


SIGMOID_CASES = _sigmoid_cases()
SIGMOID_IDS = [c.id for c in SIGMOID_CASES]


def _from_output_cases():
    """act_bwd_from_output on one page tensor; seg_loss(out_act = Sigmoid), Dice and Jaccard, at c = 1, 2, 4 on both
    shapes (seg_grad_vec_kernel where the image is a multiple of 16 bytes, the generic kernel elsewhere) and c = 3"""
    out, seed = [], 9700
    for dtype in ('float32', 'float16'):
        seed += 100
        probs = [FromOutputProblem('act', dtype, seed, SHAPE, 1)]
        for kind in ('dice', 'jaccard'):
            probs += [FromOutputProblem(kind, dtype, seed + 10 * c + i, shape, c)
                      for c in (1, 2, 4) for i, shape in enumerate(SEG_SHAPES)]
            probs.append(FromOutputProblem(kind, dtype, seed + 30, SEG_SHAPES[1], 3))
        out += [Case(f'{dtype[5:]}-{p.name}', p, {}, ('dx',), {}, ()) for p in probs]
    return tuple(out)


# (shape, pad1) -> seed, chosen by trying ten each (from 14400 + 10 shape + 400 pad1): inputs with a contested slope whose
# widened tolerances keep under the cap of test_elementwise_bound_host.py and under which that file's four wrong
# kernels are all told from a right one (a single flipped slope or a coarser d_a1 is near the limit of what 2^-11
# roundings let any bound see: of the ten seeds some show one of them at 0.5 .. 1 of the bound)
PAIR_FAINT_SEEDS = {(0, 0.0): 14403, (0, 0.25): 14503, (1, 0.0): 14417, (2, 0.25): 14529}


@functools.lru_cache(maxsize=None)
def pair_dx_problem(base, sig):
    return PairDxProblem(base, sig)


def _pair_dx_cases():
    """float32: the module's pair problem (pad1 0.25), act2 none and Sigmoid; binary16: the module's (pad1 0) and the same
    shape with pad1 0.25, 128 columns with pad1 0 (the kernel's MODE 0), each with act2 none and Sigmoid, and 71 columns"""
    faint = lambda i, pad1: problem('pair_faint', 'float16', (i, pad1))
    bases = [(problem('pair', 'float32', 0), (False, True)), (faint(0, 0.0), (False, True)), (faint(0, 0.25), (False, True)),
             (faint(1, 0.0), (False, True)), (faint(2, 0.25), (False,))]
    out = []
    for base, sigs in bases:
        for sig in sigs:
            p = pair_dx_problem(base, sig)
            out.append(Case(f'{p.dtype[5:]}-{p.name}', p, {}, ('dx',), {}, ('dx',) if p.half else ()))
    return tuple(out)


PAIR_DX_CASES = _pair_dx_cases()
PAIR_DX_IDS = [c.id for c in PAIR_DX_CASES]
FROM_OUTPUT_CASES = _from_output_cases()
FROM_OUTPUT_IDS = [c.id for c in FROM_OUTPUT_CASES]


# ---- mutations -------------------------------------------------------------------------------------------------------------
def pair_dx_mutants(p):
    """{name: mutate(stage, value)} for PairDxProblem.restated: four wrong pair backward kernels"""
    t = p.parts
    w = p.q['x'].shape[2]
    col = 64 if w > 64 else w // 2                       # first column of the second wave's strip
    # a (position, channel) whose slope is decided and agrees with the oracle's; of those, the one whose flip moves its own
    # dx pixel by the MEDIAN multiple of that pixel's tolerance: half of all single flips are easier to see
    tol = p.tolerances()['dx']
    effect = (1.0 - ALPHA) * np.abs(t['ga1']) * np.abs(p.q['w1'][1, 1, 0]) / tol
    candidates = np.flatnonzero(~t['flip'].ravel())
    order = candidates[np.argsort(effect.ravel()[candidates])]
    at = np.unravel_index(order[len(order) // 2], effect.shape)
    state = {}

    def drop_tap(stage, v):
        if stage == 'd_a1':
            state['d'] = v
        if stage == 'dx':                                # tap (ty, tx) = (1, 2) reads d_a1 of column col - 1
            w1 = p.q['w1'].astype(v.dtype) if not p.half else p.q['w1'].astype(np.float16).astype(v.dtype)
            v = v.copy()
            v[:, :, col, 0] -= (state['d'][:, :, col - 1, :] * w1[1, 2, 0]).sum(axis=-1)
        return v

    def flip_slope(stage, v):
        if stage == 'slope':
            v = v.copy()
            v[at] = v.dtype.type(1.0 + ALPHA) - v[at]
        return v

    def round_twice(stage, v):
        if stage != 'd_a1':
            return v
        if p.half:                                       # binary16 with the low 3 bits of the significand cut off
            bits = v.astype(np.float16).view(np.uint16) & np.uint16(0xFFF8)
            return bits.view(np.float16).astype(v.dtype)
        bits = v.astype(np.float32).view(np.uint32) & np.uint32(0xFFFF0000)      # float32: bfloat16 by truncation
        return bits.view(np.float32).astype(v.dtype)

    def row_off(stage, v):
        if stage == 'slope':                             # the mask of row r + 1 (the last row keeps its own)
            v = np.concatenate([v[:, 1:], v[:, -1:]], axis=1)
        return v

    return {'one tap of w1 dropped at a strip-border column': drop_tap, 'a slope flipped at a decided z1': flip_slope,
            'd_a1 rounded twice': round_twice, 'the mask read one row off': row_off}


def sigmoid_by_tanh16(v, dt=np.float32):
    """0.5 (1 + tanh(v / 2)) in float32 with the argument of tanh rounded to binary16"""
    with np.errstate(over='ignore'):
        t = (v * np.float32(0.5)).astype(np.float16).astype(np.float32)
    return (np.float32(0.5) * (np.float32(1) + np.tanh(t))).astype(np.float32)


def sigmoid_clamped(v, dt=np.float32):
    """the "stable Sigmoid" shortcut: expf(-v) with v clamped to [-16, 16]"""
    return sigmoid(np.clip(v, np.float32(-16), np.float32(16)), np.float32)


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
