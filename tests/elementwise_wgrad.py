"""The weight gradients (dw, db) of the conv, upsample+conv, conv-pair, dense and windows kernels ELEMENT BY ELEMENT:
the bound, the problems and the case table that test_elementwise_bound_host.py (no GPU) and test_gpu_elementwise.py
share.  elementwise_bound.py does the same for y and dx; this module builds on it.

Why.  Every other test judges a weight gradient with rel_linf (max |a - b| / max |b|, 2e-5) on operands of one magnitude.
The weight-gradient kernels are the most layered code of the hot path: per-thread float32 sums, block partials
[block][column], a float64 finish that maps partial COLUMNS to dw / db addresses by one of four layout rules
(finish_group.hip: FIN_COLS, FIN_TAPROWS, FIN_FAST, FIN_PAIR), run as the producer's own kernel or as one entry of a
deferred group with a `first_block` offset; depth slabs in the MFMA GEMM; an unscale by 2^-k in binary16.  A column that
lands one channel over, a neighbouring tap's partial that leaks in, a db that picks up a dw column: none of it moves
rel_linf when the receiving element is large, and with operands of one magnitude every element is large.

The bound.  Per element of dw and db

    tol = gamma(n + 8) S  +  u32 |init + ref|        (the last term only when the call accumulates onto `init`)

  gamma(n)   n u / (1 - n u), u = u32 = 2^-24: a float32 sum of n products in ANY order misses the exact sum by at most
             gamma(n) sum |x_i g_i| (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 3.1).  Block
             partials, a float64 finish and depth slabs are orders of summation: nothing is added for them;
  n          the terms of one element: N OH OW for a conv, the high-resolution pixels for the upconv, the rows for dense
             and windows;
  + 8        elementwise_bound.SLACK: roundings on a term already counted in S (here: the accumulation, the padding value,
             a LeakyReLU scaling of the pair);
  S          the oracle's own weight gradient on the absolute values of its operands (|padding value| included);
  u32 |..|   the one rounding of the sum onto `init`.
Nothing is measured and nothing carries a safety factor.  binary16: x and dy are binary16 already, dw / db are float32
and a product of two binary16 numbers is exact in float32, so no operand term and no store term apply; the unscale by
2^-k is exact.  The conv pair composes the bound through both layers (PairWgradProblem).

Shapes.  gamma(n) grows with the pixel count: at the 3 x 37 x 141 page of elementwise_bound.py (n = 15 651) a leak of
2^-17 of the neighbouring channel is 0.2 .. 8 tolerances, at n ~ 1 900 it is tens to hundreds.  So every case has n <=
2048 (MAX_TERMS), and every configuration runs at two pages: (3, 20, 32) -- several images, w % 4 == 0 (the aligned
float4 row path of the one-input-channel table kernels), whole bands of four output rows at stride 1 and a short last
band at stride 2 (10 rows) -- and (1, 13, 141) -- three 64-column tiles with a ragged last one, the scalar row path, a
short last band at either stride (13 and 7 rows).  Low-resolution upconv inputs: (3, 10, 16), (1, 6, 71).
These are the smallest pages at which the tile, band and column logic still runs; dense and windows have 67 rows, and
one dense case has 1 500 (47 depth tiles: 16 slabs of 3 with a last one of 2 under the default options).

Inputs.  x and dy from elementwise_bound.scaled_input: the elements of dw differ by many powers of two over (cin, cout).
binary16 spends its exponent budget on the channels (LIMITS16: 2^(+-6) per channel, 2^(+-2) per strip; only the stored x
and 2^k dy must be normal, no S is stored) and dy carries the largest gradient scale 2^k that keeps it finite (k > 0 is
asserted).  Dense and windows operands carry per-row AND per-column exponents (columns: 6 for x, 10 for dy, as
dense_weights).  Accumulating calls start from init = float32(ref r), |r| in [0.25, 1] with a random sign per element:
it neither swamps nor vanishes against any element.  (A switched-off bias has ref = 0: its init is r itself, which an
accumulating call must leave as it is and an overwriting call must replace by 0.)  Which channels neighbour each other,
and by how much they differ, is the seed's doing: every problem takes the first of ten seeds under which the leak mutant
reaches 2 tolerances on every output that has one (`visible`; the pair: PAIR_SEED) -- a property of the inputs, found
without any kernel.

The binary16 pair (PairWgrad16Problem, PAIR16_PAGES).  conv_pair_strip_h.hip rounds w1, w2, a1, g and d_a1 to binary16;
composed against an oracle that rounds nowhere, those 2^-11 operand terms give up to 170 |ref| for dw1 and more than
|ref| for dw2 (the sums cancel).  So the reference is the KERNEL'S OWN sequence of roundings, restated in float64 on the
stored binary16 x, dy, yout and the float32 parameters, separately for pair_strip_bwd_h_kernel ('strip', width <= 512:
the slope from the float32 z, float32 products, one rounding) and pair_wave_bwd_h_kernel ('wave': z and s rounded first,
the slope from the sign bit of the rounded z, binary16 products with alpha16 = 0.010002), and every binary16 rounding of
a value the kernel computes in float32 (z1, s = dgrad(g, r16(w2)), g under a Sigmoid) is an INTERVAL [r16(v' - e),
r16(v' + e)] with e that value's own gamma bound: rounding, LeakyReLU and a product with a non-negative constant are
monotone, so the endpoints bound every outcome; where they coincide (97 % of a1 and d_a1) the kernel's value is known bit
for bit.  With width = hi - lo, max = the larger endpoint magnitude, n = N H W:
    dw2   wgrad(width(a1), |g|max) + wgrad(|a1|max, width(g)) + gamma(n + 8) wgrad(|a1|max, |g|max)
    dw1   wgrad(|x|, width(d_a1)) + gamma(n + 8) wgrad(|x|, |d_a1|max), |r16(pad1)| in the border; db1: ones for x
    db2   sum width(g) + gamma(n + 8) sum |g|max                      (+ u32 |init + ref| for an accumulating call)
Products of two binary16 numbers are exact in float32 and the unscale by 2^-k is exact: nothing else enters, nothing is
tuned.  elementwise_bound.py ("The binary16 pair at its own roundings") derives each term, cites the kernel lines, states
the inputs (w1 with b1, and w2, spread over 2^(+-5) per channel with the two extremes as neighbours; x and dy with mild
region exponents of opposite sign; dy times the largest 2^k that keeps dy, d_a1 and dx finite) and how seeds are chosen.
Host figures (test_elementwise_bound_host.py), cooperative / wave kernel: contested a1 1.4 .. 3.3 % / 0.9 .. 3.1 %, d_a1
2.0 .. 3.4 % / 1.7 .. 3.1 %, g under a Sigmoid <= 0.15 %, no contested slope; widening / arithmetic part at most 0.38 (dw1),
0.27 (db1), 0.52 (dw2), 0.016 (db2) on any element (cap: above 1 on at most 5 % of the elements); median tol / |ref| 1.0e-3 ..
7.6e-3 (db2 up to 1.9e-2); room (float32 restatement / tol) <= 0.057 / 0.022; k = 7 .. 12.  Mutants: the 2^-17 leak 2.9 ..
208 / 2.2 .. 71 tolerances on dw1, 3.4 .. 148 / 2.1 .. 401 on dw2 (db1 0.09 .. 26, printed, not asserted) with rel_linf 7.6e-6,
inside the 2e-4 of test_gpu_pair_forms.py; a halo column summed twice 80 .. 477 / 29 .. 217; the overlap row of two bands
summed twice 553 .. 987 / 841 .. 2 920; the wave restatement with the strip kernel's slope-and-product rule, or with alpha
unrounded in d_a1, moves no weight gradient by more than 0.39 tolerances (2.1e-4 of the alpha-slope terms: below gamma(n
+ 8) S by construction) and is rejected on dx, at 1.3 .. 10 and 1.4 .. 11 tolerances.
On the MI355X the largest err / tol over all launch forms was, cooperative / wave kernel: dw1 0.007 / 0.021, db1 0.003 /
0.015, dw2 0.048 / 0.026, db2 < 0.0005 both, and 0.958 / 0.955 for the dx of the same launches (the binary16 store).

Not covered.
  * The leak mutant for single-channel cases (1 -> 1 convs and upconvs): there is no neighbouring channel, and the
    elementwise bound adds a check of precision only.

Host figures, as test_elementwise_bound_host.py prints them (it asserts room <= 0.5, leak > 1, rel_linf < 2e-5):
  room   the float32 NumPy restatement over the tolerance, largest element: table configurations 0.0087 (float32 and
         binary16), MFMA conv 0.0034, generic conv 0.0086, upconvs 0.0043, pair 0.0086 (dw1, through kernel_steps), dense
         0.119 and windows 0.080 (n = 67: gamma(75) is small), dense with 1 500 rows 0.027;
  leak   2^-17 of the neighbouring channel over the tolerance, largest element, smallest .. largest case: table float32
         dw 3.6 .. 782, db 7.1 .. 125; table binary16 dw 2.1 .. 342, db 3.0 .. 76; MFMA conv dw 146 .. 175, db 18 .. 27;
         generic conv dw 211 .. 820, db 9.1 .. 13; upconv 4 -> 4 dw 5.7 .. 313, db 4.0 .. 56; dense 2.1e3 .. 1.9e6; windows
         1.6e6; pair dw1 6.0 .. 107, dw2 10.6 .. 21.5, db1 0.07 .. 0.14 (not asserted, see PAIR_SEED).  Its rel_linf is
         7.63e-6 in every case: the suite's 2e-5 accepts it;
  pair   no contested slope at either page (the widening term is 0 everywhere); largest tol / |ref| 0.18 (dw1), 0.28
         (dw2), 0.14 (db1), 0.0064 (db2).
On the MI355X the largest err / tol was 0.124 (dense, 67 rows), 0.024 (windows) and at most 0.009 for every other case.
"""
import functools
from collections import namedtuple

import numpy as np

import elementwise_bound as B
from oracle import nn_oracle as O
from test_gpu_conv_padding import DGRAD, TABLE, WGRAD, expect_kernel, make_dims
from test_gpu_gemm_configs import GEMM_DEFAULTS

SHAPES = ((3, 20, 32), (1, 13, 141))            # pages; see the module docstring
LOW_SHAPES = ((3, 10, 16), (1, 6, 71))          # low-resolution upconv inputs
MAX_TERMS = 2048                                # the largest n of any case
LEAK = 2.0 ** -17                               # the share of the neighbouring channel the leak mutant adds
ALLOW_W = 2e-5                                  # the suite's rel_linf allowance for dw / db
LIMITS16 = dict(image=1, band=1, strip=2, channel=6)     # binary16: |e| <= 10, x in 2^[-12, 10]
SLAB_ROWS = 1500                                # the dense case whose dw GEMM splits its depth
WIDEN_CAP = B.WIDEN_CAP                             # pair: share of dw1 / db1 elements a contested slope may dominate


wgrad = B.wgrad                                 # (dw, db) of the oracle's conv for input x and output gradient g


def ratio(got, want, tol):
    """|got - want| / tol per element; where tol is 0 (a switched-off bias) only the exact value passes; NaN is infinite"""
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(tol > 0, err / tol, np.where(err == 0, 0.0, np.inf))
    return np.where(np.isnan(r), np.inf, r)


class WgradProblem(B.Problem):
    """One set of operands and its weight gradients.  `run(q, dt)`: the oracle's code in `dt` arithmetic -> {output:
    array}; `sums`: {output: (S, n)}."""
    outputs = ('dw', 'db')
    stored = ('x', 'g')
    bias = True

    @functools.cached_property
    def gscale(self):
        """binary16: log2 of the factor dy is stored with -- the largest that keeps 2^k dy finite"""
        if not self.half:
            return 0
        return int(np.floor(np.log2(B.F16_MAX / np.abs(self.q['g']).max())))

    def device(self, key):
        """operand `key` as the kernel receives it"""
        return self.q[key] * 2.0 ** self.gscale if key == 'g' else self.q[key]

    def check_ranges(self):
        """binary16: x and 2^k dy are representable and inside the normal range, k > 0"""
        if not self.half:
            return
        assert 0 < self.gscale <= 24, (self.name, self.gscale)
        for k in self.stored:
            a = np.abs(self.device(k))
            assert B.F16_MIN <= a.min() and a.max() <= B.F16_MAX, (self.name, k, a.min(), a.max())
            assert np.array_equal(B.r16(self.device(k)), self.device(k)), (self.name, k)

    def restated(self):
        """the float32 NumPy restatement"""
        out = self.run(self.cast(self.q, np.float32), np.float32)
        assert all(a.dtype == np.float32 for a in out.values()), {k: a.dtype for k, a in out.items()}
        return {k: a.astype(np.float64) for k, a in out.items()}

    @functools.cached_property
    def init(self):
        """{output: what an accumulating call starts from}: float32(ref r), |r| in [0.25, 1], random sign"""
        rng = np.random.default_rng(self.seed + 77)
        out = {}
        for k in self.outputs:
            r = B.signed_unit(rng, self.ref[k].shape, 'float32')
            live = self.ref[k] if np.any(self.ref[k] != 0) else np.ones(r.shape)         # (a switched-off bias)
            out[k] = (live * r).astype(np.float32).astype(np.float64)
            out[k].setflags(write=False)
        return out

    def expected(self, name, accumulate):
        return self.ref[name] + self.init[name] if accumulate else self.ref[name]

    def arithmetic(self):
        """{output: gamma(n + 8) S}"""
        return {k: B.gamma(n + B.SLACK) * s for k, (s, n) in self.sums.items()}

    def tolerances(self, accumulate=False):
        out = self.arithmetic()
        if accumulate:
            out = {k: t + B.U32 * np.abs(self.expected(k, True)) for k, t in out.items()}
        return out

    def terms(self):
        """the largest n of the outputs"""
        return max(n for _, n in self.sums.values())

    def leak_axis(self, name):
        """the channel axis of output `name` along which a neighbour exists: the output channels if there are several,
        else the input channels; None: a single channel"""
        shape = self.ref[name].shape
        for axis in range(len(shape) - 1, max(len(shape) - 3, -1), -1):
            if shape[axis] > 1:
                return axis
        return None

    def leaked(self, name):
        """the reference with 2^-17 of the neighbouring channel's value added to every element, or None"""
        axis = self.leak_axis(name)
        return None if axis is None else self.ref[name] + LEAK * np.roll(self.ref[name], 1, axis=axis)


class ConvWgradProblem(WgradProblem):
    def __init__(self, name, dtype, seed, geom, shape, pad_value=0.0, bias=True):
        super().__init__(name, dtype, seed)
        kh, kw, cin, cout, sh, sw, ph, pw = geom
        self.d = make_dims(*shape, kh, kw, cin, cout, sh, sw, ph, pw)
        self.pad_value, self.bias = pad_value, bias

    def draw(self, rng):
        d, limits = self.d, LIMITS16 if self.half else None
        return dict(x=B.scaled_input(rng, (d.n, d.h, d.w, d.cin), self.dtype, limits),
                    g=B.scaled_input(rng, (d.n, d.oh, d.ow, d.cout), self.dtype, limits))

    def run(self, q, dt, pad_value=None):
        d = self.d
        pv = self.pad_value if pad_value is None else pad_value
        dw, db = wgrad(q['x'], q['g'], (d.kh, d.kw), (d.sh, d.sw), (d.ph, d.pw), pv, self.bias)
        return dict(dw=dw, db=db)

    def abs_sums(self):
        n = self.d.n * self.d.oh * self.d.ow
        s = self.run({k: np.abs(v) for k, v in self.q.items()}, np.float64, abs(self.pad_value))
        return {k: (v, n) for k, v in s.items()}


class UpWgradProblem(WgradProblem):
    """Upsample2D(2) + conv 5x5 (padding 2, padding value 0): dw, db from the low-resolution x and the high-resolution dy"""

    def __init__(self, name, dtype, seed, ch, shape):
        super().__init__(name, dtype, seed)
        self.ch, self.shape = ch, shape

    def draw(self, rng):
        (n, hl, wl), ch, limits = self.shape, self.ch, LIMITS16 if self.half else None
        return dict(x=B.scaled_input(rng, (n, hl, wl, ch), self.dtype, limits),
                    g=B.scaled_input(rng, (n, 2 * hl, 2 * wl, ch), self.dtype, limits))

    def run(self, q, dt):
        dw, db = wgrad(O.upsample2d_fwd(q['x'], (2, 2)), q['g'], (5, 5), 1, 2, 0.0, True)
        return dict(dw=dw, db=db)

    def abs_sums(self):
        n, hl, wl = self.shape
        s = self.run({k: np.abs(v) for k, v in self.q.items()}, np.float64)
        return {k: (v, 4 * n * hl * wl) for k, v in s.items()}


def row_col_scaled(rng, rows, cols, col_limit):
    """(rows, cols) magnitudes [0.25, 1] 2^(row exponent in [-16, 16] + column exponent in [-col_limit, col_limit])"""
    e = B.spread(rng, rows, 16)[:, None] + B.spread(rng, cols, col_limit)[None, :]
    return B.signed_unit(rng, (rows, cols), 'float32') * 2.0 ** e


class DenseWgradProblem(WgradProblem):
    """dw = [x, 1]^T . dy, bias row last; rows carry 2^[-16, 16], the columns of x 2^[-6, 6] and of dy 2^[-10, 10]"""
    outputs = ('dw',)
    stored = ()

    def __init__(self, name, dtype, seed, rows):
        super().__init__(name, dtype, seed)
        self.rows = rows

    def draw(self, rng):
        return dict(x=row_col_scaled(rng, self.rows, B.DENSE_K, 6), w=B.dense_weights(rng),
                    g=row_col_scaled(rng, self.rows, B.DENSE_N, 10))

    def run(self, q, dt):
        return dict(dw=O.dense_bwd(q['x'], q['w'], q['g'])[1])

    def abs_sums(self):
        s = self.run({k: np.abs(v) for k, v in self.q.items()}, np.float64)
        return dict(dw=(s['dw'], self.rows))


class WindowsWgradProblem(WgradProblem):
    """dw of fixed-width windows + flatten + dense as one implicit GEMM (ops.windows_dense_bwd)"""
    outputs = ('dw',)
    stored = ()

    def draw(self, rng):
        return dict(x=B.scaled_input(rng, B.WIN_SHAPE, 'float32'), w=B.dense_weights(rng),
                    g=row_col_scaled(rng, B.DENSE_M, B.DENSE_N, 10))

    def run(self, q, dt):
        rows = O.fixed_width_fwd(q['x'], B.WIN_WIDTH).astype(dt).reshape(B.DENSE_M, B.DENSE_K)
        return dict(dw=O.dense_bwd(rows, q['w'], q['g'])[1])

    def abs_sums(self):
        s = self.run({k: np.abs(v) for k, v in self.q.items()}, np.float64)
        return dict(dw=(s['dw'], B.DENSE_M))


class PairWgradProblem(WgradProblem):
    """dw1, db1, dw2, db2 of conv_pair_bwd, float32: conv3x3(1 -> 16, padding value pad1) + LeakyReLU + conv3x3(16 -> 1)
    [+ Sigmoid, whose derivative the kernel takes from the stored output `yout`].  The operands, the kernel's rounding
    points (`kernel_steps`) and the slope rule are elementwise_bound.PairDxProblem's (`dx`).

    The bound through both layers, n = N H W, wgrad = the oracle's conv2d_bwd weight outputs:
      a1     the kernel's a1 lies within Ea1 = gamma(9 + 8) S1 of the oracle's (PairProblem._composed: LeakyReLU is
             1-Lipschitz), S1 = conv(|x|, |w1|, |b1|, |pad1|);
      g      act2 none: dy itself, Eg = 0.  Sigmoid: g = dy (y (1 - y)), three float32 roundings
             (pair_strip_bwd_kernel: `gv *= yn * (1.f - yn)`): Eg = gamma(3) |g|;
      dw2    tol = wgrad(Ea1, |g|) + wgrad(|a1| + Ea1, Eg) + gamma(n + 8) wgrad(|a1| + Ea1, |g| + Eg)
             (inherited from a1, inherited from g, its own sum);  db2 = sum g: sum Eg + gamma(n + 8) sum (|g| + Eg);
      ga1    = dgrad(g, w2) within Ega = (gamma(9 + 8) [+ 3 u]) dgrad(|g|, |w2|) (PairDxProblem.parts); where the slope of z1
             is the oracle's, gz1 = slope ga1 and Egz = slope Ega;
      dw1    tol = wgrad(|x|, Egz) + gamma(n + 8) wgrad(|x|, |gz1| + Egz) + wgrad(|x|, flip (1 - alpha)(|ga1| + Ega))
             with |pad1| in the border; the last term widens the elements that a slope the kernel may take otherwise than
             the oracle (|z1| within gamma(9 + 8) S1 of 0) reaches;  db1 likewise with ones for x.
    No element is left out.  The host test caps the elements of dw1 / db1 whose widening exceeds the arithmetic part at
    5 %, the cap PairDxProblem uses for dx."""
    outputs = ('dw1', 'db1', 'dw2', 'db2')
    stored = ('x', 'g', 'yout')

    def __init__(self, dx):
        super().__init__(dx.name.replace('-dx', '-dw'), dx.dtype, dx.seed)
        assert not dx.half
        self.dx, self.sig, self.pad1 = dx, dx.sig, dx.pad1

    @property
    def q(self):
        return self.dx.q

    def _grads(self, x, a1, g, d_a1, dt):
        dw2, db2 = wgrad(a1, g, (3, 3), 1, 1, 0.0, True)
        dw1, db1 = wgrad(x, d_a1, (3, 3), 1, 1, self.pad1, True)
        return dict(dw1=dw1, db1=db1, dw2=dw2, db2=db2)

    def run(self, q, dt):
        z1 = O.conv2d_fwd(q['x'], q['w1'], q['b1'], 1, 1, dt(self.pad1), True)
        g = self.dx.g_eff(q, dt)
        ga1 = self.dx.dgrad(g, q['w2'])
        return self._grads(q['x'], B.leaky(z1, dt), g, ga1 * B.slope_of(z1, dt), dt)

    def restated(self):
        """through the kernel's rounding points (PairDxProblem.kernel_steps) in float32"""
        q = self.cast(self.q, np.float32)
        z1, _, d_a1, _ = self.dx.kernel_steps(q, np.float32)
        out = self._grads(q['x'], B.leaky(z1, np.float32), self.dx.g_eff(q, np.float32), d_a1, np.float32)
        assert all(a.dtype == np.float32 for a in out.values())
        return {k: a.astype(np.float64) for k, a in out.items()}

    @functools.cached_property
    def parts(self):
        """{output: (arithmetic part, widening)}"""
        q, a, t = self.q, {k: np.abs(v) for k, v in self.q.items()}, self.dx.parts
        n = q['x'].shape[0] * q['x'].shape[1] * q['x'].shape[2]
        gam = B.gamma(n + B.SLACK)
        z1 = t['z1']
        a1 = np.abs(B.leaky(z1, np.float64))
        ea1 = B.gamma(9 + B.SLACK) * O.conv2d_fwd(a['x'], a['w1'], a['b1'], 1, 1, abs(self.pad1), True)
        g = np.abs(self.dx.g_eff(q, np.float64))
        eg = B.gamma(3) * g if self.sig else np.zeros(g.shape)
        dw2 = wgrad(ea1, g, (3, 3), 1, 1)[0] + wgrad(a1 + ea1, eg, (3, 3), 1, 1)[0] + \
            gam * wgrad(a1 + ea1, g + eg, (3, 3), 1, 1)[0]
        db2 = eg.sum(axis=(0, 1, 2)) + gam * (g + eg).sum(axis=(0, 1, 2))
        sl = B.slope_of(z1)
        gz1, egz = np.abs(t['ga1'] * sl), t['ega'] * sl
        pv = abs(self.pad1)
        inherited = wgrad(a['x'], egz, (3, 3), 1, 1, pv)
        own = wgrad(a['x'], gz1 + egz, (3, 3), 1, 1, pv)
        widen = wgrad(a['x'], t['flip'] * (1.0 - B.ALPHA) * (np.abs(t['ga1']) + t['ega']), (3, 3), 1, 1, pv)
        zero = lambda v: np.zeros(v.shape)
        return dict(dw1=(inherited[0] + gam * own[0], widen[0]), db1=(inherited[1] + gam * own[1], widen[1]),
                    dw2=(dw2, zero(dw2)), db2=(db2, zero(db2)))

    def arithmetic(self):
        return {k: a + w for k, (a, w) in self.parts.items()}

    def widened_share(self, name):
        """share of the elements of `name` whose widening exceeds the arithmetic part"""
        a, w = self.parts[name]
        return float(np.mean(w > a))

    def terms(self):
        x = self.q['x'].shape
        return x[0] * x[1] * x[2]

    def check_ranges(self):
        pass


class PairWgrad16Problem(WgradProblem):
    """dw1, db1, dw2, db2 of conv_pair_bwd in binary16, judged at the KERNEL'S OWN roundings: `kernel` = 'strip'
    (pair_strip_bwd_h_kernel, width <= 512) or 'wave' (pair_wave_bwd_h_kernel) selects the restatement, every binary16
    rounding of a float32-computed value is an interval (elementwise_bound.Pair16Steps derives every term; the module
    docstring gives the tolerances).  The reference is the restatement at the nominal values, the gradients unscaled by
    2^-k.  `steps.ref['dx']` / `steps.tolerances()['dx']` judge the dx of the same launch, as stored (times 2^k)."""
    outputs = ('dw1', 'db1', 'dw2', 'db2')
    stored = ('x', 'g', 'yout')

    def __init__(self, steps):
        super().__init__(steps.name + '-dw', 'float16', steps.base.seed)
        self.steps, self.kernel, self.sig, self.pad1 = steps, steps.kernel, steps.sig, steps.pad1

    @functools.cached_property
    def q(self):
        q = dict(self.steps.base.q, yout=self.steps.yout)
        for a in q.values():
            a.setflags(write=False)
        return q

    @property
    def gscale(self):
        return self.steps.gscale

    @functools.cached_property
    def ref(self):
        return {k: self.steps.ref[k] for k in self.outputs}

    def restated(self, mutant=None):
        """the float32 NumPy restatement (Pair16Steps.restated names the mutants)"""
        out = self.steps.restated(mutant)
        return {k: out[k] for k in self.outputs}

    @property
    def parts(self):
        """{output: (arithmetic part, widening = the width(..) terms)}"""
        return {k: self.steps.parts[k] for k in self.outputs}

    def arithmetic(self):
        return {k: a + w for k, (a, w) in self.parts.items()}

    def widened_share(self, name):
        """share of the elements of `name` whose widening exceeds the arithmetic part"""
        return self.steps.widened_share(name)

    def terms(self):
        return self.steps.terms

    def check_ranges(self):
        self.steps.check_ranges()


# ---- the case table --------------------------------------------------------------------------------------------------------
# WCase: a problem, the options it runs under, the (entry, kernel family) `Runtime.last_conv` must report after the call
# (None: no conv entry point) and, for the dense case whose GEMM splits its depth, (M, N, depth) of that GEMM.
WCase = namedtuple('WCase', 'id problem opts kernel gemm', defaults=(None, None))
SEED0, SEED_TRIES, SEED_STEP = 19000, 10, 20000
VISIBLE = 2.0                                   # the leak mutant of a chosen seed reaches this many tolerances
# The pair's inputs are elementwise_bound's (PairProblem) at the small pages.  Of the seeds 9400 .. 9439, 9420 is the one
# whose leak mutant shows best on dw1 and dw2 at both pages, with act2 none and Sigmoid (>= 6.0 and >= 10.6 tolerances;
# 9400: 0.29 and 0.39); no slope is contested under it.  db1 = sum of gz1 inherits sum Egz, up to 0.024 |ref|: under no
# seed tried does a 2^-17 leak reach its tolerance (largest: 0.38), so the mutant is not asserted for db1.
PAIR_SEED = 9420


def leak_ratios(p):
    """{output: the leak mutant's largest err / tol} for the outputs that have one (a neighbouring channel, a live bias)"""
    tol = p.tolerances()
    return {k: float(ratio(p.leaked(k), p.ref[k], tol[k]).max()) for k in p.outputs
            if p.leak_axis(k) is not None and np.any(p.ref[k] != 0)}


def leak_asserted(p):
    """the outputs whose leak mutant must be rejected"""
    return tuple(k for k in leak_ratios(p) if k != 'db1')


def visible(make, seed):
    """the problem make(seed') of the first of SEED_TRIES seeds whose leak mutant reaches VISIBLE tolerances on every
    output that has one -- the seed decides which channels neighbour each other and how much they differ; a property of
    the inputs alone.  Without such a seed the last one stands and test_elementwise_bound_host.py fails."""
    for j in range(SEED_TRIES):
        p = make(seed + j * SEED_STEP)
        if all(r >= VISIBLE for r in leak_ratios(p).values()):
            break
    return p


@functools.lru_cache(maxsize=None)
def wproblem(kind, dtype, key, si):
    """kind 'table' / 'up': key = the table row / the channels; si: index into SHAPES / LOW_SHAPES"""
    if kind == 'pair':                           # key: act2 is a Sigmoid
        return PairWgradProblem(B.pair_dx_problem(_pair_base(si), key))
    return visible(lambda seed: _problem(kind, dtype, key, si, seed),
                   SEED0 + 1000 * si + (0 if dtype == 'float32' else 5000))


def _problem(kind, dtype, key, si, seed):
    tag = lambda s: f'{s[0]}x{s[1]}x{s[2]}'
    if kind == 'table':
        cfg = TABLE[key]
        # even rows of the table: a padding value and no bias; odd rows: a bias and zero padding (as elementwise_bound)
        return ConvWgradProblem(f'table{key}-{tag(SHAPES[si])}', dtype, seed + key, (*cfg[:6], *cfg.net_pad), SHAPES[si],
                                pad_value=0.25 if key % 2 == 0 else 0.0, bias=key % 2 == 1)
    if kind == 'mfma':
        return ConvWgradProblem(f'mfma-{tag(SHAPES[si])}', dtype, seed + 100, B.MFMA_GEOM, SHAPES[si])
    if kind == 'generic':
        return ConvWgradProblem(f'generic-{tag(SHAPES[si])}', dtype, seed + 200, B.GENERIC_GEOM, SHAPES[si], pad_value=0.25)
    if kind == 'up':
        return UpWgradProblem(f'up{key}-{tag(LOW_SHAPES[si])}', dtype, seed + 300 + key, key, LOW_SHAPES[si])
    if kind == 'dense':                          # key: rows
        return DenseWgradProblem(f'dense{key}', dtype, seed + 500 + key, key)
    assert kind == 'windows'
    return WindowsWgradProblem('windows', dtype, seed + 600)


@functools.lru_cache(maxsize=None)
def _pair_base(si):
    """elementwise_bound's float32 pair inputs (pad1 0.25) at the small pages"""
    return B.PairProblem(f'pair-{SHAPES[si][0]}x{SHAPES[si][1]}x{SHAPES[si][2]}', 'float32', PAIR_SEED, shape=SHAPES[si])


def _conv_case(p, opts, tag=''):
    name = expect_kernel(WGRAD, p.dtype, p.d, p.pad_value, opts)
    return WCase(f'{p.dtype[5:]}-{p.name}-dw{tag}', p, opts, (WGRAD, name))


def _cases():
    out = []
    for si in range(len(SHAPES)):
        for i in range(len(TABLE)):
            out.append(_conv_case(wproblem('table', 'float32', i, si), {}))
            out.append(_conv_case(wproblem('table', 'float32', i, si), {'t32': 0, 'tiled': 0}, '-t32_0-tiled0'))
            out.append(_conv_case(wproblem('table', 'float16', i, si), {}))
            out.append(_conv_case(wproblem('table', 'float16', i, si), {'h16': 0}, '-h16_0'))
        out.append(_conv_case(wproblem('mfma', 'float32', 0, si), {'mfma': 2}, '-mfma2'))
        out.append(_conv_case(wproblem('generic', 'float32', 0, si), {}))
        for dtype in ('float32', 'float16'):
            for ch in (4, 1):
                p = wproblem('up', dtype, ch, si)
                out.append(WCase(f'{dtype[5:]}-{p.name}-dw', p, {}))
        for sig in (False, True):
            p = wproblem('pair', 'float32', sig, si)
            out.append(WCase(f'32-{p.name}', p, {}))
    # dense: the generic GEMM (67 rows are too few for the automatic MFMA choice), the MFMA GEMM, and 1 500 rows
    # whose depth the MFMA GEMM splits under the default options (`gemm`: test_gpu_elementwise.py asserts the report)
    p = wproblem('dense', 'float32', B.DENSE_M, 0)
    out.append(WCase('32-dense-dw', p, dict(GEMM_DEFAULTS)))
    out.append(WCase('32-dense-dw-mfma2', p, dict(GEMM_DEFAULTS, mfma=2)))
    out.append(WCase(f'32-dense{SLAB_ROWS}-dw', wproblem('dense', 'float32', SLAB_ROWS, 0), dict(GEMM_DEFAULTS),
                     None, (B.DENSE_K + 1, B.DENSE_N, SLAB_ROWS)))
    d = make_dims(B.WIN_SHAPE[0], B.WIN_SHAPE[1], B.WIN_SHAPE[2], B.WIN_SHAPE[1], B.WIN_WIDTH, B.WIN_SHAPE[3], B.DENSE_N, 1, 1,
                  0, B.WIN_WIDTH // 2)._replace(oh=1, ow=B.WIN_SHAPE[2])
    # (windows_dense_bwd runs dw, then dx: last_conv reports the backward-data call)
    out.append(WCase('32-windows-dw', wproblem('windows', 'float32', 0, 0), {}, (DGRAD, expect_kernel(DGRAD, 'float32', d))))
    return tuple(out)


WCASES = _cases()
WCASE_IDS = [c.id for c in WCASES]


# ---- the binary16 pair: (kernel, page, pad1), each with act2 none and Sigmoid --------------------------------------------
# strip (one cooperative block): several images / a ragged width with and without a padding value (MODE 1) / two whole
# waves at pad1 0 (MODE 0).  wave: 600 columns = ten strips of 64 every 62, three blocks of four with two live in the
# last, a ragged last strip -- at pad1 0 the whole strips take front<2> (keep_l / keep_r alone) and the last one front<1>
# in ONE launch, at pad1 0.25 all take front<1>; 560 columns: the last strip ends on the page, front<2> only; three
# images of one row.
PAIR16_PAGES = (('strip', (3, 20, 32), 0.25), ('strip', (1, 13, 141), 0.0), ('strip', (1, 13, 141), 0.25),
                ('strip', (2, 8, 128), 0.0), ('wave', (1, 3, 600), 0.0), ('wave', (1, 3, 600), 0.25),
                ('wave', (1, 3, 560), 0.0), ('wave', (3, 1, 560), 0.25))


def _leak_visible(steps):
    r = leak_ratios(PairWgrad16Problem(steps))
    return r['dw1'] >= VISIBLE and r['dw2'] >= VISIBLE


@functools.lru_cache(maxsize=None)
def pair16_problem(kernel, shape, pad1, sig):
    return PairWgrad16Problem(B.pair16_steps(shape, pad1, sig, kernel, _leak_visible))


# (the problems are built when a test asks for them -- the seed search costs seconds: the table holds their keys)
PAIR16_KEYS = tuple((kernel, shape, pad1, sig) for kernel, shape, pad1 in PAIR16_PAGES for sig in (False, True))
PAIR16_IDS = [f'16-pair16-{s[0]}x{s[1]}x{s[2]}-pad{pad1:g}-{kernel}' + ('-sigmoid' if sig else '') + '-dw'
              for kernel, s, pad1, sig in PAIR16_KEYS]
