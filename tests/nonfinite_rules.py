"""What a kernel must do with a NaN or an Inf in an operand: the rules, the plants and the step-level cases that
test_nonfinite_host.py (no GPU) and test_gpu_nonfinite.py share.

Why.  Trainer.train (my_model/trainer.py) has one defence against a diverged run: after each epoch it asks every model
nan_weights() -- ops.has_nan over the flat parameter pack -- and on a NaN reloads the last weights with a smaller learning
rate.  Nothing looks at the losses or the gradients, so the defence rests on a property the kernels must have one by one:
a non-finite value anywhere in a step's forward or backward pass arrives in the weights as NaN.  In NumPy that happens by
itself; a kernel can swallow it (fmaxf(NaN, a) is a), carry it into another image (a prefetched tile, a register window) or
turn it into a huge finite number.  With finite data such a leak is a small numeric error; with one NaN it is there or it
is not.

bad(a) = ~isfinite(a).  For a kernel output K and the float64 oracle's output R on the same planted operands:

  R1  nothing swallowed   bad(R) is a subset of bad(K), and isnan(R) of isnan(K).  One exception, binary16 loss gradients
                          (`saturating`): where R is +-Inf, K may be +-65504 with R's sign -- loss.hip saturates a finite
                          overflow on purpose; a NaN has no exception.
  R2  nothing crosses     per-image outputs (y, dx, a loss gradient): in every image other than the planted one K is finite
                          and within the case's tolerance of R.
  R3  agreement           where K and R are both finite they agree under the case's EXISTING tolerance, evaluated on the
                          planted operands (the host test asserts that this tolerance is itself non-finite only where R is).
  R4  spread              the count of bad(K) & ~bad(R) is returned and printed.  A conv-family kernel may spread inside the
                          planted image only (a Toeplitz or MFMA form multiplies a zero band by the NaN: R2 already forbids
                          the rest); an `exact` kernel (elementwise, copy-like, reduction-free) may not spread at all: bad(K)
                          == bad(R); a weight gradient may spread to other channels and taps.

Plants.  Three positions per tensor, one run each: the first element (first pixel of image 0, channel 0), an interior
element of the middle image, the last element (last pixel of the last image, last channel: the ragged last tile in both
directions).  Values NaN and +Inf; -Inf once per family, at the interior position.  A weight is planted at its CENTRE tap:
the oracle multiplies the padding value by every tap, so a NaN in a border tap times a zero padding is NaN in the oracle
and rightly nothing in a kernel that skips the taps outside the image -- the centre tap never lies outside.

No figure is introduced here: every tolerance is the reused case's own.  Where v = +-Inf enters a Sigmoid the oracle's
result is exactly 1 or 0 (finite: +Inf into a Sigmoid is legitimately 1) and the derived tolerance E sigma'(|v| - E) reads
Inf - Inf; there the inherited term is taken at E = 0 (an infinite v has no neighbourhood; 1 / (1 + expf(-+Inf)) is exact).
"""
import copy
from collections import namedtuple

import numpy as np

import elementwise_bound as B
import elementwise_wgrad as W
from oracle import nn_oracle as O

F16_MAX = 65504.0
NAN, INF = float('nan'), float('inf')


def bad(a):
    return ~np.isfinite(np.asarray(a, dtype=np.float64))


def describe(value):
    return 'nan' if value != value else ('+inf' if value > 0 else '-inf')


# ---- positions -----------------------------------------------------------------------------------------------------------
def positions(shape):
    """{name: index}: first element, an interior element of the middle image, last element"""
    return dict(first=tuple(0 for _ in shape), interior=tuple(s // 2 for s in shape), last=tuple(s - 1 for s in shape))


def centre(shape):
    return tuple(s // 2 for s in shape)


def put(a, index, value):
    """a float64 copy of `a` with `value` at `index` (read-only, as the problems keep their operands)"""
    out = np.array(a, dtype=np.float64)
    out[index] = value
    out.setflags(write=False)
    return out


# ---- the rules -------------------------------------------------------------------------------------------------------------
Verdict = namedtuple('Verdict', 'failures spread')


def judge(what, K, R, tol, image=None, images=None, exact=False, saturating=False, judged=None):
    """The four rules for one output.
    tol      elementwise absolute tolerance (broadcastable), evaluated on the planted operands
    images   integer array broadcastable to R: the image each element belongs to (None: not a per-image output)
    image    the planted image (None: the plant reaches every image -- a weight, a bias -- and R2 has nothing to judge)
    exact    R4: no spread at all
    judged   boolean mask of the elements whose VALUE is compared (R1 and R4 hold everywhere)"""
    K, R = np.asarray(K, dtype=np.float64), np.asarray(R, dtype=np.float64)
    assert K.shape == R.shape, (what, K.shape, R.shape)
    tol = np.broadcast_to(np.asarray(tol, dtype=np.float64), R.shape)
    bk, br = bad(K), bad(R)
    failures = []
    swallowed = br & ~bk
    if saturating:
        swallowed &= ~(np.isinf(R) & (K == np.sign(R) * F16_MAX))
    if swallowed.any():
        at = tuple(int(i) for i in np.argwhere(swallowed)[0])
        failures.append(f'{what}: R1 {int(swallowed.sum())} non-finite elements of the oracle are finite in the kernel, first at '
                        f'{at}: {K[at]!r} for {R[at]!r}')
    lost_nan = np.isnan(R) & ~np.isnan(K)
    if lost_nan.any() and not swallowed.any():
        at = tuple(int(i) for i in np.argwhere(lost_nan)[0])
        failures.append(f'{what}: R1 {int(lost_nan.sum())} NaN of the oracle are not NaN in the kernel, first at {at}: {K[at]!r}')
    with np.errstate(invalid='ignore'):
        off = ~bk & ~br & ~(np.abs(K - R) <= tol)
    if judged is not None:
        off &= np.broadcast_to(judged, R.shape)
    other = np.zeros(R.shape, bool)
    if images is not None and image is not None:
        other = np.broadcast_to(np.asarray(images) != image, R.shape)
        crossed = other & bk
        if crossed.any():
            at = tuple(int(i) for i in np.argwhere(crossed)[0])
            failures.append(f'{what}: R2 {int(crossed.sum())} non-finite elements outside image {image}, first at {at}')
        if (off & other).any():
            at = tuple(int(i) for i in np.argwhere(off & other)[0])
            failures.append(f'{what}: R2 {int((off & other).sum())} elements outside image {image} miss the tolerance, first at '
                            f'{at}: {K[at]!r} for {R[at]!r} (tol {tol[at]:.3e})')
    if (off & ~other).any():
        at = tuple(int(i) for i in np.argwhere(off & ~other)[0])
        failures.append(f'{what}: R3 {int((off & ~other).sum())} finite elements miss the tolerance, first at {at}: {K[at]!r} for '
                        f'{R[at]!r} (tol {tol[at]:.3e})')
    spread = int((bk & ~br).sum())
    if exact and spread:
        at = tuple(int(i) for i in np.argwhere(bk & ~br)[0])
        failures.append(f'{what}: R4 {spread} elements are non-finite where the oracle is finite, first at {at}: {K[at]!r} for '
                        f'{R[at]!r}')
    return Verdict(failures, spread)


def tolerance_is_sound(tol, R):
    """the tolerance is non-finite only where the oracle is"""
    tol = np.broadcast_to(np.asarray(tol, dtype=np.float64), np.shape(R))
    return not (bad(tol) & ~bad(R)).any()


# ---- mutants (test_nonfinite_host.py) --------------------------------------------------------------------------------------
def clamped(a):
    """what grad_store<_Float16> did: clip to +-65504 with fmaxf / fminf, which turn a NaN into -65504"""
    a = np.asarray(a, dtype=np.float64)
    return np.where(np.isnan(a), -F16_MAX, np.clip(a, -F16_MAX, F16_MAX))


def leaked(a, images, image):
    """one NaN copied into the first element of another image"""
    out = np.array(a, dtype=np.float64)
    target = np.argwhere(np.broadcast_to(np.asarray(images) != image, out.shape) & ~bad(out))
    out[tuple(target[0])] = np.nan
    return out


def one_more(a):
    """one extra NaN at the first finite element"""
    out = np.array(a, dtype=np.float64)
    out[tuple(np.argwhere(~bad(out))[0])] = np.nan
    return out


# ---- planted copies of the elementwise problems ----------------------------------------------------------------------------
def replanted(p, changes):
    """problem `p` (elementwise_bound / elementwise_wgrad) with its operands changed: changes = {operand: (index, value)}.
    Everything derived from the operands (reference, S, tolerances) is evaluated anew; what describes the CLEAN inputs --
    the Sigmoid shift, the gradient scale of a binary16 dy, the value an accumulating call starts from -- is kept."""
    if isinstance(p, B.SigmoidProblem):
        c = copy.copy(p)
        c.__dict__['shift'] = p.shift
        c.__dict__['inner'] = replanted(p.inner, changes)
        c.__dict__.pop('ref', None)
        return c
    if isinstance(p, W.WgradProblem):
        p.gscale, p.init                                 # (cached on the clean problem, copied below)
    c = copy.copy(p)
    for k in ('q', 'ref', 'sums', '_composed', 'parts'):
        c.__dict__.pop(k, None)
    if isinstance(p, W.PairWgradProblem):
        c.dx = replanted(p.dx, changes)
        return c
    q = dict(p.q)
    for key, (index, value) in changes.items():
        q[key] = put(q[key], index, value)
    c.__dict__['q'] = q
    return c


def tolerances(p, operand16=(), accumulate=False):
    """the case's own tolerances on the problem's (planted) operands"""
    with np.errstate(all='ignore'):
        if isinstance(p, W.WgradProblem):
            return p.tolerances(accumulate)
        tol = dict(p.tolerances(operand16))
        if isinstance(p, B.SigmoidProblem):
            v = p.v
            at = np.isinf(v)
            if at.any():                                 # module docstring: the inherited term at E = 0
                tol['y_sigmoid'] = np.where(at, B.sigmoid_tolerance(np.where(at, v, 0.0), 0.0, p.half), tol['y_sigmoid'])
        return tol


def reference(p):
    with np.errstate(all='ignore'):
        return p.ref


def restated(p):
    with np.errstate(all='ignore'):
        return p.restated()


def image_ids(p, name):
    """the image of every element of output `name`, broadcastable to it: axis 0 for page tensors and for the rows of a GEMM;
    the windows problem has ONE image (its 67 rows are the columns of one strip); None for a weight gradient"""
    if isinstance(p, W.WgradProblem):
        return None
    shape = reference(p)[name].shape
    if isinstance(p, B.WindowsProblem):
        return np.zeros((1,) * len(shape), int)
    return np.arange(shape[0]).reshape((shape[0],) + (1,) * (len(shape) - 1))


# Plant: changes = {operand: (index, value)}; outputs: the outputs it is judged on (None: all); image: the planted image of
# those outputs (None: every image)
Plant = namedtuple('Plant', 'id changes outputs image')
FORWARD, BACKWARD = ('y', 'y_leaky', 'y_sigmoid'), ('dx', 'dx_leaky')


def _activation_plants(p, key, outputs, minus, image_of=lambda index: index[0]):
    shape = p.q[key].shape
    out = []
    for where, index in positions(shape).items():
        for value in (NAN, INF) + ((-INF,) if minus and where == 'interior' else ()):
            out.append(Plant(f'{key}[{where}]={describe(value)}', {key: (index, value)}, outputs, image_of(index)))
    return out


def plants(p, minus=False):
    """the plants of one problem of elementwise_bound.CASES / SIGMOID_CASES (module docstring); minus: also -Inf"""
    inner = p.inner if isinstance(p, B.SigmoidProblem) else p
    one_image = (lambda index: 0) if isinstance(inner, B.WindowsProblem) else (lambda index: index[0])
    out = _activation_plants(inner, 'x', FORWARD, minus, one_image)
    if not isinstance(p, B.SigmoidProblem):
        out += _activation_plants(inner, 'g', BACKWARD, minus, one_image)
    for key in inner.weights:
        forward_only = isinstance(p, B.SigmoidProblem)
        for value in (NAN, INF):
            out.append(Plant(f'{key}[centre]={describe(value)}', {key: (centre(inner.q[key].shape), value)},
                             FORWARD if forward_only else None, None))
    biases = [k for k in ('b', 'b1', 'b2') if k in inner.q and getattr(inner, 'bias', True)]
    for key in biases:
        out.append(Plant(f'{key}[centre]=nan', {key: (centre(inner.q[key].shape), NAN)}, FORWARD, None))
    return out


def last_pixel_unused(d):
    """whether no window of the conv geometry `d` reaches the last input row or column (a stride that leaves a rest): a value
    planted there reaches nothing in the oracle, and must reach nothing in a kernel"""
    return (d.oh - 1) * d.sh + d.kh - 1 - d.ph < d.h - 1 or (d.ow - 1) * d.sw + d.kw - 1 - d.pw < d.w - 1


def wgrad_plants(p, minus=False):
    """x and dy of a weight-gradient problem at the three positions; every output is judged"""
    return _activation_plants(p, 'x', None, minus) + _activation_plants(p, 'g', None, minus)


def with_planted_init(p):
    """a copy of weight-gradient problem `p` whose accumulating calls start from a value with one NaN (at the centre of
    every output): the sum onto it must stay NaN there"""
    c = copy.copy(p)
    c.__dict__['init'] = {name: put(a, centre(a.shape), NAN) for name, a in p.init.items()}
    return c


# ---- step level ------------------------------------------------------------------------------------------------------------
# One NaN in (i) one input pixel of image 0, (ii) one weight, (iii) one label.  The nets of a PageTrainer share their layers:
# 'monochrome' is the label of the Monochrome net AND the input of the Paragraph and Line nets.  So a run plants the layers
# of one row below and every net meets each of its three plants in some run, while the nets a run does not reach must stay
# finite (nothing crosses nets):
#   run          layers planted                       becomes NaN                       stays finite
STEP_RUNS = {
    'inputs':    (('image', 'char_lines'),             ('Monochrome', 'Char'),           ('Paragraph', 'Line')),
    'shared':    (('monochrome',),                     ('Monochrome', 'Paragraph', 'Line'), ('Char',)),
    'labels':    (('paragraph', 'line', 'char_labels'), ('Paragraph', 'Line', 'Char'),    ('Monochrome',)),
    'weights':   ((),                                  ('Monochrome', 'Paragraph', 'Line', 'Char'), ()),
}
# A label is planted in every channel (class) of one position: the Line net's two output channels and the Char net's 162
# classes each have their own column of the last layer's weights, which a NaN in ONE channel of the label does not reach in
# the oracle either (dw[..., c] sums over dy[..., c] alone) -- such a case is not used at step level.
LABEL_LAYERS = ('monochrome', 'paragraph', 'line', 'char_labels')


def step_index(layer, shape):
    """where a layer of a page batch is planted: an interior pixel of image 0 (one row of the Char labels), every channel
    of a label, the single channel of an input"""
    if len(shape) == 2:
        return (shape[0] // 4, slice(None))
    return (0, shape[1] // 2, shape[2] // 2, slice(None))


def planted_batch(batch, layers):
    out = dict(batch)
    for layer in layers:
        a = np.array(batch[layer], dtype=np.float64)
        a[step_index(layer, a.shape)] = np.nan
        out[layer] = a
    return out


def first_weight(names):
    """the parameter a 'weights' run plants: the weights of the net's first layer (its first element)"""
    return sorted(n for n in names if n.endswith('/w'))[0]


# ---- elementwise, shape, loss, regulariser and optimizer cases -----------------------------------------------------------
# MapCase: operands(dtype) -> {name: float64 array representable in dtype}; planted = {operand: values}; oracle(q) ->
# {output: float64 array}; outputs = {output: 'bits' (a copy: compared bit for bit) or 'close' (the rel_linf tolerance of
# test_gpu_streaming_ops.TOL, taken of the largest finite |R|)}; exact: R4 allows no spread; images: {output: how many
# leading axes name the image (0: not a per-image output)}.
TOL = {'float32': 1e-5, 'float16': 1e-3}            # test_gpu_streaming_ops.TOL
ALL_VALUES = (NAN, INF, -INF)
ALPHA = B.ALPHA


class MapCase:
    def __init__(self, id, draw, planted, oracle, outputs, exact=True, per_image=True, where=None, saturating=False):
        self.id, self.draw, self.planted, self.oracle, self.outputs = id, draw, planted, oracle, outputs
        self.exact, self.per_image, self.where, self.saturating = exact, per_image, where, saturating

    def operands(self, dtype):
        rng = np.random.default_rng(sum(map(ord, self.id)))
        q = {k: np.asarray(v, dtype=np.float64).astype(B.STORE[dtype]).astype(np.float64) for k, v in self.draw(rng).items()}
        for a in q.values():
            a.setflags(write=False)
        return q

    def plants(self, q):
        out = []
        for key, values in self.planted.items():
            spots = positions(q[key].shape) if self.where is None or key not in self.where else self.where[key](q[key].shape)
            for where, index in spots.items():
                for value in values:
                    out.append(Plant(f'{key}[{where}]={describe(value)}', {key: (index, value)}, None, index[0]))
        return out

    def reference(self, q):
        with np.errstate(all='ignore'):
            return {k: np.asarray(v, dtype=np.float64) for k, v in self.oracle(q).items()}

    def restated(self, q, dtype):
        """the oracle's code on float32 operands, a binary16 output rounded once"""
        with np.errstate(all='ignore'):
            out = self.oracle({k: v.astype(np.float32) for k, v in q.items()})
            return {k: np.asarray(v).astype(B.STORE[dtype]).astype(np.float64) if self.outputs[k] != 'int' else
                    np.asarray(v, dtype=np.float64) for k, v in out.items()}

    def tolerance(self, name, R, dtype):
        if self.outputs[name] != 'close':
            return 0.0
        finite = np.abs(R[np.isfinite(R)])
        return TOL[dtype] * (finite.max() if finite.size else 0.0)

    def images(self, name, R):
        if not self.per_image or R.ndim == 0:
            return None
        return np.arange(R.shape[0]).reshape((R.shape[0],) + (1,) * (R.ndim - 1))

    def changed(self, q, plant):
        out = dict(q)
        for key, (index, value) in plant.changes.items():
            out[key] = put(q[key], index, value)
        return out


def _acts():
    shape = B.SHAPE + (1,)                              # 15 651 elements: odd, a scalar tail behind the 16-byte vectors
    fwd = {'relu': O.relu_fwd, 'leaky': lambda x: O.leaky_relu_fwd(x, ALPHA), 'sigmoid': O.sigmoid_fwd}
    bwd = {'relu': O.relu_bwd, 'leaky': lambda x, g: O.leaky_relu_bwd(x, g, ALPHA), 'sigmoid': O.sigmoid_bwd}
    # the derivative from the OUTPUT as uocr_common.h states it (act_grad_from_output): the slope of a LeakyReLU from the
    # sign of y, y (1 - y) for a Sigmoid -- elementwise_bound.FromOutputProblem's reference
    out = {'leaky': lambda y, g: g * B.slope_of(y), 'sigmoid': lambda y, g: g * (y * (1.0 - y))}
    x = lambda rng: rng.standard_normal(shape) * 3.0
    y01 = lambda rng: rng.uniform(0.01, 0.99, shape)
    cases = []
    for kind in ('leaky', 'relu', 'sigmoid'):
        cases.append(MapCase(f'act_fwd-{kind}', lambda rng: dict(x=x(rng)), dict(x=ALL_VALUES),
                             lambda q, f=fwd[kind]: dict(y=f(q['x'])), dict(y='close')))
        # Sigmoid', x = -Inf: the oracle's e / (e + 1)^2 overflows to NaN for EVERY x < -709, finite ones too -- an
        # artefact of its formula, not a non-finite operand passed on; not planted
        cases.append(MapCase(f'act_bwd-{kind}', lambda rng: dict(x=x(rng), dy=x(rng)),
                             dict(x=(NAN, INF) if kind == 'sigmoid' else ALL_VALUES, dy=ALL_VALUES),
                             lambda q, f=bwd[kind]: dict(dx=f(q['x'], q['dy'])), dict(dx='close')))
    for kind in ('leaky', 'sigmoid'):
        draw = (lambda rng: dict(y=O.leaky_relu_fwd(x(rng), ALPHA), dy=x(rng))) if kind == 'leaky' else \
            (lambda rng: dict(y=y01(rng), dy=x(rng)))
        cases.append(MapCase(f'act_bwd_from_output-{kind}', draw, dict(y=ALL_VALUES, dy=ALL_VALUES),
                             lambda q, f=out[kind]: dict(dx=f(q['y'], q['dy'])), dict(dx='close')))
    return cases


def _window_spots(shape):
    """the four positions of one interior 2 x 2 window, and the last one of the last image"""
    n, h, w, c = shape
    oy, ox = (h // 2) // 2, (w // 2) // 2
    out = {f'window+{dy}{dx}': (n // 2, 2 * oy + dy, 2 * ox + dx, c // 2) for dy in (0, 1) for dx in (0, 1)}
    out['first'] = (0, 0, 0, 0)
    out['last'] = (n - 1, 2 * (h // 2) - 1, 2 * (w // 2) - 1, c - 1)
    return out


def _shapes():
    cases = []
    normal = lambda shape: (lambda rng: rng.standard_normal(shape))
    # upsample 2 x 2: the 16-byte kernels (float32, 1 or 4 channels, a row of whole vectors) and the generic ones
    for shape in ((3, 9, 36, 4), (3, 9, 35, 3)):
        up = (shape[0], 2 * shape[1], 2 * shape[2], shape[3])
        cases.append(MapCase(f'upsample2d-{shape[2]}x{shape[3]}', lambda rng, s=shape, u=up: dict(x=normal(s)(rng), g=normal(u)(rng)),
                             dict(x=ALL_VALUES, g=ALL_VALUES),
                             lambda q: dict(y=O.upsample2d_fwd(q['x'], (2, 2)), dx=O.upsample2d_bwd(q['g'], (2, 2))),
                             dict(y='bits', dx='close')))
    fw, width = (2, 5, 67, 3), 8
    cases.append(MapCase('fixed_width', lambda rng: dict(x=normal(fw)(rng), g=normal((fw[0] * fw[2], fw[1], width, fw[3]))(rng)),
                         dict(x=ALL_VALUES, g=ALL_VALUES),
                         lambda q: dict(y=O.fixed_width_fwd(q['x'], width), dx=O.fixed_width_bwd(q['g'], fw, width)),
                         dict(y='bits', dx='close'), per_image=False))
    a, b = (3, 9, 35, 2), (3, 9, 35, 3)
    cases.append(MapCase('copy_2d', lambda rng: dict(a=normal(a)(rng), b=normal(b)(rng)), dict(a=ALL_VALUES, b=ALL_VALUES),
                         lambda q: dict(cat=O.concat_fwd([q['a'], q['b']]), **dict(zip(('part_a', 'part_b'), O.concat_bwd(
                             O.concat_fwd([q['a'], q['b']]), [a, b])))), dict(cat='bits', part_a='bits', part_b='bits')))
    cases.append(MapCase('convert', lambda rng: dict(x=normal(B.SHAPE)(rng)), dict(x=ALL_VALUES), lambda q: dict(y=q['x']),
                         dict(y='bits')))
    # max-pool 2 x 2: the 16-byte kernels (float32, whole windows, channels a multiple of four) and the generic ones.  A NaN
    # sticks in the maximum as in np.max, and `vals == y` is False for it: the window's mask is all zero, and the backward
    # pass divides by that count -- the oracle's dx is NaN at all four positions.  -Inf is never the maximum: not planted
    for shape in ((3, 8, 36, 4), (3, 9, 35, 3)):
        oshape = (shape[0], shape[1] // 2, shape[2] // 2, shape[3])

        def pool(q, s=shape):
            y, mask = O.maxpool2d_fwd(q['x'], (2, 2), (2, 2), (0, 0))
            return dict(y=y, mask=mask, dx=O.maxpool2d_bwd(q['g'], mask, s, (2, 2), (2, 2), (0, 0)))
        cases.append(MapCase(f'maxpool2d-{shape[2]}x{shape[3]}', lambda rng, s=shape, o=oshape: dict(x=normal(s)(rng), g=normal(o)(rng)),
                             dict(x=(NAN, INF), g=ALL_VALUES), pool, dict(y='bits', mask='int', dx='close'),
                             where=dict(x=_window_spots)))
    return cases


MAP_CASES = _acts() + _shapes()
MAP_IDS = [c.id for c in MAP_CASES]
# (case, operand, value) at which the ORACLE itself stays finite everywhere -- such a plant still checks that the kernel
# stays finite and right; every other plant must make the oracle non-finite somewhere.  A mask (x >= 0) of NaN is 0 and
# of +-Inf is 0 or 1; a Sigmoid maps +-Inf to 1 and 0; the LeakyReLU slope read off y is alpha for a NaN.
ORACLE_ABSORBS = {('act_fwd-sigmoid', 'x', '+inf'), ('act_fwd-sigmoid', 'x', '-inf'), ('act_bwd-sigmoid', 'x', '+inf')}
ORACLE_ABSORBS |= {(f'act_bwd-{k}', 'x', v) for k in ('relu', 'leaky') for v in ('nan', '+inf', '-inf')}
ORACLE_ABSORBS |= {('act_bwd_from_output-leaky', 'y', v) for v in ('nan', '+inf', '-inf')}
# (case, plant id): the first column of the first window of fixed_width and the last column of the last one lie in the zero
# padding, which the backward pass crops
ORACLE_ABSORBS |= {('fixed_width', f'g[{w}]={v}') for w in ('first', 'last') for v in ('nan', '+inf', '-inf')}


def absorbed(case_id, plant):
    (key, (_, value)), = plant.changes.items()
    return (case_id, key, describe(value)) in ORACLE_ABSORBS or (case_id, plant.id) in ORACLE_ABSORBS


# ---- losses --------------------------------------------------------------------------------------------------------------
SegCase = namedtuple('SegCase', 'id problem kind out_act')


def _seg_cases():
    """Dice and Jaccard at c = 1, 2, 4 on both shapes of elementwise_bound.SEG_SHAPES (the vector kernels where an image is a
    multiple of 16 bytes, the generic ones elsewhere) and c = 3, float32 and binary16, with and without out_act='sigmoid':
    the problems of elementwise_bound.FROM_OUTPUT_CASES (stored Sigmoid outputs y, labels 0 / 1)"""
    out = []
    for c in B.FROM_OUTPUT_CASES:
        if c.problem.kind != 'act':
            out += [SegCase(f'{c.id}-{"sigmoid" if act else "plain"}', c.problem, c.problem.kind, act) for act in (None, 'sigmoid')]
    return out


SEG_CASES = _seg_cases()
SEG_IDS = [c.id for c in SEG_CASES]


def seg_reference(case, q):
    """(loss, gradient times the binary16 gradient scale) of the oracle"""
    with np.errstate(all='ignore'):
        loss, grad = (O.dice_loss if case.kind == 'dice' else O.jaccard_loss)(q['y'], q['gt'])
        if case.out_act:
            grad = grad * (q['y'] * (1.0 - q['y']))
        return loss, grad * 2.0 ** case.problem.gscale


def seg_tolerance(case, q, R):
    """with the Sigmoid folded in: elementwise_bound.FromOutputProblem's bound on these operands; without: the rel_linf
    tolerance of test_gpu_streaming_ops (check_seg), of the largest finite |R|"""
    if case.out_act:
        return tolerances(replant_q(case.problem, q))['dx']
    finite = np.abs(R[np.isfinite(R)])
    return TOL[case.problem.dtype] * (finite.max() if finite.size else 0.0)


def replant_q(p, q):
    c = copy.copy(p)
    for k in ('q', 'ref', 'sums'):
        c.__dict__.pop(k, None)
    c.__dict__['q'] = q
    return c


def seg_plants(q, minus=False):
    """pred and, separately, the labels at the three positions; the planted (image, channel) pair"""
    shape = q['y'].shape
    out = []
    for key in ('y', 'gt'):
        for where, index in positions(shape).items():
            for value in (NAN, INF) + ((-INF,) if minus and where == 'interior' else ()):
                out.append(Plant(f'{key}[{where}]={describe(value)}', {key: (index, value)}, None, index[0] * shape[3] + index[3]))
    return out


def seg_pairs(shape):
    """the (image, channel) pair of every element"""
    n, _, _, c = shape
    return (np.arange(n)[:, None] * c + np.arange(c)[None, :]).reshape(n, 1, 1, c)


CE_SHAPES = ((37, 162), (37, 16))                      # 64 and 16 lanes per row of uocr_softmax_ce
# -Inf in a softmax row is exp(-Inf) = 0, a probability of exactly 0 -- which the oracle's loss (no epsilon in the log)
# turns into 0 * log 0 = NaN for ANY row that underflows, finite logits included: an artefact of its formula; not planted
CE_VALUES = dict(softmax=(NAN, INF), sigmoid=ALL_VALUES)


def ce_operands(shape, dtype, soft):
    rng = np.random.default_rng(shape[1])
    pred = (rng.standard_normal(shape) * 3.0).astype(B.STORE[dtype]).astype(np.float64)
    gt = np.zeros(shape)
    if soft:
        gt[np.arange(shape[0]), rng.integers(0, shape[1], shape[0])] = 1.0
    else:
        gt = (rng.random(shape) > 0.7).astype(np.float64)
    return dict(pred=pred, gt=gt)


def ce_reference(kind, q):
    with np.errstate(all='ignore'):
        return (O.softmax_ce_loss if kind == 'softmax' else O.sigmoid_ce_loss)(q['pred'], q['gt'])


# ---- regularisers and optimizers ---------------------------------------------------------------------------------------------
def reg_reference(kind, w, g0, strength):
    with np.errstate(all='ignore'):
        loss, dg = (O.l1_reg if kind == 'l1' else O.l2_reg)(w, strength)
        return loss, g0 + dg


OPTIMIZERS = ('momentum', 'adam', 'rmsprop', 'momentum_fused', 'adam_fused')
OPT_HYPER = dict(momentum=(0.05, 0.9), adam=(0.0015, 0.9, 0.999), rmsprop=(0.01, 0.95))
OPT_RANGES = lambda n: [(('l2', 2.0 ** -7), 1, 1023), (('l1', 3 * 2.0 ** -8), 1023, 1026), (('l1', 2.0 ** -6), n - 3, n)]   # noqa: E731


def opt_spots(n, trip):
    """one NaN in the gradient at the first index, one at the last and one past the first grid trip of `trip` elements"""
    return (0, min(trip + 3, n - 2), n - 1)


def opt_reference(opt, w, g, v, a):
    """the oracle's step on float64 copies -> (w, v, a) (what an optimizer does not keep comes back unchanged)"""
    f32 = lambda x: float(np.float32(x))
    with np.errstate(all='ignore'):
        g = g.copy()
        if opt.endswith('_fused'):
            for (kind, strength), lo, hi in OPT_RANGES(w.size):
                g[lo:hi] += (O.l1_reg if kind == 'l1' else O.l2_reg)(w[lo:hi], strength)[1]
        base = opt.split('_')[0]
        hyper = tuple(f32(h) for h in OPT_HYPER[base])
        if base == 'momentum':
            ref = O.MomentumState(*hyper)
            ref.state['p'] = v
            return ref.update('p', w, g), ref.state['p'], a
        if base == 'adam':
            ref = O.AdamState(*hyper)
            ref.state['p'] = (v, a)
            return (ref.update('p', w, g),) + tuple(ref.state['p'])
        ref = O.RMSPropState(*hyper)
        ref.state['p'] = a
        return ref.update('p', w, g), v, ref.state['p']


# ---- families ----------------------------------------------------------------------------------------------------------------
def family(c):
    """the kernel family of a case of CASES / SIGMOID_CASES / WCASES: the kind of problem, the type, the options"""
    p = c.problem
    base = p.base if isinstance(p, B.SigmoidProblem) else p
    kind = ''.join(ch for ch in base.name.split('-')[0] if not ch.isdigit())
    return kind, p.dtype, type(p).__name__, tuple(sorted(c.opts.items()))


def minus_cases(cases):
    """ids of the first case of every family: the ones that also plant -Inf"""
    first = {}
    for c in cases:
        first.setdefault(family(c), c.id)
    return set(first.values())
