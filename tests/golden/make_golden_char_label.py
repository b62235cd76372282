#!/usr/bin/env python3
"""Generate tests/golden/char_label.npz: inputs and expected outputs of the CharLabel stage and of a [CharLabel, Char]
model system, taken from the REFERENCE (needs the reference checkout; see make_golden.py, whose import stand-ins this
script reuses by importing it).

    python tests/golden/make_golden_char_label.py

Route taken: every label array is the return value of the reference's `LabelChar._func1` (interpreter/interpreter.py:
547-571), called directly -- constructing `LabelChar` would start its worker pool.  Only inputs and outputs are stored.

Contents
  (a) ops     line_names; per line {name}/x (1, H, W, C) float64, {name}/labels (W, 162) float64 as _func1 returned them,
              {name}/ids int32 (W,) = the one-hot position of every row, -1 for a zero row.  Lines:
                hand      6 rows, 6 columns built by hand: a tie of two classes (the one that starts higher wins), the
                          same tie in the other order, "unknown" in the majority, a tie of "unknown" with a class with
                          "unknown" first, the same tie with the class first, all bits zero (class 0)
                constant  every element 0.5: nothing exceeds t, every column is class 0
                spacing   bits at 0.5, one letter_spacing element at 1.0: that channel alone sets the max and lifts t
                          above every bit (asserted: without it the labels are different)
                w8, w17, w64, w130, w33   H = 32, C = 9: a random class per column, 20-40 % of the pixels replaced by
                          other classes or by codes that are no class, so that the votes are contested
                ties      H = 4: two candidates with two rows each in most columns
                h5, h1    5 rows and 1 row
  (b) system  a page [[line, line], [line]] of widths 24, 40, 17 (H = 32): char{p}_{l} (1, 32, W, 9), mono{p}_{l}
              (1, 32, W, 1), labels{p}_{l} from _func1; the reference's Char net (make_char, analytic weights) trained
              by ONE ModelSystem.train call through the reference's CharSelector (one step per line), once with
              Momentum(lr=0.01, momentum=0) and once with Adam(lr=0.0015): accumulated losses, char_pred[p][l] and the
              final weights in the key format of paragraph_crop.npz under the prefixes sgd/ and adam/.

Every value is a multiple of 1/64 in [0, 1] (exact in binary16) and lies more than 1e-3 from its line's threshold
t = (mean + max) / 2 (asserted), so that a float32 or binary16 mean cannot flip a bit: the reference alone decides every
pixel.  The one exception is `constant`, where every element EQUALS t: the mean of n equal dyadic values is that value in
every float type and summation order, so `x > t` is false everywhere there too.
"""
import os
import sys
from collections import Counter

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (installs the stand-ins, puts the reference on sys.path)
from make_golden_crops import sample_prediction, save_reproducible  # noqa: E402

from components.interpreter import interpreter as ref_interp  # noqa: E402
from components.my_model import model as ref_mm  # noqa: E402
from components.nn import optimizers as ref_opt  # noqa: E402
from components.nn.model_system import ModelComponent, ModelSystem  # noqa: E402
from components.primitives import BITS_COUNT, CHARS  # noqa: E402

MARGIN = 1e-3
N_CHARS = len(CHARS)
C = BITS_COUNT + 1                                                 # bit_0 .. bit_7, letter_spacing (constants.py:22-25)
assert (BITS_COUNT, N_CHARS) == (8, 162)


def encode(codes, r, low=(0, 8), high=(56, 64)):
    """(1, H, W, C) from int codes (H, W): bit i of the code in channel i, least significant first; a set bit is a
    multiple of 1/64 in high / 64, a clear one in low / 64; letter_spacing gets a mixture of both"""
    h, w = codes.shape
    bits = (codes[:, :, None] >> np.arange(BITS_COUNT)) & 1
    bits = np.concatenate([bits, r.integers(0, 2, (h, w, 1))], axis=2)
    lo, hi = r.integers(low[0], low[1] + 1, bits.shape), r.integers(high[0], high[1] + 1, bits.shape)
    return (np.where(bits == 1, hi, lo) / 64.0)[None]


def contested(h, w, seed, replaced):
    """a class per column; `replaced` of the pixels become another class or (one in three) a code that is no class"""
    r = np.random.default_rng(seed)
    codes = np.repeat(r.integers(0, N_CHARS, (1, w)), h, axis=0)
    other = np.where(r.random((h, w)) < 1 / 3, r.integers(N_CHARS, 2 ** BITS_COUNT, (h, w)), r.integers(0, N_CHARS, (h, w)))
    codes = np.where(r.random((h, w)) < replaced, other, codes)
    return encode(codes, r)


def hand_built():
    codes = np.array([[5, 7, 200, 201, 9, 0],
                      [5, 7, 200, 202, 9, 0],
                      [5, 7, 201, 203, 9, 0],
                      [7, 5, 202, 9, 250, 0],
                      [7, 5, 3, 9, 251, 0],
                      [7, 5, 3, 9, 252, 0]])
    x = (((codes[:, :, None] >> np.arange(C)) & 1).astype(np.float64))[None]
    x[0, 0, 0, BITS_COUNT] = 1.0                                   # letter_spacing: in the statistics only
    return x, [5, 7, -1, -1, 9, 0]


def two_by_two(w, seed):
    r = np.random.default_rng(seed)
    a, b = r.integers(0, 200, w), r.integers(0, 200, w)
    order = r.integers(0, 3, w)                                    # a a b b / a b a b / a b b a
    rows = np.array([[0, 0, 1, 1], [0, 1, 0, 1], [0, 1, 1, 0]])[order].T
    return encode(np.where(rows == 0, a, b), r)


def threshold(x):
    return 0.5 * (np.mean(x) + np.max(x))


def ids_of(labels):
    assert set(np.unique(labels)) <= {0.0, 1.0} and labels.sum(axis=1).max() <= 1
    return np.where(labels.any(axis=1), labels.argmax(axis=1), -1).astype(np.int32)


def outcomes(x):
    """what happened in the columns of x, by the rules as the header states them: {'tie', 'unknown', 'zero'}"""
    bits = x[0, :, :, :BITS_COUNT] > threshold(x)
    codes = (bits * (1 << np.arange(BITS_COUNT))).sum(axis=2)
    seen = set()
    for column in codes.T:
        counts = Counter(int(c) if c < N_CHARS else -1 for c in column).most_common()
        if len(counts) > 1 and counts[0][1] == counts[1][1]:
            seen.add('tie')
        seen.add({-1: 'unknown', 0: 'zero'}.get(counts[0][0], 'class'))
    return seen


def check_margin(name, x):
    distance = np.min(np.abs(x - threshold(x)))
    assert distance > MARGIN, f'{name}: an element lies within {MARGIN} of the threshold'
    assert np.array_equal(x, x.astype(np.float16).astype(np.float64)) and x.min() >= 0 and x.max() <= 1


def gen_ops(out):
    r = np.random.default_rng(5)
    hand, hand_ids = hand_built()
    spacing = encode(np.repeat(r.integers(1, N_CHARS, (1, 12)), 7, axis=0), r, low=(0, 0), high=(32, 32))
    spacing[..., BITS_COUNT] = 0.0
    spacing[0, 3, 5, BITS_COUNT] = 1.0
    lines = [('hand', hand), ('constant', np.full((1, 9, 11, C), 0.5)), ('spacing', spacing),
             ('w8', contested(32, 8, 11, 0.2)), ('w17', contested(32, 17, 12, 0.4)), ('w64', contested(32, 64, 13, 0.3)),
             ('w130', contested(32, 130, 14, 0.35)), ('w33', contested(32, 33, 15, 0.4)), ('ties', two_by_two(29, 16)),
             ('h5', contested(5, 21, 17, 0.4)), ('h1', contested(1, 40, 18, 0.4))]
    seen = set()
    for name, x in lines:
        if name != 'constant':
            check_margin(name, x)
        labels = ref_interp.LabelChar._func1(x)                    # interpreter.py:547-571
        assert labels.shape == (x.shape[2], N_CHARS)
        out[f'{name}/x'], out[f'{name}/labels'], out[f'{name}/ids'] = x, labels, ids_of(labels)
        seen |= outcomes(x)
        print(f'{name:9s} {x.shape[1]:3d} x {x.shape[2]:3d} t = {threshold(x):.4f}: '
              f'{len(set(ids_of(labels).tolist()))} different rows, {int((ids_of(labels) < 0).sum())} zero rows')
    assert seen >= {'tie', 'unknown', 'zero'}, seen
    assert out['hand/ids'].tolist() == hand_ids, out['hand/ids']
    assert not out['constant/ids'].any() and not out['spacing/ids'].any()
    without = spacing.copy()
    without[..., BITS_COUNT] = 0.0
    assert ids_of(ref_interp.LabelChar._func1(without)).min() > 0, 'the letter_spacing channel does not decide `spacing`'
    out['line_names'] = np.array([name for name, _ in lines])


def gen_system(out):
    r = np.random.default_rng(21)
    page = [[24, 40], [17]]
    chars, monos, labels = [], [], []
    for p, widths in enumerate(page):
        chars.append([]), monos.append([]), labels.append([])
        for l, w in enumerate(widths):
            x = contested(32, w, 100 + 10 * p + l, 0.3)
            check_margin(f'char{p}_{l}', x)
            chars[p].append(x)
            monos[p].append(r.integers(0, 65, (1, 32, w, 1)) / 64.0)
            labels[p].append(ref_interp.LabelChar._func1(x))
            out[f'char{p}_{l}'], out[f'mono{p}_{l}'], out[f'labels{p}_{l}'] = x, monos[p][l], labels[p][l]
    for tag, make_opt in (('sgd', lambda: ref_opt.Momentum(lr=0.01, momentum=0)), ('adam', lambda: ref_opt.Adam(lr=0.0015))):
        np.random.seed(11)
        char = ref_mm.make_char(monos[0][0].shape, make_opt())
        mg.set_analytic_weights(char)
        system = ModelSystem([ModelComponent(
            'Char', char, ref_mm.CharSelector('cropped_2_monochrome', 'char_labels', 'char_pred'), delist_result=True)])
        context = {'cropped_2_monochrome': [list(m) for m in monos], 'char_labels': [list(v) for v in labels]}
        system.train(context)                                      # three steps: one per line
        entry = context['losses']['Char']
        assert len(entry['output_losses']) == 3 and [len(v) for v in context['char_pred']] == [2, 1]
        out[f'{tag}/train/Char/output_losses'] = np.array(entry['output_losses'])
        out[f'{tag}/train/Char/regularization_loss'] = np.array(entry['regularization_loss'])
        for p, per_line in enumerate(context['char_pred']):
            for l, pred in enumerate(per_line):
                assert pred.shape == (page[p][l], N_CHARS)
                sample_prediction(f'{tag}/train/char_pred{p}_{l}', pred, out)
        for pname, param in char.params().items():
            mg.sample_param(f'{tag}/final/{pname}', param.value, out)


def main():
    out = {}
    gen_ops(out)
    gen_system(out)
    save_reproducible('char_label', out)


if __name__ == '__main__':
    main()
