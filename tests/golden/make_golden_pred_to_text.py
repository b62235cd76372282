#!/usr/bin/env python3
"""Generate tests/golden/pred_to_text.npz: inputs and expected outputs of the PredToText stage and of a
[Char, PredToText] model system, taken from the REFERENCE (needs the reference checkout; see make_golden.py, whose
import stand-ins this script reuses by importing it).

    python tests/golden/make_golden_pred_to_text.py

Route taken: every text is the return value of the reference's `PredToText._func1` (interpreter/interpreter.py:596-614),
called directly -- constructing `PredToText` would start its worker pool.  Only inputs and outputs are stored.

Contents
  chars   the reference's 162 characters as a unicode array; pairs (18, 2) int32: the look-alike pairs
          (SIMILAR_CHARS_PAIRS_LIST) as positions in chars; cls (162,) int32: the pair of every character, -1 for none
  (a) ops line_names; per line {name}/x (W, 162) float64, {name}/text (the str _func1 returned, as a unicode array),
          {name}/ids int32: the positions of the text's characters in chars.  Lines:
            hand   built row by row: a paired character twice, an unpaired one twice, a Cyrillic / Latin look-alike in
                   both orders, a look-alike pair separated by a tab row (both emitted), by an all-zero row (the second
                   dropped), by a NaN row (the second dropped), a row whose maximum is -0.0, a row of negatives whose
                   maximum is -0.5 (emits), a two-way tie whose candidates are a look-alike pair, a tie with column 0,
                   a row with all 162 equal and not zero
            w1     one row
            w8, w17, w64, w130, w300   random rows with one clear maximum each, the ids drawn so that about a third of
                   the adjacent pairs fall in one pair class and a tenth are tabs
            ties   every row an exact 2- or 3-way tie: more ids than rows
            zeros  every row's maximum is 0 (or -0.0): the text is ''
  (b) system  the page [[24, 40], [17]] of system/mono{p}_{l} (1, 32, W, 1), drawn as make_golden_char_label.gen_system
          draws its page; the reference's Char net (make_char, analytic weights), Model.predict on every line (the
          reference's CharSelector has no get_X of its own, so its ModelSystem.predict cannot walk lines: the loop of
          this project's CharSelector.get_X is made here); system/char_pred{p}_{l} (W, 162), system/text{p}_{l} and system/ids{p}_{l} from
          _func1 on every char_pred.  In every row the gap between the largest and the second largest output exceeds
          1e-3 x max|output of the line| (asserted; input seeds are tried in order until it holds), so a float32 net
          whose outputs agree with these to better than that finds the same maxima.

Every value of (a) is a multiple of 1/64 (exact in binary16) or a NaN, so ties and zeros are exact in float32, float64
and binary16 alike (asserted).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (installs the stand-ins, puts the reference on sys.path)
from make_golden_crops import sample_prediction, save_reproducible  # noqa: E402

from components.interpreter import interpreter as ref_interp  # noqa: E402
from components.my_model import model as ref_mm  # noqa: E402
from components.primitives import CHARS, CHARS_IDS, SIMILAR_CHARS_PAIRS_LIST  # noqa: E402

MARGIN = 1e-3
N_CHARS = len(CHARS)
PAIRS = np.array([[CHARS_IDS[c] for c in pair] for pair in SIMILAR_CHARS_PAIRS_LIST], np.int32)
CLS = np.full(N_CHARS, -1, np.int32)
for _index, _pair in enumerate(PAIRS):
    CLS[_pair] = _index
assert N_CHARS == 162 and PAIRS.shape == (18, 2) and len(set(PAIRS.reshape(-1).tolist())) == 36
PAIRED, UNPAIRED = np.flatnonzero(CLS >= 0), np.flatnonzero(CLS[1:] < 0) + 1

# ids the hand-built line uses
CYR_A, LAT_A, LAT_B, CYR_E, LAT_E, CYR_O, LAT_O, CYR_P, LAT_P, CYR_U, LAT_Y, ONE = 2, 78, 79, 7, 82, 17, 92, 19, 93, 22, 102, 69
assert (CHARS[LAT_A], CHARS[LAT_B], CHARS[LAT_E], CHARS[LAT_O], CHARS[LAT_P], CHARS[LAT_Y], CHARS[ONE]) == tuple('abeopy1')
assert CLS[CYR_A] == CLS[LAT_A] >= 0 and CLS[CYR_E] == CLS[LAT_E] >= 0 and CLS[CYR_O] == CLS[LAT_O] >= 0
assert CLS[CYR_P] == CLS[LAT_P] >= 0 and CLS[CYR_U] == CLS[LAT_Y] >= 0 and CLS[LAT_B] == CLS[ONE] == -1


def peaked(ids, r, low=(-32, 32), high=(48, 64)):
    """(len(ids), 162): multiples of 1/64 in low / 64 everywhere, one value in high / 64 at every row's id"""
    x = r.integers(low[0], low[1] + 1, (len(ids), N_CHARS))
    x[np.arange(len(ids)), ids] = r.integers(high[0], high[1] + 1, len(ids))
    return x / 64.0


def hand_built():
    r = np.random.default_rng(3)
    kinds = ([LAT_A, LAT_A, LAT_B, LAT_B, CYR_A, LAT_A, 0, LAT_A, CYR_A, 0, CYR_E, 0, LAT_E, CYR_O, 'zero', LAT_O, 0,
              CYR_P, 'nan', LAT_P, 'negative zero', 'negative', 'pair tie', 'tab tie', 'all equal'])
    x = peaked([k if isinstance(k, int) else 1 for k in kinds], r)
    for row, kind in enumerate(kinds):
        if kind == 'zero':
            x[row] = 0.0
        elif kind == 'nan':
            x[row, 40] = np.nan
        elif kind == 'negative zero':
            x[row] = -0.5
            x[row, 5] = -0.0
        elif kind == 'negative':
            x[row] = -np.abs(x[row]) - 1.0
            x[row, ONE] = -0.5
        elif kind == 'pair tie':
            x[row] = np.minimum(x[row], 0.25)
            x[row, [CYR_U, LAT_Y]] = 0.75
        elif kind == 'tab tie':
            x[row] = np.minimum(x[row], 0.25)
            x[row, [0, LAT_B]] = 0.5
        elif kind == 'all equal':
            x[row] = 0.25
    # a a | b b | cyr-a lat-a | tab | lat-a cyr-a | tab | cyr-e tab lat-e | cyr-o 0 lat-o | tab | cyr-p nan lat-p |
    # -0.0 | '1' at -0.5 | the tie cyr-u = lat-y | the tie tab = b | 0 .. 161
    expected = [LAT_A, LAT_B, LAT_B, CYR_A, LAT_A, CYR_E, LAT_E, CYR_O, CYR_P, ONE, CYR_U, LAT_B]
    return x, expected + walk(list(range(N_CHARS)), LAT_B)         # (`all equal` is walked with b remembered)


def walk(ids, remembered=None):
    """the reference's loop (:603-613) on ids, as the header of this file states it"""
    out = []
    for i in ids:
        if i == 0:
            remembered = None
        elif remembered is None or CLS[i] < 0 or CLS[remembered] != CLS[i]:
            out.append(i)
            remembered = i
    return out


def drawn_ids(w, r):
    """about a tenth tabs; after a paired id, four times in ten, a member of the same pair"""
    ids = []
    for _ in range(w):
        u = r.random()
        if u < 0.1:
            ids.append(0)
        elif ids and CLS[ids[-1]] >= 0 and u < 0.5:
            ids.append(int(r.choice(PAIRS[CLS[ids[-1]]])))
        else:
            ids.append(int(r.choice(PAIRED if r.random() < 0.6 else UNPAIRED)))
    return ids


def tied(w, r):
    x = r.integers(-32, 33, (w, N_CHARS))
    for row in range(w):
        columns = r.choice(N_CHARS, int(r.integers(2, 4)), replace=False)
        if row % 3 == 0:                                            # a tie inside one pair, now and then
            columns = PAIRS[r.integers(0, len(PAIRS))]
        x[row, columns] = 48
    return x / 64.0


def zeros(w, r):
    x = -r.integers(0, 33, (w, N_CHARS)) / 64.0
    x[np.arange(w), r.integers(0, N_CHARS, w)] = 0.0
    for row in x[1::3]:
        row[row == 0] = -0.0                                        # every third row: all its zeros are -0.0
    assert any(np.signbit(row[row == 0]).all() for row in x) and any(not np.signbit(row[row == 0]).any() for row in x)
    return x


def behaviours(x):
    """what the rules, as the header states them, meet in x: a set of names"""
    seen, remembered, separator, before_tab = set(), None, None, None
    with np.errstate(invalid='ignore'):
        maxima = np.max(x, axis=1)
    for row, m in zip(x, maxima):
        if np.isnan(m) or m == 0:
            separator = 'nan row' if np.isnan(m) else 'zero row'
            seen.add('negative zero maximum' if m == 0 and np.signbit(m) else separator)
            continue
        columns = np.flatnonzero(row == m).tolist()
        if m < 0:
            seen.add('negative maximum')
        if len(columns) == N_CHARS:
            seen.add('all equal')
        elif len(columns) > 1:
            seen.add('tie with the tab' if 0 in columns else 'tie')
            if len(columns) == 2 and CLS[columns[0]] >= 0 and CLS[columns[0]] == CLS[columns[1]]:
                seen.add('tie of a pair')
        for i in columns:
            if i == 0:
                remembered, separator = None, 'tab'
                continue
            same = remembered is not None and CLS[i] >= 0 and CLS[remembered] == CLS[i]
            if remembered == i:
                seen.add('paired twice: dropped' if same else 'unpaired twice: kept')
            elif same:
                seen.add(('cyrillic then latin' if remembered < i else 'latin then cyrillic') + ': dropped')
                if separator in ('zero row', 'nan row'):
                    seen.add(f'pair across a {separator}: dropped')
            elif separator == 'tab' and CLS[i] >= 0 and before_tab is not None and CLS[before_tab] == CLS[i]:
                seen.add('pair across a tab: kept')
            if not same:
                remembered = i
            before_tab, separator = i, None
    return seen


HAND_BEHAVIOURS = {'paired twice: dropped', 'unpaired twice: kept', 'cyrillic then latin: dropped', 'latin then cyrillic: dropped',
                   'pair across a tab: kept', 'pair across a zero row: dropped', 'pair across a nan row: dropped',
                   'negative zero maximum', 'negative maximum', 'tie of a pair', 'tie with the tab', 'all equal'}


def reference_text(x):
    text = ref_interp.PredToText._func1(x)                         # interpreter.py:596-614
    return text, np.array([CHARS_IDS[c] for c in text], np.int32)


def gen_ops(out):
    r = np.random.default_rng(7)
    hand, hand_ids = hand_built()
    lines = [('hand', hand), ('w1', peaked([LAT_B], r))]
    lines += [(f'w{w}', peaked(drawn_ids(w, r), r)) for w in (8, 17, 64, 130, 300)]
    lines += [('ties', tied(40, r)), ('zeros', zeros(12, r))]
    for name, x in lines:
        finite = x[~np.isnan(x)]
        assert np.array_equal(finite * 64, np.round(finite * 64)) and np.abs(finite).max() <= 2, f'{name}: not multiples of 1/64'
        assert np.array_equal(x, x.astype(np.float16).astype(np.float64), equal_nan=True), f'{name}: not exact in binary16'
        text, ids = reference_text(x)
        out[f'{name}/x'], out[f'{name}/text'], out[f'{name}/ids'] = x, np.array(text), ids
        print(f'{name:6s} {x.shape[0]:3d} rows: {len(ids):3d} ids  {text[:60]!r}')
    seen = behaviours(hand)
    assert seen >= HAND_BEHAVIOURS, HAND_BEHAVIOURS - seen
    assert out['hand/ids'].tolist() == hand_ids, (out['hand/ids'].tolist(), hand_ids)
    assert len(out['ties/ids']) > out['ties/x'].shape[0] and str(out['zeros/text']) == '' and len(out['w1/ids']) == 1
    for name in ('w64', 'w130', 'w300'):                            # what the drawn ids were meant to hold
        ids = np.argmax(out[f'{name}/x'], axis=1)
        same = np.mean((CLS[ids[1:]] >= 0) & (CLS[ids[1:]] == CLS[ids[:-1]]))
        assert 0.2 < same < 0.45 and 0.04 < np.mean(ids == 0) < 0.2, (name, same, np.mean(ids == 0))
    out['line_names'] = np.array([name for name, _ in lines])


def clear_maxima(pred):
    top = np.sort(pred, axis=1)[:, -2:]
    return np.min(top[:, 1] - top[:, 0]) > MARGIN * np.max(np.abs(pred))


def delisted(outputs):
    return outputs[0] if isinstance(outputs, list) else outputs


def gen_system(out):
    page = [[24, 40], [17]]
    for seed in range(21, 61):                                      # (21: the page of char_label.npz)
        r = np.random.default_rng(seed)
        monos = [[r.integers(0, 65, (1, 32, w, 1)) / 64.0 for w in widths] for widths in page]
        np.random.seed(11)
        char = ref_mm.make_char(monos[0][0].shape)
        mg.set_analytic_weights(char)
        preds = [[delisted(char.predict(x)) for x in per_line] for per_line in monos]   # one pass per line, as get_X of
        # this project's CharSelector walks the page (the reference's CharSelector defines get() only: its inherited
        # get_X hands ModelSystem.predict whole paragraphs, which no net takes)
        if all(clear_maxima(pred) for per_line in preds for pred in per_line):
            break
    else:
        raise AssertionError(f'no input seed gives every row a maximum that is clear by {MARGIN}')
    print(f'system: input seed {seed}')
    out['system/seed'] = np.array(seed)
    for p, per_line in enumerate(preds):
        for l, pred in enumerate(per_line):
            assert pred.shape == (page[p][l], N_CHARS)
            text, ids = reference_text(pred)
            out[f'system/mono{p}_{l}'] = monos[p][l]
            sample_prediction(f'system/char_pred{p}_{l}', pred, out)
            out[f'system/text{p}_{l}'], out[f'system/ids{p}_{l}'] = np.array(text), ids
            print(f'  line {p}.{l}: {len(ids)} ids {text[:50]!r}')


def main():
    out = {'chars': np.array(list(CHARS)), 'pairs': PAIRS, 'cls': CLS}
    gen_ops(out)
    gen_system(out)
    save_reproducible('pred_to_text', out)


if __name__ == '__main__':
    main()
