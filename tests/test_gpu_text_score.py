"""The text score on the GPU (csrc/text_score.hip) against the rules of tests/text_score_rules.py, which
tests/test_text_score_host.py pins.  Scores and ids EQUAL the rules in every dtype (`==`, no tolerance): the kernels compare
and count, and every input is a multiple of 1/64 -- the same number in binary16, float32 and float64 -- or a NaN.  All
sizes come from uocr_text_score_limits.  Then ops.text_score, the evaluate systems on generated pages, evaluate_text and
its command line."""
import ctypes as C
import json

import numpy as np
import pytest

import text_score_rules as T

pytestmark = pytest.mark.gpu

DTYPES = ('float32', 'float64', 'float16')
N_CHARS = 162
FILL = 0xFF                                                        # what every ids buffer holds before a call (no id is 255)
SLACK = 5                                                          # bytes of every ids buffer past the line's width
UNSET = -7                                                         # what the scores hold before a call


@pytest.fixture
def rt():
    from univer_ocr_amd.nn import CP
    CP.use_gpu(0)
    CP.set_dtype('float32')
    return CP, CP.runtime()


@pytest.fixture(scope='module')
def limits():
    """(rows per block, lines per launch, columns per panel, widest line) of the library"""
    from univer_ocr_amd.hip import lib as hiplib
    outs = [C.c_int(0) for _ in range(4)]
    assert hiplib.get_lib().uocr_text_score_limits(*[C.byref(out) for out in outs]) == 0
    rows, per_launch, panel, max_width = [out.value for out in outs]
    assert rows > 1 and per_launch > 0 and panel % 64 == 0 and panel > 0 and max_width > 2 * panel
    return rows, per_launch, panel, max_width


def tables():
    from univer_ocr_amd.my_model.crop import SIMILAR_PAIRS
    return {'identity': T.identity(N_CHARS), 'pairs': T.look_alikes_equal(SIMILAR_PAIRS, N_CHARS)}


# ---- hand-built matrices ---------------------------------------------------------------------------------------------------
def matrix(ids, rng, n_chars=N_CHARS):
    """(len(ids), n_chars) float64 of multiples of 1/64 whose row ids are `ids`: a row of id -1 is all zero, -0.0 over
    negatives, or holds a NaN; one row in seven of the others has a negative maximum; three in ten hold their maximum
    again in later columns"""
    M = rng.integers(-32, 17, (len(ids), n_chars)) / 64.0
    for r, i in enumerate(ids):
        kind = rng.random()
        if i < 0:
            if kind < 1 / 3:
                M[r] = 0.0
            elif kind < 2 / 3:
                M[r] = -np.abs(M[r]) - 1 / 64
                M[r, rng.integers(n_chars)] = -0.0
            else:
                M[r, rng.integers(n_chars)] = np.nan
        else:
            value = 0.5 + rng.integers(0, 17) / 64
            if kind < 1 / 7:
                M[r], value = -np.abs(M[r]) - 0.5, -0.25
            M[r, i] = value
            if kind > 0.7 and i + 1 < n_chars:
                M[r, rng.integers(i + 1, n_chars, 2)] = value
    assert T.row_ids(M) == list(ids)
    return M


def spread(string, rng):
    """row ids that read as `string`: every id a run of 1 to 3 rows; a tab or a row without a maximum between equal
    neighbours, one time in five between others, now and then in front"""
    out = [int(rng.choice([0, -1]))] * int(rng.integers(0, 3))
    for i in string:
        if out and (out[-1] == i or rng.random() < 0.2):
            out += [int(rng.choice([0, -1]))] * int(rng.integers(1, 3))
        out += [int(i)] * int(rng.integers(1, 4))
    assert T.collapse(out) == [int(i) for i in string]
    return out


def line_of(expected, read, rng, n_chars=N_CHARS):
    """(pred, label) of one width whose readings are the strings `read` and `expected`"""
    rows_read, rows_expected = spread(read, rng), spread(expected, rng)
    w = max(len(rows_read), len(rows_expected), 1) + int(rng.integers(0, 3))
    pad = lambda ids: ids + [int(rng.choice([0, -1])) for _ in range(w - len(ids))]
    return matrix(pad(rows_read), rng, n_chars), matrix(pad(rows_expected), rng, n_chars)


def strings(m, n, rng):
    """an expected string of m ids, most of them halves of look-alike pairs, and a read string of n made from it: a slice
    or an extension, one id in seven replaced, one in seven swapped for its look-alike"""
    from univer_ocr_amd.my_model.crop import SIMILAR_PAIRS
    partner = {**{a: b for a, b in SIMILAR_PAIRS}, **{b: a for a, b in SIMILAR_PAIRS}}
    pool = sorted(partner) + [1, 3, 70, 130, 161]
    expected = rng.choice(pool, m).tolist()
    start = int(rng.integers(0, m - n + 1)) if n < m else 0
    read = expected[start:start + n] + rng.choice(pool, max(0, n - m)).tolist()
    for k in range(n):
        u = rng.random()
        if u < 1 / 7:
            read[k] = int(rng.choice(pool))
        elif u < 2 / 7 and read[k] in partner:
            read[k] = partner[read[k]]
    return expected, read


def raw_call(runtime, dtype, pred, label, w, n_chars, canon, read_ids, expected_ids, scores, n_lines=None):
    """uocr_text_score on lists of device addresses (None = a null entry; a list that is None: a null array)"""
    from univer_ocr_amd.hip import lib as hiplib
    n = len(w) if n_lines is None else n_lines
    pointers = lambda values: None if values is None else (C.c_void_p * len(values))(*values)
    ints = lambda values: None if values is None else (C.c_int * len(values))(*[int(v) for v in values])
    code = dtype if isinstance(dtype, int) else hiplib.dtype_code(dtype)
    runtime.call('uocr_text_score', code, n, pointers(pred), pointers(label), ints(w), n_chars, ints(canon), pointers(read_ids),
                 pointers(expected_ids), scores)


class Outputs:
    """ids buffers of w + SLACK bytes, filled with FILL, and (n + 1, 4) scores that start as UNSET"""

    def __init__(self, CP, widths):
        self.CP, self.n = CP, len(widths)
        self.read = [CP.copy(np.full(w + SLACK, FILL, np.uint8), np.uint8) for w in widths]
        self.expected = [CP.copy(np.full(w + SLACK, FILL, np.uint8), np.uint8) for w in widths]
        self.scores = CP.copy(np.full((self.n + 1, 4), UNSET, np.int32), np.int32)

    def host(self):
        scores = self.CP.asnumpy(self.scores)
        assert (scores[self.n] == UNSET).all(), 'written behind the scores'
        return scores[:self.n], [self.CP.asnumpy(a) for a in self.read], [self.CP.asnumpy(a) for a in self.expected]

    def untouched(self):
        scores, read, expected = self.host()
        return (scores == UNSET).all() and all((v == FILL).all() for v in read + expected)


def upload(CP, x, dtype, offset=0):
    """x on the device in dtype, `offset` elements behind the start of its buffer: (buffer, address)"""
    flat = np.concatenate([np.zeros(offset), x.reshape(-1)])
    buffer = CP.copy(flat, dtype)
    return buffer, buffer.ptr + offset * np.dtype(dtype).itemsize


def run_lines(rt, lines, canon, dtype='float32', want=None, with_ids=True, offsets=(0, 0), what=''):
    """ONE uocr_text_score call on host (pred, label) pairs: scores and ids EQUAL `want` (default: the rules'), and no byte
    behind a reading was touched.  Returns the scores."""
    CP, runtime = rt
    want = [T.score(pred, label, canon) for pred, label in lines] if want is None else want
    widths = [pred.shape[0] for pred, _ in lines]
    preds = [upload(CP, pred, dtype, offsets[0]) for pred, _ in lines]
    labels = [upload(CP, label, dtype, offsets[1]) for _, label in lines]
    out = Outputs(CP, widths)
    raw_call(runtime, dtype, [p for _, p in preds], [p for _, p in labels], widths, lines[0][0].shape[1], canon,
             [a.ptr for a in out.read] if with_ids else None, [a.ptr for a in out.expected] if with_ids else None, out.scores.ptr)
    scores, read, expected = out.host()
    for i, ((d, m, n), read_ids, expected_ids) in enumerate(want):
        where = f'{what} line {i} (w {widths[i]}, expected {m}, read {n}) {dtype}'
        assert scores[i].tolist() == [d, m, n, 0], f'{where}: scores {scores[i].tolist()}, the rules say {[d, m, n, 0]}'
        if with_ids:
            assert read[i][:n].tolist() == read_ids and expected[i][:m].tolist() == expected_ids, f'{where}: ids differ'
            assert (read[i][n:] == FILL).all() and (expected[i][m:] == FILL).all(), f'{where}: bytes behind a reading were written'
        else:
            assert (read[i] == FILL).all() and (expected[i] == FILL).all()
    return scores


_cases = {}


def length_cases(limits):
    """the lines of the length test and what the rules say of them under both tables, made once"""
    if not _cases:
        rows, _, panel, _ = limits
        assert rows == 64, 'the lengths below are written around chunks of 64 rows'
        per_lane = range(1, panel // 64 + 1)
        expected_lengths = sorted({0, 1, 63, 64, 65, panel + 1, panel + 65} | {64 * k + d for k in per_lane for d in (-1, 0, 1)})
        read_lengths = [0, 1, 2, 63, 64, 65, 300]
        pairs = [(m, read_lengths[(k + shift) % 7]) for k, m in enumerate(expected_lengths) for shift in (0, 3)]
        pairs += [(0, 0), (0, 300), (panel, 300), (panel + 1, 300), (panel + 65, 300), (panel + 65, 65), (2 * panel + 3, 40)]
        rng = np.random.default_rng(60)
        lines = [line_of(*strings(m, n, rng), rng) for m, n in pairs]
        a, b = 7, 9
        runs = [[a] * 70 + [0] + [a] * 60 + [b] * 10,              # a run across a block and a chunk border; one from row 64 + 7 on
                [b] * 64 + [b] * 3 + [a] * 61 + [b],                # across row 63 | 64; a new run from row 128 on
                [a] * 64 + [b] * 64 + [-1] + [b],                   # a new run exactly at row 64; a run ended by a row without a maximum
                [a] * 63 + [0] + [a] * 64 + [a],                    # the tab in row 63: the same id starts again at row 64
                [a] * 63 + [-1] + [a] * 70]
        assert [T.collapse(r) for r in runs] == [[a, a, b], [b, a, b], [a, b, b], [a, a], [a, a]]
        for k, ids in enumerate(runs):
            other = runs[(k + 1) % len(runs)]
            w = max(len(ids), len(other))
            lines.append((matrix(ids + [0] * (w - len(ids)), rng), matrix(other + [0] * (w - len(other)), rng)))
        _cases['lines'], _cases['pairs'] = lines, pairs
        for name, canon in tables().items():
            _cases[name] = [T.score(pred, label, canon) for pred, label in lines]
        for (m, n), ((_, got_m, got_n), _, _) in zip(pairs, _cases['identity']):
            assert (m, n) == (got_m, got_n)
        differing = sum(a[0] != b[0] for a, b in zip(_cases['identity'], _cases['pairs']))
        assert differing > len(lines) // 4, 'the table matters'
    return _cases


@pytest.mark.parametrize('table', ['identity', 'pairs'])
@pytest.mark.parametrize('dtype', DTYPES)
def test_scores_and_ids_equal_the_rules_at_every_length(dtype, table, limits, rt):
    cases = length_cases(limits)
    run_lines(rt, cases['lines'], tables()[table], dtype, want=cases[table], what=table)


@pytest.mark.parametrize('dtype', DTYPES)
def test_matrices_off_the_vector_alignment(dtype, limits, rt):
    """both matrices one and three elements behind a 16-byte border (n_chars = 162 moves the head of every row besides):
    every row has a scalar head and tail; the maximum sits in the first and in the last columns of some rows"""
    rng = np.random.default_rng(61)
    canon = tables()['pairs']
    ids = [1, 1, N_CHARS - 1, N_CHARS - 1, 2, N_CHARS - 2, 0, 1, 3, N_CHARS - 1] * 7
    lines = [(matrix(ids, rng), matrix(ids[::-1], rng)), line_of(*strings(70, 66, rng), rng)]
    want = [T.score(pred, label, canon) for pred, label in lines]
    for offsets in ((1, 3), (3, 1), (2, 5)):
        run_lines(rt, lines, canon, dtype, want=want, offsets=offsets, what=f'offsets {offsets}')


@pytest.mark.parametrize('n_chars', [1, 2, 63, 64, 65, 255])
def test_class_counts(n_chars, limits, rt):
    rng = np.random.default_rng(62 + n_chars)
    canon = rng.integers(0, n_chars, n_chars).astype(np.int32)
    lines = []
    for w in (1, 66, 130):
        ids = [rng.integers(-1, n_chars, w).tolist() for _ in range(2)]
        lines.append((matrix(ids[0], rng, n_chars), matrix(ids[1], rng, n_chars)))
    for dtype in DTYPES:
        run_lines(rt, lines, canon, dtype, what=f'n_chars={n_chars}')


# ---- launch grouping, optional outputs -----------------------------------------------------------------------------------
def test_more_lines_than_one_launch_takes(limits, rt):
    rows, per_launch, _, _ = limits
    rng = np.random.default_rng(63)
    canon = tables()['pairs']
    lengths = [(int(rng.integers(0, 6)), int(rng.integers(0, 6))) if i % 9 else (rows + 3, rows - 2) for i in range(per_launch + 1)]
    lines = [line_of(*strings(m, n, rng), rng) for m, n in lengths]
    assert len({pred.shape[0] for pred, _ in lines}) > 5, 'the widths differ'
    want = [T.score(pred, label, canon) for pred, label in lines]
    assert len({w[0] for w in want}) > 3
    run_lines(rt, lines, canon, want=want, what='two launch pairs')
    for i in (0, per_launch - 1, per_launch):                       # the first and the last line of each launch, alone
        run_lines(rt, [lines[i]], canon, want=[want[i]], what=f'line {i} alone')
    run_lines(rt, lines[:per_launch], canon, want=want[:per_launch], what='exactly one group')


def test_optional_outputs(limits, rt):
    cases = length_cases(limits)
    lines, want = cases['lines'][::5], cases['pairs'][::5]
    with_ids = run_lines(rt, lines, tables()['pairs'], want=want, with_ids=True)
    without = run_lines(rt, lines, tables()['pairs'], want=want, with_ids=False)
    assert with_ids.tobytes() == without.tobytes()


# ---- arguments -----------------------------------------------------------------------------------------------------------
def test_argument_errors_write_nothing(limits, rt):
    from univer_ocr_amd.hip import HipError
    CP, runtime = rt
    _, _, _, max_width = limits
    rng = np.random.default_rng(64)
    canon = tables()['pairs'].tolist()
    lines = [line_of(*strings(5, 4, rng), rng), line_of(*strings(9, 9, rng), rng)]
    widths = [pred.shape[0] for pred, _ in lines]
    x = [CP.copy(pred, np.float32) for pred, _ in lines]
    y = [CP.copy(label, np.float32) for _, label in lines]
    out = Outputs(CP, widths)
    read_ptr, expected_ptr = [a.ptr for a in out.read], [a.ptr for a in out.expected]
    good = dict(dtype='float32', pred=[a.ptr for a in x], label=[a.ptr for a in y], w=widths, n_chars=N_CHARS, canon=canon,
                read_ids=read_ptr, expected_ids=expected_ptr, scores=out.scores.ptr, n_lines=2)
    bad = [(dict(pred=None), -1), (dict(label=None), -1), (dict(w=None), -1), (dict(canon=None), -1), (dict(scores=None), -1),
           (dict(n_lines=-1), -1), (dict(pred=[x[0].ptr, None]), -1), (dict(label=[None, y[1].ptr]), -1),
           (dict(w=[widths[0], 0]), -1), (dict(w=[-3, widths[1]]), -1), (dict(w=[widths[0], max_width + 1]), -1),
           (dict(n_chars=0), -1), (dict(n_chars=256, canon=[0] * 256), -1), (dict(canon=canon[:-1] + [N_CHARS]), -1),
           (dict(canon=[-1] + canon[1:]), -1), (dict(pred=[x[0].ptr, x[1].ptr + 2]), -1),
           (dict(label=[y[0].ptr + 2, y[1].ptr]), -1), (dict(scores=out.scores.ptr + 2), -1), (dict(dtype=7), -2)]
    for change, code in bad:
        with pytest.raises(HipError, match=rf'\({code}\)'):
            raw_call(runtime, **dict(good, **change))
        assert out.untouched(), f'{change}: the outputs were touched'
    raw_call(runtime, **dict(good, n_lines=0))                     # nothing to do: OK, no launch
    raw_call(runtime, 'float32', None, None, None, N_CHARS, None, None, None, None, n_lines=0)   # ... whatever else is passed
    assert out.untouched()
    raw_call(runtime, **good)
    scores = out.host()[0]
    assert scores.tolist() == [[*T.score(pred, label, canon)[0], 0] for pred, label in lines]


# ---- repeatability, capture ----------------------------------------------------------------------------------------------
def test_second_call_after_a_larger_one_and_repeatability(limits, rt):
    """row ids, readings and boundary columns of a larger call stay in the workspace: a smaller call must not read them;
    the same call twice gives the same bytes"""
    _, _, panel, _ = limits
    rng = np.random.default_rng(65)
    canon = tables()['identity']
    big = [line_of(*strings(panel + 70, 200, rng), rng), line_of(*strings(150, 2 * panel, rng), rng)]
    small = [line_of(*strings(66, 3, rng), rng), line_of(*strings(0, 0, rng), rng), line_of(*strings(5, 70, rng), rng)]
    first = run_lines(rt, big, canon, what='big')
    run_lines(rt, small, canon, what='small after big')
    again = run_lines(rt, big, canon, what='big again')
    assert first.tobytes() == again.tobytes()


def test_capture_and_replay(limits, rt):
    """the call is asynchronous and capturable: a replayed graph scores what the input buffers hold then"""
    import torch
    CP, runtime = rt
    _, _, panel, _ = limits
    rng = np.random.default_rng(66)
    canon = tables()['pairs']
    widths = (5 * panel + 7, 130)
    versions = []
    for _ in range(2):
        lines = []
        for w, (m, n) in zip(widths, ((panel + 3, 90), (20, 24))):
            rows_read, rows_expected = (spread(s, rng) for s in strings(m, n, rng)[::-1])
            assert max(len(rows_read), len(rows_expected)) <= w
            lines.append((matrix(rows_read + [0] * (w - len(rows_read)), rng), matrix(rows_expected + [0] * (w - len(rows_expected)), rng)))
        versions.append(lines)
    x = [CP.copy(pred, np.float32) for pred, _ in versions[0]]
    y = [CP.copy(label, np.float32) for _, label in versions[0]]
    out = Outputs(CP, widths)
    with runtime.capture(torch.cuda.MemPool()) as graph:
        raw_call(runtime, 'float32', [a.ptr for a in x], [a.ptr for a in y], widths, N_CHARS, canon, [a.ptr for a in out.read],
                 [a.ptr for a in out.expected], out.scores.ptr)
    seen = set()
    for lines in versions[::-1] + versions:
        for a, b, (pred, label) in zip(x, y, lines):
            a.set(pred), b.set(label)
        for a in out.read + out.expected:
            a.set(np.full(a.shape, FILL, np.uint8))
        graph.replay()
        scores, read, expected = out.host()
        for i, (pred, label) in enumerate(lines):
            (d, m, n), read_ids, expected_ids = T.score(pred, label, canon)
            assert scores[i].tolist() == [d, m, n, 0]
            assert read[i][:n].tolist() == read_ids and (read[i][n:] == FILL).all()
            assert expected[i][:m].tolist() == expected_ids and (expected[i][m:] == FILL).all()
        seen.add(scores.tobytes())
    assert len(seen) == 2, 'the two versions score differently'


# ---- ops.text_score --------------------------------------------------------------------------------------------------------
def test_wrapper_makes_one_call_and_one_readback(limits, rt, monkeypatch):
    from univer_ocr_amd.my_model.crop import CHARS, ScoreText
    from univer_ocr_amd.nn import ops
    from univer_ocr_amd.nn.gpu import DeviceArray
    CP, runtime = rt
    cases = length_cases(limits)
    canon = tables()['pairs']
    pick = slice(0, None, 4)
    lines, want = cases['lines'][pick], cases['pairs'][pick]
    calls, readbacks = [], []
    original, numpy = runtime.call, DeviceArray.numpy
    monkeypatch.setattr(runtime, 'call', lambda name, *args: (calls.append(name), original(name, *args))[1])
    monkeypatch.setattr(DeviceArray, 'numpy', lambda self: (readbacks.append(self.shape), numpy(self))[1])
    for dtype in DTYPES:
        preds = [CP.copy(pred, dtype) for pred, _ in lines]
        labels = [CP.copy(label, dtype) for _, label in lines]
        del calls[:], readbacks[:]
        scores = ops.text_score(preds, labels, canon)
        assert calls.count('uocr_text_score') == 1 and len(readbacks) == 1
        assert scores.dtype == np.int32 and scores.tolist() == [list(w[0]) for w in want]
        del calls[:], readbacks[:]
        scores, read, expected = ops.text_score(preds, labels, canon, want_ids=True)
        assert calls.count('uocr_text_score') == 1 and len(readbacks) == 1
        assert scores.tolist() == [list(w[0]) for w in want] and read == [w[1] for w in want] and expected == [w[2] for w in want]
        del calls[:], readbacks[:]
        nested = ScoreText()([preds[:2], [], preds[2:]], [labels[:2], [], labels[2:]])
        assert calls.count('uocr_text_score') == 1 and len(readbacks) == 1
        text = lambda ids: ''.join(CHARS[i] for i in ids)
        for k, pick_of in enumerate((lambda w: w[0], lambda w: text(w[1]), lambda w: text(w[2]))):
            assert nested[k] == [[pick_of(w) for w in want[:2]], [], [pick_of(w) for w in want[2:]]]
    del calls[:], readbacks[:]
    empty = ops.text_score([], [], canon)
    assert empty.shape == (0, 3) and ops.text_score([], [], canon, want_ids=True)[1:] == ([], [])
    assert ScoreText()([], []) == ([], [], []) and ScoreText()([[]], [[]]) == ([[]], [[]], [[]])
    assert 'uocr_text_score' not in calls and readbacks == [], 'nothing to score: no call, no copy'
    a, b = CP.copy(lines[0][0], np.float32), CP.copy(lines[1][1], np.float32)
    assert a.shape != b.shape
    for args in (([a], [b], canon), ([a], [a, a], canon), ([a], [a], canon[:-1]), ([a], [CP.copy(lines[0][1], np.float64)], canon),
                 ([lines[0][0]], [a], canon)):
        with pytest.raises(ValueError, match='text_score'):
            ops.text_score(*args)
    assert 'uocr_text_score' not in calls
    monkeypatch.undo()


# ---- the systems -------------------------------------------------------------------------------------------------------------
def check_scores_against_the_rules(CP, context, similar=True):
    """text_scores, read_text and expected_text of a context equal the rules applied to its downloaded char_pred and
    char_labels; returns the number of lines"""
    from univer_ocr_amd.my_model.crop import CHARS, canonical_ids
    canon = canonical_ids(similar=similar)
    text = lambda ids: ''.join(CHARS[i] for i in ids)
    crops = context['cropped_2_monochrome']
    assert [len(p) for p in context['text_scores']] == [len(p) for p in crops] == [len(p) for p in context['char_labels']]
    assert [len(p) for p in context['read_text']] == [len(p) for p in crops] == [len(p) for p in context['expected_text']]
    assert [len(p) for p in context['text']] == [len(p) for p in crops]
    lines = 0
    for p, paragraph in enumerate(crops):
        for l, crop in enumerate(paragraph):
            pred, label = CP.asnumpy(context['char_pred'][p][l]), CP.asnumpy(context['char_labels'][p][l])
            assert pred.shape == label.shape == (crop.shape[2], N_CHARS)
            scores, read, expected = T.score(pred, label, canon)
            assert context['text_scores'][p][l] == scores, f'text_scores[{p}][{l}]'
            assert context['read_text'][p][l] == text(read) and context['expected_text'][p][l] == text(expected)
            lines += 1
    return lines


def test_evaluate_system_on_the_true_crops(rt):
    from univer_ocr_amd.my_model.crop import ScoreText
    from univer_ocr_amd.my_model.model import make_evaluate_context_maker, make_evaluate_system
    from univer_ocr_amd.my_model.pages import GeneratedPages, PagesWithText
    CP, _ = rt
    np.random.seed(0)
    source = GeneratedPages(1, 256, 512, seed=31, length=1)
    pages = PagesWithText(source, 1)
    system, models, names = make_evaluate_system((1, 32, 64, 1), crops='true')
    assert names == ['ParagraphCrop', 'LineCrop', 'CharLabel', 'Char', 'PredToText', 'TextScore'] and list(models) == ['Char']
    assert len(system.components) == len(names)
    context = make_evaluate_context_maker('true')(pages.get, (0,))
    system.predict(context)
    boxes = source.tables(None, first_page=pages.page_of(0), n_pages=1)['paragraphs'].numpy()[0]
    typed = pages.texts(0)
    reading_order = sorted(range(len(typed)), key=lambda p: (boxes[p, 1], boxes[p, 0]))       # the order of the labelling
    assert len(typed) >= 2 and context['expected_text'] == [typed[p] for p in reading_order]
    scores, read, expected = ScoreText()(context['char_labels'], context['char_labels'])
    assert read == expected == context['expected_text']
    assert scores == [[(0, len(line), len(line)) for line in paragraph] for paragraph in expected]
    assert check_scores_against_the_rules(CP, context) == sum(len(p) for p in typed)


def plant_true_paragraphs_and_two_lines(system, names, pages, index):
    """behind the untrained Paragraph and Line nets (which still run): the page's paragraph layer, and two planted lines
    per paragraph crop"""
    from test_gpu_pred_to_text import planted_lines
    from univer_ocr_amd.nn import CP
    from univer_ocr_amd.nn.model_system import RawFunctionComponent

    def plant_paragraphs(context):
        context['paragraph_pred'] = pages.get(index, ['paragraph'])['paragraph']

    def plant_lines(context):
        context['line_pred'] = [CP.copy(planted_lines(crop.shape)) for crop in context['cropped_monochrome']]
    system.components.insert(names.index('ParagraphCrop'), RawFunctionComponent(plant_paragraphs))
    system.components.insert(names.index('LineCrop') + 1, RawFunctionComponent(plant_lines))


def test_evaluate_system_on_predicted_crops(rt):
    from test_gpu_models import set_analytic_weights
    from univer_ocr_amd.my_model.evaluate import evaluate_text
    from univer_ocr_amd.my_model.model import make_evaluate_context_maker, make_evaluate_system
    from univer_ocr_amd.my_model.pages import GeneratedPages, PagesWithText
    from univer_ocr_amd.nn.model_system import RawFunctionComponent
    CP, _ = rt
    pages = PagesWithText(GeneratedPages(1, 64, 128, seed=12, length=2), 2)
    assert sum(len(paragraph) for paragraph in pages.texts(0)) > 0, 'the page holds text'
    make_context = make_evaluate_context_maker('predicted')
    expected_names = ['Monochrome', 'Paragraph', 'ParagraphCrop', 'Line', 'LineCrop', 'CharLabel', 'Char', 'PredToText', 'TextScore']
    # whatever the untrained nets find
    np.random.seed(0)
    system, models, names = make_evaluate_system((1, 64, 128, 1), crops='predicted', find_rotation=False)
    assert names == expected_names and len(system.components) == len(names) and sorted(models) == ['Char', 'Line', 'Monochrome', 'Paragraph']
    context = make_context(pages.get, (0,))
    assert sorted(context) == ['char', 'monochrome_X']
    system.predict(context)
    found = check_scores_against_the_rules(CP, context)
    print(f'the untrained nets found {len(context["cropped_monochrome"])} paragraphs and {found} lines')
    # true paragraphs, two planted lines in each: the labels ride with the crops, one Char pass per line or one per page
    # (analytic weights, whose maxima are clear of the rounding that separates the two passes: tests/test_gpu_char_lines.py)
    results = {}
    for batching in ('line', 'page'):
        system, models, names = make_evaluate_system((1, 64, 128, 1), crops='predicted', find_rotation=False, char_batching=batching)
        for model in models.values():
            set_analytic_weights(model)
        plant_true_paragraphs_and_two_lines(system, names, pages, 0)
        context = make_context(pages.get, (0,))
        system.predict(context)
        assert check_scores_against_the_rules(CP, context) == 2 * len(pages.texts(0)) > 0
        results[batching] = (context['text_scores'], context['read_text'], context['expected_text'])
        assert any(n_expected > 0 for paragraph in context['text_scores'] for _, n_expected, _ in paragraph), 'the crops hold labels'
    assert results['line'] == results['page']
    # a page on which nothing is found
    np.random.seed(0)
    system, _, names = make_evaluate_system((1, 64, 128, 1), crops='predicted', find_rotation=False)

    def no_paragraph(context):
        context['paragraph_pred'] = CP.copy(np.zeros((1, 64, 128, 1)))
    system.components.insert(names.index('ParagraphCrop'), RawFunctionComponent(no_paragraph))
    contexts = []
    report = evaluate_text(pages, 1, system, crops='predicted', contexts=contexts)
    for key in ('cropped_2_monochrome', 'char_labels', 'text', 'text_scores', 'read_text', 'expected_text'):
        assert contexts[0][key] == [], key
    assert 'char_pred' not in contexts[0]
    assert report.pages == 1 and report.lines == 0 and report.cer is None and report.coverage == 0.0
    assert report.typed_chars == sum(len(line) for paragraph in pages.texts(0) for line in paragraph) > 0


def test_evaluate_text_and_its_command_line(rt, capsys):
    from univer_ocr_amd.my_model import evaluate
    from univer_ocr_amd.my_model.pages import GeneratedPages, PagesWithText
    CP, _ = rt
    np.random.seed(0)
    pages = PagesWithText(GeneratedPages(1, 96, 384, seed=77, length=2), 2)
    contexts = []
    report = evaluate.evaluate_text(pages, 2, contexts=contexts)
    assert isinstance(report, evaluate.TextReport) and len(contexts) == 2
    assert report._fields == ('pages', 'lines', 'exact_lines', 'typed_chars', 'expected_chars', 'read_chars', 'distance', 'cer', 'coverage')
    scores = [score for context in contexts for paragraph in context['text_scores'] for score in paragraph]
    typed = [line for i in range(2) for paragraph in pages.texts(i) for line in paragraph]
    assert report.pages == 2 and report.lines == len(scores) == len(typed) > 0
    assert report.typed_chars == sum(len(line) for line in typed)
    assert (report.distance, report.expected_chars, report.read_chars) == tuple(sum(s[k] for s in scores) for k in range(3))
    assert report.exact_lines == sum(s[0] == 0 for s in scores)
    assert report.coverage == 1.0 and report.cer == report.distance / report.expected_chars
    for context in contexts:
        check_scores_against_the_rules(CP, context)
    # the command line: one JSON line with the same fields
    capsys.readouterr()
    np.random.seed(0)
    evaluate.main(['--pages', '2', '--height', '96', '--width', '384', '--seed', '77'])
    printed = capsys.readouterr().out.strip().split('\n')
    assert len(printed) == 1
    assert json.loads(printed[0]) == report._asdict(), 'the same seed, the same weights: the same report'
    np.random.seed(0)
    evaluate.main(['--pages', '1', '--height', '96', '--width', '384', '--seed', '77', '--distinct-look-alikes', '--page-line-labels'])
    distinct = json.loads(capsys.readouterr().out)
    assert list(distinct) == list(report._fields) and distinct['pages'] == 1 and distinct['coverage'] == 1.0
