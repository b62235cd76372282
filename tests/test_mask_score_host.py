"""Host side of the mask score: the rules of tests/mask_score_rules.py -- the oracle of
tests/test_gpu_mask_score.py -- pinned against the reference's binary_classification_metrics (tests/golden/mask_score.npz),
against a brute-force loop over pairs of components, against hand-made planes, and against the property the component
count rests on: a match at an IoU above one half is mutual and unique.  Then the two entry points of the library as far as
they go without a GPU, and the adding-up of my_model/evaluate.py."""
import ctypes as C
import os

import numpy as np

import mask_score_rules as M
from conftest import ROOT, load_golden

NEW_SYMBOLS = {'uocr_label_overlap': 12, 'uocr_label_overlap_limits': 4}     # name -> arguments, the context included


# ---- pixel numbers against the reference -------------------------------------------------------------------------------------
def test_pixel_numbers_equal_the_reference():
    """The ints by equality; the ratios within rtol = 1e-12: both sides are at most six float64 roundings of exact
    integers, a bound near 1e-15 -- the margin stands three orders above that and far below any wrong formula."""
    golden = load_golden('mask_score')
    names = [str(name) for name in golden['names']]
    assert len(names) == 12
    for name in names:
        prediction, truth = golden[f'{name}/prediction'], golden[f'{name}/truth']
        table = M.overlap_table(truth, prediction, 0, 0)
        tp, fp, fn, tn = M.summary(table)[:4]
        counts = [int(((prediction == p) & (truth == t)).sum()) for p, t in ((1, 1), (1, 0), (0, 1), (0, 0))]
        assert [int(tp), int(fp), int(fn), int(tn)] == counts and min(counts) > 0, name
        assert table.tolist() == [[counts[3], counts[1]], [counts[2], counts[0]]], name
        for beta in (1, 2):
            mine = M.pixel_numbers(tp, fp, fn, tn, beta)
            assert None not in mine
            np.testing.assert_allclose(mine, golden[f'{name}/beta{beta}'], rtol=1e-12, atol=0, err_msg=f'{name} beta {beta}')


def test_ops_numbers_equal_the_rules():
    """what nn/ops.py derives on the host (f1beta = 1) is what the rules derive, to the bit, and None where they say None"""
    from univer_ocr_amd.nn.ops import mask_numbers
    rng = np.random.default_rng(5)
    cases = [tuple(int(v) for v in rng.integers(0, 4, 4) * rng.integers(0, 1000, 4)) for _ in range(300)] + [(0, 0, 0, 0)]
    nones = 0
    for tp, fp, fn, tn in cases:
        accuracy, precision, recall, f1 = M.pixel_numbers(tp, fp, fn, tn)
        got = mask_numbers(tp, fp, fn, tn)
        assert got == (precision, recall, f1, accuracy, M.ratio(tp, tp + fp + fn)), (tp, fp, fn, tn)
        nones += None in got
    assert 20 < nones < len(cases)


# ---- rows against brute force --------------------------------------------------------------------------------------------------
def random_planes(rng, h, w, components, noise):
    """rectangles that overwrite each other, numbered 1 .. components, and `noise` single pixels of any label"""
    plane = np.zeros((h, w), np.int32)
    for label in range(1, components + 1):
        y, x = rng.integers(0, h), rng.integers(0, w)
        plane[y:y + rng.integers(1, h // 2 + 2), x:x + rng.integers(1, w // 2 + 2)] = label
    ys, xs = rng.integers(0, h, noise), rng.integers(0, w, noise)
    plane[ys, xs] = rng.integers(0, components + 3, noise)
    return plane


def brute_rows(a, b, cap_a, cap_b):
    """rows by the words of the contract, a loop over the pairs of buckets"""
    ba, bb = M.bucket(a, cap_a), M.bucket(b, cap_b)
    rows = []
    for r in range(cap_a + 2):
        best, inter = 0, 0
        for s in range(1, cap_b + 1):
            count = int(((ba == r) & (bb == s)).sum())
            if count > inter:
                best, inter = s, count
        rows.append([int((ba == r).sum()), best, inter, int((bb == best).sum()) if best else 0])
    return np.array(rows, np.int64)


def test_rows_equal_a_brute_force_loop_and_matches_are_mutual_and_unique():
    rng = np.random.default_rng(11)
    matched_total = unmatched = 0
    for case in range(200):
        h, w = int(rng.integers(1, 24)), int(rng.integers(1, 24))
        cap_a, cap_b = int(rng.integers(0, 10)), int(rng.integers(0, 10))
        a = random_planes(rng, h, w, int(rng.integers(0, 7)), int(rng.integers(0, 10)))
        if case % 3:
            b = np.roll(a, int(rng.integers(-1, 2)), axis=1)              # mostly the same components: matches happen
            b[rng.integers(0, h), :] = rng.integers(0, 4)
        else:
            b = random_planes(rng, h, w, int(rng.integers(0, 7)), int(rng.integers(0, 10)))
        table, rows, cols, summary = M.everything(a, b, cap_a, cap_b)
        assert table.sum() == h * w
        assert np.array_equal(rows, brute_rows(a, b, cap_a, cap_b)), case
        assert np.array_equal(cols, brute_rows(b, a, cap_b, cap_a)), case
        assert summary[:4].sum() == h * w and summary[0] == ((a != 0) & (b != 0)).sum()
        # mutual and unique: the same count from the columns, every matched row is the best row of its best column, and
        # no column is the match of two rows
        is_match = lambda line: line[1] > 0 and 2 * line[2] > line[0] + line[3] - line[2]
        from_rows = [(r, int(rows[r, 1])) for r in range(1, cap_a + 1) if is_match(rows[r])]
        from_cols = [(int(cols[s, 1]), s) for s in range(1, cap_b + 1) if is_match(cols[s])]
        assert sorted(from_rows) == sorted(from_cols), case
        assert len({s for _, s in from_rows}) == len(from_rows) == summary[6]
        assert M.matched_ious(rows) == [table[r, s] / (rows[r, 0] + cols[s, 0] - table[r, s]) for r, s in from_rows]
        matched_total += len(from_rows)
        unmatched += int(summary[4]) - len(from_rows)
    assert matched_total > 50 and unmatched > 50, (matched_total, unmatched)       # (the cases hold both kinds)


def test_ties_go_to_the_smaller_index():
    a = np.array([[1, 1, 1, 1, 2, 2]], np.int32)
    b = np.array([[3, 3, 2, 2, 2, 1]], np.int32)
    table, rows, cols, summary = M.everything(a, b, 3, 3)
    assert rows[1].tolist() == [4, 2, 2, 3]                             # columns 2 and 3 overlap component 1 in 2 pixels each
    assert rows[2].tolist() == [2, 1, 1, 1]                             # and columns 1 and 2 component 2 in 1 each
    assert cols[2].tolist() == [3, 1, 2, 4] and cols[3].tolist() == [2, 1, 2, 4] and cols[1].tolist() == [1, 2, 1, 2]
    assert rows[0].tolist() == [0, 0, 0, 0] and rows[3].tolist() == [0, 0, 0, 0]
    assert summary.tolist() == [6, 0, 0, 0, 2, 3, 0, 0]
    # a tie between a component and the overflow or the background is no tie: neither is ever `best`
    table, rows, _, _ = M.everything(np.array([[1, 1, 1, 1, 1, 1]], np.int32), np.array([[0, 0, 9, 9, 2, 2]], np.int32), 1, 2)
    assert table[1].tolist() == [2, 0, 2, 2] and rows[1].tolist() == [6, 2, 2, 2]


def test_buckets_caps_and_strange_labels():
    top = 2 ** 31 - 1
    labels = np.array([0, 1, 3, 4, 5, top, -1, -2 ** 31], np.int32)
    assert M.bucket(labels, 4).tolist() == [0, 1, 3, 4, 5, 5, 5, 5]
    assert M.bucket(labels, 0).tolist() == [0, 1, 1, 1, 1, 1, 1, 1]
    assert M.bucket(labels, 3).tolist() == [0, 1, 3, 4, 4, 4, 4, 4]
    a = np.array([[0, 1, 3, 4, 5, top, -1, 2]], np.int32)
    b = np.array([[0, 1, 3, 3, 3, 3, 3, -7]], np.int32)
    table, rows, cols, summary = M.everything(a, b, 4, 3)
    assert table.shape == (6, 5) and table.sum() == 8
    assert table[5].tolist() == [0, 0, 0, 3, 0] and table[4, 3] == 1 and table[2, 4] == 1
    assert summary.tolist() == [7, 0, 0, 1, 4, 2, 1, 4]                 # the match: component 1 on component 1
    assert rows[5].tolist() == [3, 3, 3, 5] and cols[4].tolist() == [1, 2, 1, 1]
    # caps 0: the confusion matrix of foreground against foreground, no components
    table, rows, cols, summary = M.everything(a, b, 0, 0)
    assert table.tolist() == [[1, 0], [0, 7]] and summary.tolist() == [7, 0, 0, 1, 0, 0, 0, 7]
    assert rows.tolist() == [[1, 0, 0, 0], [7, 0, 0, 0]] and cols.tolist() == rows.tolist()
    table, _, _, summary = M.everything(np.array([[0, 0, 2, 5]], np.int32), np.array([[0, 7, 0, 1]], np.int32), 0, 0)
    assert table.tolist() == [[1, 1], [1, 1]] and summary.tolist() == [1, 1, 1, 1, 0, 0, 0, 3]


def test_split_and_merged_paragraphs():
    """what the pixel numbers hide: a paragraph predicted as two, and two paragraphs joined by a bridge one pixel wide"""
    page = np.zeros((40, 60), np.int32)
    page[5:35, 10:50] = 1
    halves = np.zeros_like(page)
    halves[5:19, 10:50], halves[21:35, 10:50] = 1, 2                    # two rows of the paragraph are missing between
    _, rows, _, summary = M.everything(page, halves, 8, 8)
    assert summary[4:7].tolist()[:2] == [1, 2] and summary[6] <= 1
    assert summary[6] == 0 and rows[1].tolist() == [1200, 1, 560, 560]  # neither half reaches half of the union
    f1 = M.pixel_numbers(*summary[:4])[3]
    assert f1 > 0.9

    truth = np.zeros((40, 60), np.int32)
    truth[4:18, 8:52], truth[22:36, 8:52] = 1, 2
    joined = (truth > 0).astype(np.int32)
    joined[18:22, 30] = 1                                               # the bridge: one component now
    _, rows, cols, summary = M.everything(truth, joined, 8, 8)
    assert summary[4:7].tolist() == [2, 1, 0]
    assert rows[1].tolist() == [616, 1, 616, 1236] and rows[2].tolist() == [616, 1, 616, 1236]
    assert summary[:4].tolist() == [1232, 4, 0, 2400 - 1236]
    accuracy, precision, recall, f1 = M.pixel_numbers(*summary[:4])
    assert f1 > 0.9 and recall == 1.0
    # and the page read well: everything found
    _, _, _, summary = M.everything(truth, np.roll(truth, 1, axis=1), 8, 8)
    assert summary[4:7].tolist() == [2, 2, 2]


# ---- bindings --------------------------------------------------------------------------------------------------------------
def test_library_exports_the_new_entry_points():
    from univer_ocr_amd.hip import lib as hiplib
    assert set(NEW_SYMBOLS) <= set(hiplib.ABI_SYMBOLS)
    for name, arguments in NEW_SYMBOLS.items():
        assert len(hiplib._PROTOS[name]) == arguments, name
    header = open(os.path.join(ROOT, 'include', 'univer_hip.h')).read()
    assert all(f'int {name}(' in header for name in NEW_SYMBOLS)
    assert not [name for name in hiplib.ABI_SYMBOLS if name.startswith('uocr_ctx_last_') and 'overlap' in name]
    assert os.path.exists(hiplib.lib_path()), 'run ./build.sh (or __graft_entry__.build()) first'
    lib = hiplib.get_lib()
    assert lib.uocr_abi_version() == 4
    for name in NEW_SYMBOLS:
        getattr(lib, name)
    # a null context is an argument error before anything else is looked at
    assert lib.uocr_label_overlap(None, 1, None, None, None, None, 0, 0, None, None, None, None) == -1
    assert lib.uocr_label_overlap(None, 0, None, None, None, None, 0, 0, None, None, None, None) == -1
    # the limits need no context; a null pointer is refused before anything is written
    outs = [C.c_int(-1) for _ in range(4)]
    assert lib.uocr_label_overlap_limits(*[C.byref(out) for out in outs]) == 0
    pixels_per_block, lds_cells, entries_per_launch, max_cap = [out.value for out in outs]
    assert pixels_per_block > 0 and entries_per_launch > 0 and max_cap > 0 and lds_cells >= 16
    assert (64 + 2) ** 2 <= lds_cells, 'the default caps of ops.mask_score count in LDS'
    for null in range(4):
        outs = [C.c_int(-1) for _ in range(4)]
        args = [None if k == null else C.byref(out) for k, out in enumerate(outs)]
        assert lib.uocr_label_overlap_limits(*args) == -1, f'null pointer {null} was accepted'
        assert all(out.value == -1 for out in outs), f'wrote before refusing null pointer {null}'


# ---- adding up ---------------------------------------------------------------------------------------------------------------
def score_of(a, b, cap):
    from univer_ocr_amd.nn.ops import mask_score_of
    _, rows, _, summary = M.everything(a, b, cap, cap)
    return mask_score_of(summary, rows)


def test_mask_score_of_one_entry():
    truth = np.zeros((20, 30), np.int32)
    truth[2:8, 2:28], truth[12:18, 2:28] = 1, 2
    score = score_of(truth, np.roll(truth, 2, axis=1), 4)
    assert score[:8] == (288, 24, 24, 264, 2, 2, 2, 0)
    assert score.rows == ((156, 1, 144, 156), (156, 2, 144, 156))
    assert score.mean_matched_iou == 144 / 168 and score.iou == 288 / 336
    assert (score.precision, score.recall, score.f1, score.accuracy) == M.pixel_numbers(288, 24, 24, 264)[1:] + (552 / 600,)
    empty = score_of(np.zeros((4, 4), np.int32), np.zeros((4, 4), np.int32), 4)
    assert empty[:8] == (0, 0, 0, 16, 0, 0, 0, 0) and empty.rows == ()
    assert (empty.precision, empty.recall, empty.f1, empty.iou, empty.mean_matched_iou) == (None,) * 5 and empty.accuracy == 1.0


def test_evaluate_masks_takes_its_ratios_from_the_sums():
    """two pages of very different sizes through a stub system that files fixed scores: the report holds the summed ints,
    and ratios of the sums, which the mean of the pages' ratios is far from"""
    from univer_ocr_amd.my_model.evaluate import MaskReport, evaluate_masks
    small_truth = np.zeros((8, 8), np.int32)
    small_truth[1:3, 1:7] = 1
    small = score_of(small_truth, np.zeros_like(small_truth), 4)         # nothing found on the small page
    big_truth = np.zeros((60, 80), np.int32)
    big_truth[5:25, 5:75], big_truth[35:55, 5:75] = 1, 2
    big = score_of(big_truth, np.roll(big_truth, 1, axis=0), 4)          # everything found on the large one
    filed = [{'monochrome': [small], 'paragraph': [small], 'line': [small, big]},
             {'monochrome': [big], 'paragraph': [big], 'line': [big, big]}]

    class Stub:
        get = None                                                       # (as a dataset: the context maker below ignores it)

        def predict(self, context):
            context['mask_scores'] = filed[context['index']]

    contexts = []
    reports = evaluate_masks(Stub(), 2, model_system=Stub(), contexts=contexts,
                             make_context=lambda get, args: {'index': args[0]})
    assert [context['index'] for context in contexts] == [0, 1]
    assert sorted(reports) == ['line', 'monochrome', 'paragraph'] and [len(reports[net]) for net in sorted(reports)] == [2, 1, 1]
    report = reports['paragraph'][0]
    assert isinstance(report, MaskReport) and report.pages == 2
    ints = [small[k] + big[k] for k in range(8)]
    assert list(report[1:9]) == ints
    tp, fp, fn, tn, expected, predicted, matched = ints[:7]
    assert (expected, predicted, matched) == (3, 2, 2)
    assert report.recall == tp / (tp + fn) and report.precision == tp / (tp + fp) and report.iou == tp / (tp + fp + fn)
    assert report.f1 == M.pixel_numbers(tp, fp, fn, tn)[3] and report.accuracy == (tp + tn) / (tp + fp + fn + tn)
    assert report.found == 2 / 3 and report.spurious == 0.0
    assert report.mean_matched_iou == big.mean_matched_iou
    assert abs(report.recall - (0.0 + big.recall) / 2) > 0.4, 'the mean of the ratios is another number'
    assert reports['line'][1].tp == 2 * big.tp and reports['line'][1].found == 1.0 and reports['line'][0] == report
    nothing = evaluate_masks(Stub(), 1, model_system=Stub(), make_context=lambda get, args: {'index': 0})['monochrome'][0]
    assert nothing.precision is None and nothing.spurious is None and nothing.found == 0.0 and nothing.recall == 0.0
