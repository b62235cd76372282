"""Host side of the batched labelling (csrc/label_batch.hip, nn/ops.py: label_batch, my_model/crop.py:
CropLines(labelling='page')): the ABI names, the argument checks that come before any call, the one call per page and
its entry order, the nesting against the per-paragraph form on stubbed tables, the two-pass capacity rule on a stubbed
runtime that writes counts and rows where the library would, the flood fill of tests/test_label_host.py against scipy
on strided channel views (what the GPU tests use as expected value), and the keyword's way through the systems.
Nothing here needs a GPU."""
import ctypes as C

import numpy as np
import pytest

from test_label_host import flood_fill

NEW_SYMBOLS = ('uocr_label_batch', 'uocr_ctx_last_label_batch')


# ---- ABI ---------------------------------------------------------------------------------------------------------------
def test_library_exports_the_new_entry_points():
    from univer_ocr_amd.hip import lib as hiplib
    lib = hiplib.get_lib()
    assert lib.uocr_abi_version() == 4
    for name in NEW_SYMBOLS:
        assert getattr(lib, name)
    # without a context both refuse with UOCR_ERR_ARG before touching anything
    assert lib.uocr_label_batch(None, 0, 0, None, None, None, None, None, 0, 0.0, None, None, 0, None) == -1
    assert lib.uocr_ctx_last_label_batch(None, None, None, None, None) == -1


# ---- ops.label_batch: checks before any call ---------------------------------------------------------------------------
class NoRuntime:
    def call(self, name, *args):
        raise AssertionError(f'{name} was called')


def test_label_batch_of_nothing_and_of_wrong_entries(monkeypatch):
    """an empty list needs no device; ranks, channels, thresholds and dtypes are checked before any call"""
    from univer_ocr_amd.nn import CP, ops
    monkeypatch.setattr(ops, '_rt', lambda: NoRuntime())
    assert ops.label_batch([]) == [] and ops.label_batch([], 'mean_max', labels=True) == []
    good = CP.zeros((1, 10, 12, 2), np.float32)
    for bad in (CP.zeros((10, 12, 2), np.float32), CP.zeros((2, 10, 12, 2), np.float32), np.zeros((1, 10, 12, 2))):
        with pytest.raises(ValueError, match='label_batch: expected'):
            ops.label_batch([(good, 0), (bad, 0)])
    for channel in (-1, 2):
        with pytest.raises(ValueError, match='label_batch: channel'):
            ops.label_batch([(good, 1), (good, channel)])
    with pytest.raises(ValueError, match='threshold'):
        ops.label_batch([(good, 0)], 'max')
    with pytest.raises(ValueError, match='max_components'):
        ops.label_batch([(good, 0)], max_components=-1)
    with pytest.raises(ValueError, match='share a dtype'):
        ops.label_batch([(good, 0), (CP.zeros((1, 10, 12, 1), np.float64), 0)])


# ---- the two-pass capacity rule on a stubbed runtime ---------------------------------------------------------------------
class TableRuntime:
    """uocr_label_batch as the header specifies its outputs, from a table per input pointer: count[i] is the true count,
    the first min(count, max_components) rows are written, the rows after them are zero"""

    def __init__(self, truth):
        self.truth, self.calls = truth, []

    def call(self, name, code, n, x, h, w, c, channel, mode, value, labels, table, max_components, count):
        assert name == 'uocr_label_batch'
        self.calls.append(dict(n=n, x=list(x), h=list(h), w=list(w), c=list(c), channel=list(channel), mode=mode,
                               labels=labels, cap=max_components))
        counts = np.ctypeslib.as_array((C.c_int32 * n).from_address(count.value))
        assert table.value % 8 == 0
        rows = np.ctypeslib.as_array((C.c_int64 * (n * max_components * 8)).from_address(table.value)).reshape(n, max_components, 8)
        rows[:] = 0
        for i in range(n):
            full = self.truth[(x[i], channel[i])]
            counts[i] = len(full)
            rows[i, :min(len(full), max_components)] = full[:max_components]


def numbered_table(count, seed):
    rng = np.random.default_rng(seed)
    table = rng.integers(1, 1000, (count, 8)).astype(np.int64)
    table[:, 0] = np.arange(count)
    return table


def stubbed(monkeypatch, counts):
    from univer_ocr_amd.nn import CP, ops
    arrays = [CP.zeros((1, 5 + i, 7, 2), np.float32) for i in range(len(counts))]
    truth = {(a.ptr, 1): numbered_table(count, i) for i, (a, count) in enumerate(zip(arrays, counts))}
    runtime = TableRuntime(truth)
    monkeypatch.setattr(ops, '_rt', lambda: runtime)
    return ops, runtime, [(a, 1) for a in arrays], [truth[(a.ptr, 1)] for a in arrays]


def check_results(results, tables):
    assert len(results) == len(tables)
    for got, table in zip(results, tables):
        assert isinstance(got.count, int) and got.count == len(table)
        assert got.table.dtype == np.int64 and np.array_equal(got.table, table)
        assert np.array_equal(got.boxes, table[:, 2:6]) and np.array_equal(got.area, table[:, 1])
        assert np.array_equal(got.center_of_mass, table[:, 6:8] / np.maximum(table[:, 1:2], 1))
        assert got.labels is None


def test_counts_within_the_cap_take_one_call(monkeypatch):
    from univer_ocr_amd.hip import lib as hiplib
    ops, runtime, entries, tables = stubbed(monkeypatch, [0, 3, 8, 1])
    check_results(ops.label_batch(entries, 'mean_max', max_components=100, cap=8), tables)
    assert len(runtime.calls) == 1
    call = runtime.calls[0]
    assert call['n'] == 4 and call['cap'] == 8 and call['mode'] == hiplib.THRESH_MEAN_MAX and call['labels'] is None
    assert call['h'] == [5, 6, 7, 8] and call['w'] == [7] * 4 and call['c'] == [2] * 4 and call['channel'] == [1] * 4
    assert call['x'] == [a.ptr for a, _ in entries]


def test_counts_above_the_cap_take_exactly_two_calls(monkeypatch):
    ops, runtime, entries, tables = stubbed(monkeypatch, [2, 9, 8, 30, 100])
    check_results(ops.label_batch(entries, 0.5, max_components=100, cap=8), tables)
    assert len(runtime.calls) == 2, 'one second call for all longer entries together, never a third'
    first, second = runtime.calls
    assert first['n'] == 5 and first['cap'] == 8
    assert second['n'] == 3 and second['cap'] == 100 and second['x'] == [entries[i][0].ptr for i in (1, 3, 4)]
    # the cap never exceeds max_components
    ops, runtime, entries, tables = stubbed(monkeypatch, [2, 5])
    check_results(ops.label_batch(entries, max_components=5, cap=256), tables)
    assert len(runtime.calls) == 1 and runtime.calls[0]['cap'] == 5


def test_counts_above_max_components_raise(monkeypatch):
    from univer_ocr_amd.hip import HipError
    ops, runtime, entries, _ = stubbed(monkeypatch, [2, 101, 9])
    with pytest.raises(HipError, match='101 components, more than max_components = 100'):
        ops.label_batch(entries, max_components=100, cap=8)
    assert len(runtime.calls) == 1


# ---- CropLines(labelling='page') ---------------------------------------------------------------------------------------
def table_of(centres_and_boxes):
    """component rows with area 1: the centre is the coordinate sum"""
    return np.array([[0, 1, y0, y1, x0, x1, cy, cx] for (cy, cx), (y0, y1, x0, x1) in centres_and_boxes], np.int64).reshape(-1, 8)


# per paragraph (top rows, bottom rows): upright with two lines given out of order, no top at all, turned by 90 degrees
PAGE_TABLES = [
    (table_of([((20, 8), (18, 22, 2, 14)), ((4, 8), (3, 6, 1, 15))]), table_of([((25, 8), (24, 27, 3, 13)), ((9, 8), (8, 11, 2, 14))])),
    (table_of([]), table_of([((9, 8), (8, 11, 2, 14))])),
    (table_of([((6, 9), (1, 11, 8, 10))]), table_of([((6, 3), (2, 10, 2, 4))])),
]


def forbidden(name):
    def stub(*args, **kwargs):
        raise AssertionError(f'ops.{name} was called')
    return stub


def patch_page_form(monkeypatch, crop, masks, calls):
    from univer_ocr_amd.nn import ops

    def label_batch(entries, threshold, max_components):
        entries = list(entries)
        calls.append((entries, threshold, max_components))
        index = {id(m): p for p, m in enumerate(masks)}
        return [ops.EntryComponents(len(PAGE_TABLES[index[id(m)]][ch]), PAGE_TABLES[index[id(m)]][ch]) for m, ch in entries]
    monkeypatch.setattr(crop.ops, 'label_batch', label_batch)
    monkeypatch.setattr(crop.ops, 'split', forbidden('split'))
    monkeypatch.setattr(crop.ops, 'label_components', forbidden('label_components'))


def patch_paragraph_form(monkeypatch, crop, masks):
    class Stub:
        def __init__(self, table):
            self.center_of_mass, self.boxes = [table[:, 6:8] / np.maximum(table[:, 1:2], 1)], [table[:, 2:6]]
    index = {id(m): p for p, m in enumerate(masks)}
    monkeypatch.setattr(crop.ops, 'label_batch', forbidden('label_batch'))
    monkeypatch.setattr(crop.ops, 'split', lambda mask, shapes: [PAGE_TABLES[index[id(mask)]][0], PAGE_TABLES[index[id(mask)]][1]])
    monkeypatch.setattr(crop.ops, 'label_components', lambda table, threshold, max_components: Stub(table))


def test_page_form_makes_one_label_batch_call_per_page(monkeypatch):
    from univer_ocr_amd.my_model import crop
    from univer_ocr_amd.nn import CP
    masks = [CP.zeros((1, 30 + p, 16, 2), np.float32) for p in range(3)]
    calls = []
    patch_page_form(monkeypatch, crop, masks, calls)
    found = crop.CropLines(max_components=77, labelling='page').find_lines(masks)
    assert len(calls) == 1
    entries, threshold, max_components = calls[0]
    assert [(id(m), ch) for m, ch in entries] == [(id(m), ch) for m in masks for ch in (0, 1)], 'entries (p, 0), (p, 1) in order'
    assert threshold == 'mean_max' and max_components == 77
    assert found == [(None, [(3, 1, 8, 14), (18, 2, 9, 12)]), (None, []), (90, [(1, 2, 10, 8)])]


def test_default_form_makes_no_label_batch_call_and_both_forms_nest_alike(monkeypatch):
    from univer_ocr_amd.my_model import crop
    from univer_ocr_amd.nn import CP
    masks = [CP.zeros((1, 30 + p, 16, 2), np.float32) for p in range(3)]
    arrays = [[CP.zeros((1, 30 + p, 16, c), np.float32) for p in range(3)] for c in (1, 9)]
    line_crops = []

    def line_crop(entries, zoomed_height, minimal_width):
        line_crops.append([(id(e[0]), *e[1:]) for e in entries])
        return [f'crop{i}' for i, _ in enumerate(entries)]
    monkeypatch.setattr(crop.ops, 'line_crop', line_crop)
    assert crop.CropLines().labelling == 'paragraph'
    patch_paragraph_form(monkeypatch, crop, masks)
    by_paragraph = crop.CropLines()
    found = by_paragraph.find_lines(masks)
    result = by_paragraph(masks, arrays)
    calls = []
    patch_page_form(monkeypatch, crop, masks, calls)
    by_page = crop.CropLines(labelling='page')
    assert by_page.find_lines(masks) == found and found[1] == (None, []) and [len(b) for _, b in found] == [2, 0, 1]
    assert by_page(masks, arrays) == result == [[['crop0', 'crop1'], [], ['crop2']], [['crop3', 'crop4'], [], ['crop5']]]
    assert line_crops[0] == line_crops[1] and len(calls) == 2
    # a page without paragraphs: no entries, no lines
    assert by_page([], [[], []]) == [[], []] and calls[2][0] == []


def test_unknown_labelling_raises():
    from univer_ocr_amd.my_model.crop import CropLines
    from univer_ocr_amd.my_model.model import make_line_crop_component, make_predict_system, make_train_char_system
    for build in (lambda: CropLines(labelling='line'), lambda: CropLines(labelling=None),
                  lambda: make_line_crop_component(line_labelling='both'),
                  lambda: make_train_char_system((1, 32, 24, 1), line_labelling='both'),
                  lambda: make_predict_system((1, 32, 48, 1), line_labelling='both')):
        with pytest.raises(ValueError, match="'paragraph' or 'page'"):
            build()


def test_keyword_reaches_the_stage():
    from univer_ocr_amd.my_model import predict
    from univer_ocr_amd.my_model.crop import CropLines
    from univer_ocr_amd.my_model.model import make_line_crop_component, make_predict_system, make_train_char_system
    for kw, expected in (({}, 'paragraph'), ({'line_labelling': 'paragraph'}, 'paragraph'), ({'line_labelling': 'page'}, 'page')):
        stage = make_line_crop_component(**kw).stage
        assert isinstance(stage, CropLines) and stage.labelling == expected
        system, _, names = make_train_char_system((1, 32, 24, 1), **kw)
        assert system.components[names.index('LineCrop')].stage.labelling == expected
        system, _, names = make_predict_system((1, 32, 48, 1), **kw)
        assert system.components[names.index('LineCrop')].stage.labelling == expected
        assert predict.load_model_system((1, 32, 48, 1), **kw).components[names.index('LineCrop')].stage.labelling == expected


def test_predict_text_and_main_pass_the_keyword_on(monkeypatch, tmp_path):
    from univer_ocr_amd.my_model import predict
    from univer_ocr_amd.nn import CP
    seen = []

    class System:
        def predict(self, context):
            context['text'] = [['line']]

    def load(shape, weights_path, find_rotation, rotation_search, line_labelling):
        seen.append(line_labelling)
        return System()
    monkeypatch.setattr(predict, 'load_model_system', load)
    monkeypatch.setattr(CP, 'use_gpu', staticmethod(lambda device_index=None: None))
    page = np.zeros((1, 16, 16, 1))
    assert predict.predict_text(page) == [['line']] and predict.predict_text(page, line_labelling='page') == [['line']]
    np.save(tmp_path / 'page.npy', page[0, :, :, 0])
    predict.main([str(tmp_path / 'page.npy')])
    predict.main([str(tmp_path / 'page.npy'), '--page-line-labels'])
    assert seen == ['paragraph', 'page', 'paragraph', 'page']


# ---- the expected value of the GPU tests ---------------------------------------------------------------------------------
def test_flood_fill_equals_scipy_on_strided_channel_views():
    """labels, slices and coordinate sums of 50 random masks of up to 9 x 70, each read as a channel of a (1, H, W, 3) array"""
    from scipy import ndimage
    rng = np.random.default_rng(2024)
    for case in range(50):
        h, w, channel = int(rng.integers(1, 10)), int(rng.integers(1, 71)), int(rng.integers(0, 3))
        x = (rng.random((1, h, w, 3)) < rng.uniform(0.2, 0.8))
        view = x[0, :, :, channel]
        assert view.strides[1] == 3 * x.itemsize or w == 1
        labels, table = flood_fill(view)
        exp_labels, count = ndimage.label(view)
        assert len(table) == count and np.array_equal(labels, exp_labels), f'case {case}'
        for k, (ys, xs) in enumerate(ndimage.find_objects(exp_labels), 1):
            first, area, y0, y1, x0, x1, sy, sx = table[k - 1]
            assert (y0, y1, x0, x1) == (ys.start, ys.stop, xs.start, xs.stop), f'case {case} component {k}'
            yy, xx = np.nonzero(exp_labels == k)
            assert (area, sy, sx) == (len(yy), yy.sum(), xx.sum()) and first == yy[0] * w + xx[0]
            cy, cx = ndimage.center_of_mass(view, exp_labels, k)
            assert np.isclose(sy / area, cy, rtol=1e-13, atol=0) and np.isclose(sx / area, cx, rtol=1e-13, atol=0)
