"""Host side of the labelling / crop feature: the fixture tests/golden/paragraph_crop.npz (made from the reference by
tests/golden/make_golden_crops.py), the NumPy flood fill the GPU tests use as expected value at sizes the fixture cannot
know (trusted only because it is pinned to the fixture here), the nested selectors, the ABI names and the modes that
still raise.  Nothing here needs a GPU."""
import os

import numpy as np
import pytest

from conftest import ROOT, load_golden

RULES = ('mean', 'mean_max', 'value')


def threshold_of(x, rule, value=None):
    """the three rules of uocr_label_components, in float64 (interpreter.py:17, :437-438 / :549)"""
    x = np.asarray(x, np.float64)
    if rule == 'mean':
        return float(np.mean(x))
    if rule == 'mean_max':
        return 0.5 * (float(np.mean(x)) + float(np.max(x)))
    return float(value)


def flood_fill(mask):
    """Labels (int32 H x W) and table (int64 count x 8: first pixel, area, y0, y1, x0, x1, sum y, sum x) of a boolean
    H x W mask: 4-connectivity, components numbered in the order of their first pixel in row-major order."""
    mask = np.asarray(mask, bool)
    h, w = mask.shape
    labels = np.zeros((h, w), np.int32)
    rows = []
    for start in np.flatnonzero(mask):
        y, x = divmod(int(start), w)
        if labels[y, x]:
            continue
        k = len(rows) + 1
        labels[y, x] = k
        stack, ys, xs = [(y, x)], [], []
        while stack:
            y, x = stack.pop()
            ys.append(y)
            xs.append(x)
            for ny, nx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                if 0 <= ny < h and 0 <= nx < w and mask[ny, nx] and not labels[ny, nx]:
                    labels[ny, nx] = k
                    stack.append((ny, nx))
        rows.append([start, len(ys), min(ys), max(ys) + 1, min(xs), max(xs) + 1, sum(ys), sum(xs)])
    return labels, np.array(rows, np.int64).reshape(len(rows), 8)


@pytest.fixture(scope='module')
def g():
    return load_golden('paragraph_crop')


def test_fixture_loads_and_is_consistent(g):
    names = [str(s) for s in g['mask_names']]
    assert len(names) == 10
    for name in names:
        x = g[f'{name}/x']
        assert x.ndim == 4 and x.shape[0] == 1 and x.shape[3] == 1
        assert 40 <= x.shape[1] <= 70 and 70 <= x.shape[2] <= 150
        for rule in RULES:
            t = threshold_of(x, rule, g[f'{name}/value_t'])
            assert np.min(np.abs(x - t)) > 1e-3, f'{name}/{rule}: an input lies within 1e-3 of its threshold'
            assert g[f'{name}/{rule}/labels'].shape == x.shape[1:3]
            assert g[f'{name}/{rule}/labels'].max() == len(g[f'{name}/{rule}/table'])
    for name in (str(s) for s in g['crop_masks']):
        count = len(g[f'{name}/mean/table'])
        for c in (1, 2, 4):
            assert g[f'{name}/img{c}'].shape == (*g[f'{name}/x'].shape[:3], c)
            assert g[f'{name}/img{c}'].min() >= 0
            for k in range(1, count + 1):
                _, _, y0, y1, x0, x1, _, _ = g[f'{name}/mean/table'][k - 1]
                assert g[f'{name}/crop{c}/{k}'].shape == (1, y1 - y0, x1 - x0, c)
    assert g['cropped_monochrome0'].shape == (1, 80, 192, 1) and g['cropped_line1'].shape == (1, 32, 128, 2)


def test_flood_fill_reproduces_the_reference(g):
    """labels, counts, boxes, areas and coordinate sums of every fixture mask and rule, exactly; centres from the sums"""
    for name in (str(s) for s in g['mask_names']):
        x = g[f'{name}/x'][0, :, :, 0]
        for rule in RULES:
            labels, table = flood_fill(x > threshold_of(x, rule, g[f'{name}/value_t']))
            assert np.array_equal(labels, g[f'{name}/{rule}/labels']), f'{name}/{rule}'
            assert np.array_equal(table, g[f'{name}/{rule}/table']), f'{name}/{rule}'
            centers = table[:, 6:8] / table[:, 1:2]
            assert np.allclose(centers, g[f'{name}/{rule}/centers'], rtol=1e-13, atol=0), f'{name}/{rule}'


def test_fixture_crops_follow_from_labels_and_boxes(g):
    """the stored crops are image * (labels == k) cut to the table's box: what uocr_masked_crop is specified to write"""
    for name in (str(s) for s in g['crop_masks']):
        labels, table = g[f'{name}/mean/labels'], g[f'{name}/mean/table']
        for c in (1, 2, 4):
            image = g[f'{name}/img{c}']
            for k, (_, _, y0, y1, x0, x1, _, _) in enumerate(table, 1):
                expected = (image[0] * (labels == k)[:, :, None])[y0:y1, x0:x1]
                assert np.array_equal(g[f'{name}/crop{c}/{k}'][0], expected)


# ---- selectors -------------------------------------------------------------------------------------------------------
class StubModel:
    """what ModelComponent needs of a model: train / predict record their inputs and publish a tagged output"""
    outputs_count = 1

    def __init__(self):
        self.seen, self.layers_outputs = [], {}

    def train(self, X, y):
        self.seen.append((X, y))
        self.layers_outputs = {0: f'pred({X})'}
        return {'output_losses': [1.0], 'regularization_loss': 0.5}

    def predict(self, X):
        self.seen.append(X)
        self.layers_outputs = {0: f'pred({X})'}
        return [self.layers_outputs[0]]


def test_line_selector_files_predictions_per_paragraph():
    from univer_ocr_amd.my_model.model import LineSelector
    from univer_ocr_amd.nn.model_system import ModelComponent
    model = StubModel()
    component = ModelComponent('Line', model, LineSelector('X', 'y', 'pred'), delist_result=True)
    context = {'X': ['a', 'b', 'c'], 'y': ['A', 'B', 'C'], 'losses': {}}
    component.train(context)
    assert model.seen == [('a', 'A'), ('b', 'B'), ('c', 'C')]
    assert context['pred'] == ['pred(a)', 'pred(b)', 'pred(c)']
    assert context['losses']['Line'] == {'output_losses': [1.0, 1.0, 1.0], 'regularization_loss': 1.5}
    # a new bind starts at paragraph 0 again: the slots are overwritten, not appended to
    context2 = {'X': ['d'], 'y': ['D'], 'losses': {}, 'pred': ['old0', 'old1']}
    component.train(context2)
    assert component.selector.paragraph_id == 0
    assert context2['pred'] == ['pred(d)', 'old1']
    context3 = {'X': ['e', 'f'], 'prediction': {}}
    component.predict(context3)
    assert model.seen[-2:] == ['e', 'f'] and context3['pred'] == ['pred(e)', 'pred(f)']
    empty = {'X': [], 'y': [], 'losses': {}}
    component.train(empty)
    assert empty['losses'] == {} and 'pred' not in empty


def test_char_selector_files_predictions_per_paragraph_and_line():
    from univer_ocr_amd.my_model.model import CharSelector
    from univer_ocr_amd.nn.model_system import ModelComponent
    model = StubModel()
    component = ModelComponent('Char', model, CharSelector('X', 'y', 'pred'), delist_result=True)
    context = {'X': [['a', 'b'], ['c'], ['d', 'e', 'f']], 'y': [['A', 'B'], ['C'], ['D', 'E', 'F']], 'losses': {}}
    component.train(context)
    assert model.seen == [('a', 'A'), ('b', 'B'), ('c', 'C'), ('d', 'D'), ('e', 'E'), ('f', 'F')]
    assert context['pred'] == [['pred(a)', 'pred(b)'], ['pred(c)'], ['pred(d)', 'pred(e)', 'pred(f)']]
    assert len(context['losses']['Char']['output_losses']) == 6
    component.selector({'X': [], 'y': []})
    assert (component.selector.paragraph_id, component.selector.line_id) == (0, 0)
    context2 = {'X': [['g']], 'prediction': {}}
    component.predict(context2)
    assert context2['pred'] == [['pred(g)']]


def test_move_components_walk_nested_structures():
    from univer_ocr_amd.my_model.model import make_move_from_gpu_component, make_move_to_gpu_component
    from univer_ocr_amd.nn import CP
    from univer_ocr_amd.nn.gpu import DeviceArray
    a, b = np.arange(6.0).reshape(1, 2, 3, 1), np.ones((1, 1, 2, 1))
    context = {'host': [[a], {'k': b}]}
    make_move_to_gpu_component([('host', 'dev')]).train(context)
    assert isinstance(context['dev'][0][0], DeviceArray) and isinstance(context['dev'][1]['k'], DeviceArray)
    make_move_from_gpu_component([('dev', 'back')]).predict(context)
    assert np.array_equal(context['back'][0][0], a.astype(CP.dtype)) and np.array_equal(context['back'][1]['k'], b)


# ---- ABI and modes ---------------------------------------------------------------------------------------------------
def test_header_and_binding_agree_on_the_threshold_modes():
    from univer_ocr_amd.hip import lib as hiplib
    header = open(os.path.join(ROOT, 'include', 'univer_hip.h')).read()
    for name in ('UOCR_THRESH_MEAN = 0', 'UOCR_THRESH_MEAN_MAX = 1', 'UOCR_THRESH_VALUE = 2'):
        assert name in header
    assert (hiplib.THRESH_MEAN, hiplib.THRESH_MEAN_MAX, hiplib.THRESH_VALUE) == (0, 1, 2)


def test_modes_that_need_missing_stages_still_raise():
    from univer_ocr_amd.my_model.model import Modes, make_context_maker, make_model_system
    for mode, stage in ((Modes.TRAIN_CHAR, 'LineCrop'), (Modes.TRAIN_ALL, 'LineCrop'), (Modes.PREDICT, 'PredToText')):
        with pytest.raises(NotImplementedError, match=stage):
            make_model_system((1, 32, 32, 1), mode=mode)
    for mode in (Modes.TRAIN_CHAR, Modes.TRAIN_ALL):
        with pytest.raises(NotImplementedError, match='LineCrop'):
            make_context_maker(mode)


def test_train_line_system_is_built_without_a_gpu():
    from univer_ocr_amd.my_model.model import LineSelector, Modes, make_context_maker, make_model_system
    from univer_ocr_amd.nn.model_system import ModelComponent, RawFunctionComponent
    from univer_ocr_amd.nn.progress_tracker import ProgressTracker
    tracker = ProgressTracker(handler=lambda *a: None)
    system, models, names = make_model_system((1, 32, 48, 1), progress_tracker=tracker, mode=Modes.TRAIN_LINE)
    assert names == ['ParagraphCrop', 'Line'] and list(models) == ['Line']
    crop, line = system.components
    assert isinstance(crop, RawFunctionComponent) and isinstance(line, ModelComponent)
    assert isinstance(line.selector, LineSelector) and line.model is models['Line']
    assert 'ParagraphCrop' in tracker.layers
    make_context = make_context_maker(Modes.TRAIN_LINE)
    layers = {'monochrome': np.zeros((1, 4, 4, 1)), 'paragraph': np.zeros((1, 4, 4, 1)), 'line': np.zeros((1, 4, 4, 2))}
    context = make_context(lambda layer_tags: {tag: layers[tag] for tag in layer_tags})
    assert sorted(context) == ['line', 'monochrome_pred', 'paragraph_pred'] and context['line'].shape == (1, 4, 4, 2)


def test_crop_paragraphs_refuses_what_it_cannot_do():
    from univer_ocr_amd.my_model.crop import CropParagraphs
    from univer_ocr_amd.nn import CP
    with pytest.raises(NotImplementedError, match='rotation search'):
        CropParagraphs(find_rotation=True)
    crop = CropParagraphs()
    with pytest.raises(ValueError):
        crop(CP.zeros((2, 8, 8, 1)), [CP.zeros((2, 8, 8, 1))])
    with pytest.raises(ValueError):
        crop(CP.zeros((1, 8, 8, 1)), [CP.zeros((1, 8, 9, 1))])
