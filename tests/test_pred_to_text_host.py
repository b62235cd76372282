"""Host side of the PredToText feature: the fixture tests/golden/pred_to_text.npz (made from the reference's
PredToText._func1 by tests/golden/make_golden_pred_to_text.py), the character and pair tables, the NumPy restatement of
the stage's rules that the GPU tests use as expected value at sizes the fixture cannot know (trusted only because it is
pinned to the fixture here), the adjacency form of the walk that the kernels evaluate, the nesting of PredToText, the
PREDICT system's assembly and the ABI names.  Nothing here needs a GPU."""

import numpy as np
import pytest

from conftest import load_golden

N_CHARS = 162
NEW_SYMBOLS = ('uocr_pred_to_text', 'uocr_ctx_last_pred_to_text')
PAGE = ((0, 0), (0, 1), (1, 0))
PREDICT_NAMES = ['Monochrome', 'Paragraph', 'ParagraphCrop', 'Line', 'LineCrop', 'Char', 'PredToText']


@pytest.fixture(scope='module')
def g():
    return load_golden('pred_to_text')


def line_names(g):
    return [str(s) for s in g['line_names']]


def test_fixture_loads_and_is_consistent(g):
    names = line_names(g)
    assert names == ['hand', 'w1', 'w8', 'w17', 'w64', 'w130', 'w300', 'ties', 'zeros']
    chars = ''.join(g['chars'].tolist())
    assert len(chars) == N_CHARS and g['pairs'].shape == (18, 2) and g['cls'].shape == (N_CHARS,)
    for name in names:
        x, text, ids = g[f'{name}/x'], str(g[f'{name}/text']), g[f'{name}/ids']
        assert x.ndim == 2 and x.shape[1] == N_CHARS and ids.dtype == np.int32 and x.dtype == np.float64
        assert name[0] != 'w' or x.shape[0] == int(name[1:])
        assert np.array_equal(x, x.astype(np.float16).astype(np.float64), equal_nan=True), f'{name}: not exact in binary16'
        finite = x[~np.isnan(x)]
        assert np.array_equal(finite * 64, np.round(finite * 64)), f'{name}: not multiples of 1/64'
        assert ''.join(chars[i] for i in ids) == text, name
    assert len(g['ties/ids']) > g['ties/x'].shape[0], 'ties: more ids than rows, so that a second call is needed'
    zeros = g['zeros/x']
    assert str(g['zeros/text']) == '' and (np.max(zeros, axis=1) == 0).all()
    assert any(np.signbit(row[row == 0]).all() for row in zeros), 'a row whose maximum is -0.0 and nothing else'
    for name in ('w8', 'w17', 'w64', 'w130', 'w300'):
        x = g[f'{name}/x']
        assert (np.sum(x == x.max(axis=1, keepdims=True), axis=1) == 1).all(), f'{name}: one maximum per row'
    for p, l in PAGE:
        w = (24, 40, 17)[PAGE.index((p, l))]
        assert g[f'system/mono{p}_{l}'].shape == (1, 32, w, 1) and g[f'system/char_pred{p}_{l}'].shape == (w, N_CHARS)
        pred = g[f'system/char_pred{p}_{l}']
        top = np.sort(pred, axis=1)[:, -2:]
        assert np.min(top[:, 1] - top[:, 0]) > 1e-3 * np.abs(pred).max(), 'a maximum a float32 net could miss'


def test_hand_built_line_holds_every_behaviour(g):
    """row by row: what the line was built to show, read off the fixture's input and the reference's output"""
    x, ids, cls = g['hand/x'], g['hand/ids'].tolist(), g['cls']
    a, b, cyr_a, cyr_e, e, cyr_o, o, cyr_p, p, cyr_u, y, one = 78, 79, 2, 7, 82, 17, 92, 19, 93, 22, 102, 69
    with np.errstate(invalid='ignore'):
        maxima = np.max(x, axis=1)
    candidates = [np.flatnonzero(row == m).tolist() if m != 0 else [] for row, m in zip(x, maxima)]
    assert candidates[:14] == [[a], [a], [b], [b], [cyr_a], [a], [0], [a], [cyr_a], [0], [cyr_e], [0], [e], [cyr_o]]
    assert not x[14].any() and candidates[15:18] == [[o], [0], [cyr_p]]
    assert np.isnan(x[18]).any() and np.isnan(maxima[18]) and candidates[18] == [] and candidates[19] == [p]
    assert maxima[20] == 0 and np.signbit(maxima[20]) and (x[20] <= 0).all()
    assert maxima[21] == -0.5 and candidates[21] == [one]
    assert candidates[22] == [cyr_u, y] and cls[cyr_u] == cls[y] >= 0
    assert candidates[23] == [0, b] and candidates[24] == list(range(N_CHARS)) and x[24, 0] != 0
    # a a -> a | b b -> b b | cyr-a a -> cyr-a | tab | a cyr-a -> a | tab | cyr-e tab e -> both | cyr-o, zeros, o -> cyr-o
    # | tab | cyr-p, NaN, p -> cyr-p | -0.0: nothing | -0.5 emits | the tied pair -> its first | tab, b -> b | all 162
    assert ids[:12] == [a, b, b, cyr_a, a, cyr_e, e, cyr_o, cyr_p, one, cyr_u, b]
    assert ids[12:] == list(range(1, N_CHARS)), 'all equal: the tab emits nothing, no two neighbours share a pair'


def test_tables_equal_the_fixture(g):
    from univer_ocr_amd.my_model import crop
    from univer_ocr_amd.my_model.model import N_CHARS as model_n_chars
    assert crop.CHARS == ''.join(g['chars'].tolist()) and len(crop.CHARS) == model_n_chars == N_CHARS
    assert np.array_equal(np.array(crop.SIMILAR_PAIRS, np.int32), g['pairs'])
    stage = crop.PredToText()
    assert stage.cls.dtype == np.int32 and np.array_equal(stage.cls, g['cls']) and stage.chars == crop.CHARS
    assert np.sum(g['cls'] >= 0) == 36 and np.sum(g['cls'] < 0) == 126 and g['cls'][0] == -1
    for k, (first, second) in enumerate(g['pairs']):
        assert g['cls'][first] == g['cls'][second] == k


def test_rules_reproduce_the_reference(g):
    """the restatement equals PredToText._func1 on every fixture line: ids and text"""
    from univer_ocr_amd.my_model.crop import CHARS, pred_to_text_rules
    lines = [(name, g[f'{name}/x'], g[f'{name}/ids'], g[f'{name}/text']) for name in line_names(g)]
    lines += [(f'system {p}.{l}', g[f'system/char_pred{p}_{l}'], g[f'system/ids{p}_{l}'], g[f'system/text{p}_{l}']) for p, l in PAGE]
    for name, x, ref_ids, ref_text in lines:
        ids = pred_to_text_rules(x)
        assert ids == ref_ids.tolist(), f'{name}: ids'
        assert ''.join(CHARS[i] for i in ids) == str(ref_text), f'{name}: text'
        for dtype in (np.float32, np.float16):
            if name.startswith('system'):
                continue                                          # (only the ops lines are exact in the narrow types)
            assert pred_to_text_rules(x.astype(dtype)) == ids, f'{name}: {dtype.__name__}'


def sequential_walk(ids, cls):
    """interpreter.py:603-613 on ids, are_similar(a, b) spelled through the pair table"""
    out, prev = [], None
    for cur in ids:
        if cur == 0:
            prev = None
            continue
        if prev is not None and cls[prev] >= 0 and cls[cur] == cls[prev]:
            continue
        out.append(cur)
        prev = cur
    return out


def test_adjacent_rule_equals_the_sequential_walk(g):
    """20 000 random id sequences weighted towards paired ids and tabs, under the 18 pairs and under random tables (classes
    of any size, the tab inside a class): two adjacent candidates decide every emission"""
    from univer_ocr_amd.my_model.crop import adjacent_rule
    rng = np.random.default_rng(40)
    cls = g['cls']
    paired = np.flatnonzero(cls >= 0)
    checked = 0
    for trial in range(20000):
        if trial % 4 == 3:
            n = int(rng.integers(1, 40))
            table = np.where(rng.random(n) < 0.3, -1, rng.integers(0, max(1, n // 3), n)).astype(np.int32)
            ids = rng.integers(0, n, int(rng.integers(0, 30))).tolist()
        else:
            table, length = cls, int(rng.integers(0, 30))
            kind = rng.random(length)
            ids = np.where(kind < 0.15, 0, np.where(kind < 0.8, rng.choice(paired[:8], length), rng.integers(0, N_CHARS, length))).tolist()
        assert adjacent_rule(ids, table) == sequential_walk(ids, table), (ids, table.tolist())
        checked += len(ids) > 1
    assert checked > 15000


def test_rules_with_another_table():
    from univer_ocr_amd.my_model.crop import pred_to_text_rules
    x = np.eye(4)[[1, 2, 3, 3, 0, 3, 1]]
    assert pred_to_text_rules(x, cls=[-1, 0, 0, -1]) == [1, 3, 3, 3, 1]
    assert pred_to_text_rules(x, cls=[-1, -1, -1, 5]) == [1, 2, 3, 3, 1]
    assert pred_to_text_rules(np.zeros((3, 4)), cls=[-1] * 4) == []


# ---- PredToText and the component ------------------------------------------------------------------------------------
def test_pred_to_text_keeps_the_nesting_with_one_call_per_page(monkeypatch):
    from univer_ocr_amd.my_model import crop
    calls = []

    def stub(lines, cls):
        calls.append((list(lines), cls))
        return [[78 + i, 79] for i, _ in enumerate(lines)]
    monkeypatch.setattr(crop.ops, 'pred_to_text', stub)
    monkeypatch.setattr(crop.ops, 'as_device', lambda a: a)
    stage = crop.PredToText()
    assert stage([['p', 'q'], [], ['r']]) == [['ab', 'bb'], [], ['cb']]
    assert len(calls) == 1 and calls[0][0] == ['p', 'q', 'r'] and calls[0][1] is stage.cls
    assert stage([]) == [] and stage([[], ['s']]) == [[], ['ab']]
    assert len(calls) == 3 and calls[1][0] == [] and calls[2][0] == ['s']
    assert all(isinstance(t, str) for paragraph in stage([['p'], ['q']]) for t in paragraph)


def test_pred_to_text_of_nothing_and_of_wrong_arrays():
    """an empty page needs no device; ranks and class counts are checked before any call"""
    from univer_ocr_amd.nn import CP, ops
    assert ops.pred_to_text([], [-1] * N_CHARS) == []
    good = CP.zeros((6, 4), np.float32)
    for bad in (CP.zeros((1, 6, 4), np.float32), np.zeros((6, 4)), CP.zeros((6, 5), np.float32)):
        with pytest.raises(ValueError, match='pred_to_text'):
            ops.pred_to_text([good, bad], [-1] * 4)


def test_component_files_the_text(monkeypatch):
    from univer_ocr_amd.my_model import crop
    from univer_ocr_amd.my_model.model import make_pred_to_text_component
    from univer_ocr_amd.nn.model_system import RawFunctionComponent
    from univer_ocr_amd.nn.progress_tracker import ProgressTracker
    monkeypatch.setattr(crop.ops, 'pred_to_text', lambda lines, cls: [[79] * (i + 1) for i, _ in enumerate(lines)])
    monkeypatch.setattr(crop.ops, 'as_device', lambda a: a)
    tracker = ProgressTracker(handler=lambda *a: None)
    component = make_pred_to_text_component(tracker)
    assert isinstance(component, RawFunctionComponent) and 'PredToText' in tracker.layers
    for run in (component.train, component.test, component.predict):
        context = {'char_pred': [['a', 'b'], [], ['c']]}
        run(context)
        assert context['text'] == [['b', 'bb'], [], ['bbb']]
    context = {}
    component.predict(context)                                   # no line on the page: the Char net filed nothing
    assert context['text'] == []
    other = make_pred_to_text_component(source='raw', target='words', lines='crops')
    context = {'raw': [['a']], 'crops': [['x'], [], []]}          # paragraphs without lines at the end of the page
    other.predict(context)
    assert context['words'] == [['b'], [], []]
    context = {'crops': [[], []]}
    other.predict(context)
    assert context['words'] == [[], []]


def test_predict_system_is_assembled_in_the_reference_order():
    from univer_ocr_amd.my_model.crop import CropAndRotateParagraphs, CropParagraphs
    from univer_ocr_amd.my_model.model import CharSelector, LineSelector, make_predict_system
    from univer_ocr_amd.nn.model_system import ModelComponent, RawFunctionComponent, StringSelector
    system, models, names = make_predict_system((1, 32, 48, 1))
    assert names == PREDICT_NAMES and list(models) == ['Monochrome', 'Paragraph', 'Line', 'Char']
    assert len(system.components) == len(names)
    for component, name in zip(system.components, names):
        if name in models:
            assert isinstance(component, ModelComponent) and component.name == name and component.model is models[name]
        else:
            assert isinstance(component, RawFunctionComponent)
    labels = lambda c: (c.selector.X_label, c.selector.pred_label)
    mono, paragraph, crop, line, _, char, _ = system.components
    assert type(mono.selector) is StringSelector and labels(mono) == ('monochrome_X', 'monochrome_pred')
    assert type(paragraph.selector) is StringSelector and labels(paragraph) == ('monochrome_pred', 'paragraph_pred')
    assert type(line.selector) is LineSelector and labels(line) == ('cropped_monochrome', 'line_pred')
    assert type(char.selector) is CharSelector and labels(char) == ('cropped_2_monochrome', 'char_pred')
    assert isinstance(crop.stage, CropAndRotateParagraphs) and crop.stage.find_rotation, 'the rotation search is the default'
    upright = make_predict_system((1, 32, 48, 1), find_rotation=False)[0]
    assert isinstance(upright.components[2].stage, CropParagraphs)


def test_make_model_system_still_refuses_predict_and_says_where_it_is():
    from univer_ocr_amd.my_model.model import Modes, make_model_system
    with pytest.raises(NotImplementedError) as refusal:
        make_model_system((1, 32, 48, 1), mode=Modes.PREDICT)
    message = str(refusal.value)
    assert 'make_predict_system' in message and 'PredToText' in message and 'find_rotation' not in message


def test_predict_text_frames_the_page_and_returns_the_text():
    """predict_text with a model system of one component that looks at what it is given"""
    from univer_ocr_amd.my_model import predict
    from univer_ocr_amd.nn.model_system import ModelSystem, RawFunctionComponent
    seen = {}

    def stage(context):
        seen['shape'], seen['type'] = context['monochrome_X'].shape, type(context['monochrome_X']).__name__
        context['text'] = [['ab'], []]
    page = np.random.default_rng(1).random((1, 40, 64, 1))
    context = {}
    assert predict.predict_text(page, ModelSystem([RawFunctionComponent(stage)]), context=context) == [['ab'], []]
    assert seen == {'shape': (1, 48, 80, 1), 'type': 'DeviceArray'} and 'prediction' in context
    with pytest.raises(ValueError, match='predict_text'):
        predict.predict_text(page[0], ModelSystem([]))


# ---- ABI ---------------------------------------------------------------------------------------------------------------
def test_library_exports_the_new_entry_points():
    from univer_ocr_amd.hip import lib as hiplib
    lib = hiplib.get_lib()
    assert lib.uocr_abi_version() == 4
    for name in NEW_SYMBOLS:
        assert getattr(lib, name)
    # without a context both refuse with UOCR_ERR_ARG before touching anything
    assert lib.uocr_pred_to_text(None, 0, 0, None, None, N_CHARS, None, None, None, None) == -1
    assert lib.uocr_ctx_last_pred_to_text(None, None, None, None) == -1
