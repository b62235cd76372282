"""PredToText on the GPU (csrc/pred_to_text.hip) against the reference's PredToText._func1 results in
tests/golden/pred_to_text.npz and, at sizes derived from the kernels' own block and launch sizes, against the NumPy
restatement of the rules that tests/test_pred_to_text_host.py pins to that fixture.  Counts and ids are exact in every
dtype (`==`, no tolerance): the kernels only compare, and every input is a multiple of 1/64 -- the same number in
binary16, float32 and float64 -- or a NaN.  Then the [Char, PredToText] system of fixture (b) and the PREDICT system,
page in, text out."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden
from test_pred_to_text_host import N_CHARS, PAGE, PREDICT_NAMES

pytestmark = pytest.mark.gpu

DTYPES = ('float32', 'float64', 'float16')
FILL = 0xFF                                                        # what every ids buffer holds before a call
SLACK = 5                                                          # bytes of every ids buffer past its capacity


@pytest.fixture(scope='module')
def g():
    return load_golden('pred_to_text')


@pytest.fixture
def rt():
    from univer_ocr_amd.nn import CP
    CP.use_gpu(0)
    CP.set_dtype('float32')
    return CP, CP.runtime()


def rules(x, cls):
    from univer_ocr_amd.my_model.crop import pred_to_text_rules
    return pred_to_text_rules(x, cls)


def raw_call(runtime, dtype, pred, w, n_chars, cls, ids, cap, count, n_lines=None):
    """uocr_pred_to_text on lists of device addresses (None = a null entry; a list that is None: a null array)"""
    from univer_ocr_amd.hip import lib as hiplib
    n = len(w) if n_lines is None else n_lines
    pointers = lambda values: None if values is None else (C.c_void_p * len(values))(*values)
    ints = lambda values: None if values is None else (C.c_int * len(values))(*[int(v) for v in values])
    code = dtype if isinstance(dtype, int) else hiplib.dtype_code(dtype)
    runtime.call('uocr_pred_to_text', code, n, pointers(pred), ints(w), n_chars, ints(cls), pointers(ids), ints(cap), pointers(count))


class Outputs:
    """ids buffers of cap + SLACK bytes, filled with FILL, and counts that start as -7"""

    def __init__(self, CP, caps):
        self.CP, self.caps = CP, [int(c) for c in caps]
        self.ids = [CP.copy(np.full(c + SLACK, FILL, np.uint8), np.uint8) for c in self.caps]
        self.count = [CP.copy(np.full(1, -7, np.int32), np.int32) for _ in self.caps]

    def pointers(self):
        return [a.ptr for a in self.ids], [a.ptr for a in self.count]

    def host(self):
        return [int(self.CP.asnumpy(a)[0]) for a in self.count], [self.CP.asnumpy(a) for a in self.ids]

    def untouched(self):
        counts, ids = self.host()
        return all(c == -7 for c in counts) and all((v == FILL).all() for v in ids)


def run_lines(rt, lines, cls, dtype='float32', caps=None, expected=None, what=''):
    """ONE uocr_pred_to_text call on host arrays (W, n_chars): count and ids EQUAL the expected ids (default: the rules'),
    cut at the capacity (default: the number of expected ids), and no byte past min(count, cap) was touched"""
    CP, runtime = rt
    expected = [rules(x, cls) for x in lines] if expected is None else expected
    caps = [len(e) for e in expected] if caps is None else caps
    dev = [CP.copy(x, dtype) for x in lines]
    out = Outputs(CP, caps)
    ids_ptr, count_ptr = out.pointers()
    raw_call(runtime, dtype, [a.ptr for a in dev], [x.shape[0] for x in lines], lines[0].shape[1], cls, ids_ptr, caps, count_ptr)
    counts, ids = out.host()
    for i, (x, exp, cap) in enumerate(zip(lines, expected, caps)):
        where = f'{what} line {i} {x.shape} {dtype} cap {cap}'
        assert counts[i] == len(exp), f'{where}: count {counts[i]}, expected {len(exp)}'
        kept = min(len(exp), cap)
        assert ids[i][:kept].tolist() == list(exp[:kept]), f'{where}: ids differ'
        assert (ids[i][kept:] == FILL).all(), f'{where}: bytes past min(count, cap) = {kept} were written'
    return counts, ids


def random_table(rng, n_chars):
    """a class table as the ABI allows it: -1 or any class in [0, n_chars), classes of any size, id 0 included"""
    classes = rng.integers(0, max(1, n_chars // 4), n_chars)
    return np.where(rng.random(n_chars) < 0.4, -1, classes).astype(np.int32)


def random_line(rng, w, cls, special=0.25):
    """(w, n_chars) of multiples of 1/64: a clear maximum per row at an id that, four times in ten, shares the class of
    the row before; a tenth tabs; `special` of the rows are instead a 2- or 3-way tie, all zero, -0.0 over negatives, or
    hold a NaN"""
    cls = np.asarray(cls)
    n_chars = len(cls)
    x = rng.integers(-32, 33, (w, n_chars)).astype(np.float64)
    last = 0
    for row in range(w):
        u, kind = rng.random(), rng.random()
        mates = np.flatnonzero(cls == cls[last]) if cls[last] >= 0 else []
        last = 0 if u < 0.1 else int(rng.choice(mates)) if len(mates) and u < 0.5 else int(rng.integers(0, n_chars))
        x[row, last] = 48 + rng.integers(0, 17)
        if kind < special / 4:
            x[row, rng.choice(n_chars, min(n_chars, int(rng.integers(2, 4))), replace=False)] = 64
        elif kind < special / 2:
            x[row] = 0.0
        elif kind < 3 * special / 4:
            x[row] = -np.abs(x[row]) - 1
            x[row, rng.integers(0, n_chars)] = -0.0
        elif kind < special:
            x[row, rng.integers(0, n_chars)] = np.nan
    return x / 64.0


@pytest.fixture
def sizes(rt, g):
    """(rows of a line per block, lines per launch) of the library"""
    run_lines(rt, [g['w1/x']], g['cls'])
    rows, per_launch, launches = rt[1].last_pred_to_text()
    assert rows > 1 and per_launch > 0 and launches == 2
    return rows, per_launch


# ---- fixture (a): the reference's ids ----------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_counts_and_ids_equal_the_reference(dtype, g, rt):
    names = [str(s) for s in g['line_names']]
    expected = [g[f'{name}/ids'].tolist() for name in names]
    run_lines(rt, [g[f'{name}/x'] for name in names], g['cls'], dtype, expected=expected, what='golden')
    assert rt[1].last_pred_to_text()[2] == 2, 'all lines of the fixture fit one launch pair'


# ---- sizes derived from the library's own ----------------------------------------------------------------------------
def boundary_lines(rows, cls):
    """candidates whose predecessor sits in another block: the last row of one block and the first row of the block
    after an EMPTY one hold the two halves of a pair; a paired id in every row of three blocks; the tab between blocks"""
    pair = np.flatnonzero(cls == cls[np.flatnonzero(cls >= 0)[0]])[:2]
    across = np.zeros((3 * rows, len(cls)))
    across[rows - 1, pair[0]] = across[2 * rows, pair[1]] = 1.0
    same = np.zeros((2 * rows + 1, len(cls)))
    same[:, pair[0]] = 0.5
    tab = across.copy()
    tab[rows, 0] = 1.0
    return [across, same, tab]


@pytest.mark.parametrize('dtype', DTYPES)
def test_widths_around_the_block_and_a_long_line_next_to_a_short_one(dtype, sizes, g, rt):
    rows, _ = sizes
    rng = np.random.default_rng(50)
    cls = g['cls']
    lines = [random_line(rng, w, cls) for w in (rows - 1, rows, rows + 1, 1, 700, 2 * rows + 5)] + boundary_lines(rows, cls)
    expected = [rules(x, cls) for x in lines]
    assert [len(e) for e in expected[-3:]] == [1, 1, 2], 'the pair across blocks collapses, unless a tab lies between'
    assert len(expected[4]) > 200
    run_lines(rt, lines, cls, dtype, expected=expected, what='sizes')
    assert rt[1].last_pred_to_text()[2] == 2


def test_more_lines_than_one_launch_takes(sizes, g, rt):
    rows, per_launch = sizes
    rng = np.random.default_rng(51)
    cls = g['cls']
    lines = [random_line(rng, int(rng.integers(1, 6)) if i % 7 else rows + 2, cls) for i in range(per_launch + 1)]
    expected = [rules(x, cls) for x in lines]
    assert len({tuple(e) for e in expected}) > per_launch // 2, 'the lines read differently'
    run_lines(rt, lines, cls, expected=expected, what='many')
    assert rt[1].last_pred_to_text()[2] == 4, 'two launch pairs'
    run_lines(rt, lines[:per_launch], cls, expected=expected[:per_launch], what='exactly one group')
    assert rt[1].last_pred_to_text()[2] == 2


@pytest.mark.parametrize('n_chars', [1, 63, 64, 65, 162, 256])
def test_class_counts_with_random_tables(n_chars, sizes, rt):
    """the 64-column words of a row's candidate mask: full, one short, one over, the most the ABI takes; rows that are not
    16-byte aligned for every n_chars that is no multiple of the vector"""
    rows, _ = sizes
    rng = np.random.default_rng(52 + n_chars)
    cls = random_table(rng, n_chars)
    lines = [random_line(rng, w, cls, special=0.3) for w in (rows + 3, 7, 1)]
    lines.append(np.full((3, n_chars), 0.25))                      # every column a candidate, three times
    expected = [rules(x, cls) for x in lines]
    assert n_chars == 1 or max(len(e) for e in expected) > rows // 2
    for dtype in DTYPES:
        run_lines(rt, lines, cls, dtype, expected=expected, what=f'n_chars={n_chars}')


def test_rows_off_the_vector_alignment(sizes, g, rt):
    """a line that starts 4 bytes past a 16-byte border: its rows begin 4 or 12 bytes past one, so every row has a
    scalar head and tail around its 16-byte loads; the maximum of some rows sits in the head, of others in the tail"""
    CP, runtime = rt
    rows, _ = sizes
    rng = np.random.default_rng(53)
    cls = g['cls']
    x = random_line(rng, rows + 9, cls, special=0.1)
    x[3], x[4], x[5], x[6] = -0.5, -0.5, -0.5, -0.5
    x[3, 1], x[4, 2], x[5, N_CHARS - 1], x[6, N_CHARS - 2] = 0.75, 0.75, 0.75, 0.75
    expected = rules(x, cls)
    for offset in (1, 2, 3):
        buffer = CP.copy(np.concatenate([np.full(offset, np.nan), x.reshape(-1), np.full(4, np.nan)]), np.float32)
        assert buffer.ptr % 16 == 0
        out = Outputs(CP, [len(expected)])
        ids_ptr, count_ptr = out.pointers()
        raw_call(runtime, 'float32', [buffer.ptr + 4 * offset], [x.shape[0]], N_CHARS, cls, ids_ptr, out.caps, count_ptr)
        counts, ids = out.host()
        assert counts == [len(expected)] and ids[0][:len(expected)].tolist() == expected and (ids[0][len(expected):] == FILL).all()


# ---- capacity ------------------------------------------------------------------------------------------------------------
def test_capacity_cuts_the_ids_and_never_the_count(g, rt):
    CP, runtime = rt
    cls = g['cls']
    names = ('w64', 'ties', 'hand', 'w8')
    lines, expected = [g[f'{name}/x'] for name in names], [g[f'{name}/ids'].tolist() for name in names]
    run_lines(rt, lines, cls, caps=[0, 0, 0, 0], expected=expected, what='cap 0')
    run_lines(rt, lines, cls, caps=[len(e) - 1 for e in expected], expected=expected, what='cap = count - 1')
    run_lines(rt, lines, cls, caps=[len(expected[0]) + 3, 1, len(expected[2]), 0], expected=expected, what='mixed')
    dev = [CP.copy(x, np.float32) for x in lines]                  # cap 0 takes a null ids pointer
    out = Outputs(CP, [0] * 4)
    raw_call(runtime, 'float32', [a.ptr for a in dev], [x.shape[0] for x in lines], N_CHARS, cls, [None] * 4, [0] * 4, out.pointers()[1])
    assert out.host()[0] == [len(e) for e in expected]


def test_wrapper_makes_one_call_and_a_second_only_for_ties(g, rt, monkeypatch):
    from univer_ocr_amd.my_model.crop import PredToText
    from univer_ocr_amd.nn import ops
    CP, runtime = rt
    cls = g['cls']
    calls = []
    original = runtime.call
    monkeypatch.setattr(runtime, 'call', lambda name, *args: (calls.append(name), original(name, *args))[1])
    for dtype in DTYPES:
        plain = ['w1', 'w8', 'w17', 'w64', 'w130', 'w300', 'zeros']
        dev = [CP.copy(g[f'{name}/x'], dtype) for name in plain]
        del calls[:]
        assert ops.pred_to_text(dev, cls) == [g[f'{name}/ids'].tolist() for name in plain]
        assert calls.count('uocr_pred_to_text') == 1, 'a page without ties: one call'
        names = [str(s) for s in g['line_names']]
        dev = [CP.copy(g[f'{name}/x'], dtype) for name in names]
        del calls[:]
        assert ops.pred_to_text(dev, cls) == [g[f'{name}/ids'].tolist() for name in names]
        assert calls.count('uocr_pred_to_text') == 2, 'hand and ties emit more ids than they have rows: one more call'
        del calls[:]
        texts = PredToText()([dev[:2], [], dev[2:]])
        assert calls.count('uocr_pred_to_text') == 2
        assert texts == [[str(g[f'{name}/text']) for name in names[:2]], [], [str(g[f'{name}/text']) for name in names[2:]]]
    monkeypatch.undo()


# ---- arguments -----------------------------------------------------------------------------------------------------------
def test_argument_errors_write_nothing(g, rt):
    from univer_ocr_amd.hip import HipError
    CP, runtime = rt
    cls = g['cls'].tolist()
    x = [CP.copy(g['w8/x'], np.float32), CP.copy(g['w17/x'], np.float32)]
    out = Outputs(CP, [8, 17])
    ids_ptr, count_ptr = out.pointers()
    good = dict(dtype='float32', pred=[a.ptr for a in x], w=[8, 17], n_chars=N_CHARS, cls=cls, ids=ids_ptr, cap=[8, 17],
                count=count_ptr, n_lines=2)
    bad = [(dict(pred=None), -1), (dict(w=None), -1), (dict(cls=None), -1), (dict(ids=None), -1), (dict(cap=None), -1),
           (dict(count=None), -1), (dict(n_lines=-1), -1), (dict(pred=[x[0].ptr, None]), -1), (dict(ids=[None, ids_ptr[1]]), -1),
           (dict(count=[count_ptr[0], None]), -1), (dict(w=[8, 0]), -1), (dict(w=[-3, 17]), -1), (dict(cap=[8, -1]), -1),
           (dict(n_chars=0), -1), (dict(n_chars=257, cls=[-1] * 257), -1), (dict(cls=[-2] + cls[1:]), -1),
           (dict(cls=cls[:-1] + [N_CHARS]), -1), (dict(pred=[x[0].ptr, x[1].ptr + 2]), -1),
           (dict(count=[count_ptr[0], count_ptr[1] + 2]), -1), (dict(dtype=7), -2)]
    for change, code in bad:
        with pytest.raises(HipError, match=rf'\({code}\)'):
            raw_call(runtime, **dict(good, **change))
        assert out.untouched(), f'{change}: the outputs were touched'
    before = runtime.last_pred_to_text()
    raw_call(runtime, **dict(good, n_lines=0))                     # nothing to do: OK, no launch
    raw_call(runtime, 'float32', None, None, N_CHARS, None, None, None, None, n_lines=0)   # ... whatever else is passed
    assert out.untouched() and runtime.last_pred_to_text() == before
    raw_call(runtime, **good)
    assert out.host()[0] == [len(g['w8/ids']), len(g['w17/ids'])]


# ---- repeatability, capture ----------------------------------------------------------------------------------------------
def test_second_call_after_a_larger_one_and_repeatability(sizes, g, rt):
    """masks and summaries of a larger call stay in the workspace: a smaller call must not read them; the same call twice
    gives the same bytes"""
    rows, _ = sizes
    rng = np.random.default_rng(54)
    cls = g['cls']
    big = [random_line(rng, 3 * rows + 1, cls), random_line(rng, 2 * rows, cls)]
    small = [random_line(rng, rows + 1, cls), np.zeros((rows, N_CHARS))]
    first = run_lines(rt, big, cls, what='big')
    run_lines(rt, small, cls, what='small after big')
    again = run_lines(rt, big, cls, what='big again')
    assert first[0] == again[0] and all(a.tobytes() == b.tobytes() for a, b in zip(first[1], again[1]))


def test_capture_and_replay(sizes, g, rt):
    """the call is asynchronous and capturable: a replayed graph reads what the input buffers hold then"""
    import torch
    CP, runtime = rt
    rows, _ = sizes
    rng = np.random.default_rng(55)
    cls = g['cls']
    widths = (2 * rows + 3, 5)
    versions = [[random_line(rng, w, cls) for w in widths] for _ in range(2)]
    caps = [2 * w for w in widths]
    dev = [CP.copy(x, np.float32) for x in versions[0]]
    out = Outputs(CP, caps)
    ids_ptr, count_ptr = out.pointers()
    with runtime.capture(torch.cuda.MemPool()) as graph:
        raw_call(runtime, 'float32', [a.ptr for a in dev], widths, N_CHARS, cls, ids_ptr, caps, count_ptr)
    for lines in versions[::-1] + versions:
        for a, x in zip(dev, lines):
            a.set(x)
        for a in out.ids:
            a.set(np.full(a.shape, FILL, np.uint8))
        graph.replay()
        counts, ids = out.host()
        for i, x in enumerate(lines):
            exp = rules(x, cls)
            assert counts[i] == len(exp) <= caps[i] and ids[i][:len(exp)].tolist() == exp and (ids[i][len(exp):] == FILL).all()


# ---- fixture (b): the [Char, PredToText] system --------------------------------------------------------------------------
def test_char_and_pred_to_text_system_gives_the_reference_texts(g, rt):
    """the device Char net, float32, analytic weights, on the page of fixture (b), through ModelSystem.predict: every
    row's maximum is clear by 1e-3 of the line's largest output in the reference (asserted by the generator and by the
    host test), so the texts are the reference's"""
    from test_gpu_models import set_analytic_weights
    from univer_ocr_amd.my_model.model import CharSelector, make_char, make_pred_to_text_component
    from univer_ocr_amd.nn.model_system import ModelComponent, ModelSystem
    CP, _ = rt
    char = make_char(g['system/mono0_0'].shape)
    set_analytic_weights(char)
    system = ModelSystem([ModelComponent('Char', char, CharSelector('cropped_2_monochrome', None, 'char_pred'), delist_result=True),
                          make_pred_to_text_component()])
    context = {'cropped_2_monochrome': [[CP.copy(g['system/mono0_0']), CP.copy(g['system/mono0_1'])], [CP.copy(g['system/mono1_0'])]]}
    system.predict(context)
    assert [len(p) for p in context['char_pred']] == [2, 1]
    for p, l in PAGE:
        pred, ref = CP.asnumpy(context['char_pred'][p][l]), g[f'system/char_pred{p}_{l}']
        err = np.max(np.abs(pred - ref)) / np.max(np.abs(ref))
        print(f'char_pred[{p}][{l}]: rel_linf {err:.2e}')
        assert err < 5e-4, 'the net is further from the reference than half the margin of the maxima'
    assert context['text'] == [[str(g['system/text0_0']), str(g['system/text0_1'])], [str(g['system/text1_0'])]]


# ---- the PREDICT system, page in, text out -------------------------------------------------------------------------------
def planted_paragraphs(shape):
    """(1, H, W, 1): an upright paragraph in the upper half, one turned by 15 degrees in the lower half"""
    _, h, w, _ = shape
    mask = np.zeros(shape)
    mask[0, h // 10:h * 4 // 10, w // 10:w * 9 // 10, 0] = 1.0
    y, x = np.mgrid[0:h, 0:w]
    c, s = np.cos(np.deg2rad(15)), np.sin(np.deg2rad(15))
    along, across = (x - w / 2) * c + (y - h * 0.73) * s, -(x - w / 2) * s + (y - h * 0.73) * c
    mask[0, :, :, 0][(np.abs(along) < w * 0.33) & (np.abs(across) < h * 0.1)] = 1.0
    assert not mask[0, h * 4 // 10:h * 4 // 10 + 2].any(), 'the two paragraphs touch'
    return mask


def planted_lines(shape):
    """(1, h, w, 2) for a paragraph crop (1, h, w, 1): two lines, top and bottom band each"""
    _, h, w, _ = shape
    mask = np.zeros((1, h, w, 2))
    for first in (h // 8, 5 * h // 8):
        mask[0, first:first + 2, w // 8:7 * w // 8, 0] = 1.0
        mask[0, first + h // 4 - 2:first + h // 4, w // 8:7 * w // 8, 1] = 1.0
    return mask


@pytest.mark.parametrize('find_rotation', [True, False])
def test_predict_system_page_in_text_out(find_rotation, rt, monkeypatch):
    """a 64 x 96 synthetic page through predict_text.  The seeded nets are not trained, so the paragraph and line masks
    are planted behind the Paragraph and Line nets (which still run); everything after them works on what the stages
    before it filed."""
    from test_gpu_models import set_analytic_weights
    from univer_ocr_amd.my_model.crop import CHARS, pred_to_text_rules
    from univer_ocr_amd.my_model.model import make_divisible_by, make_predict_system
    from univer_ocr_amd.my_model.predict import predict_text
    from univer_ocr_amd.my_model.synthetic import make_page_batch
    from univer_ocr_amd.nn.gpu import DeviceArray
    from univer_ocr_amd.nn.model_system import RawFunctionComponent
    CP, runtime = rt
    page = make_page_batch(1, 64, 96, seed=7)['image']
    framed = make_divisible_by(page, 16, 16).shape
    system, models, names = make_predict_system(framed, find_rotation=find_rotation)
    assert names == PREDICT_NAMES and len(system.components) == 7
    for model in models.values():
        set_analytic_weights(model)

    def plant_paragraphs(context):
        assert context['paragraph_pred'].shape == framed
        context['paragraph_pred'] = CP.copy(planted_paragraphs(framed))

    def plant_lines(context):
        assert len(context['line_pred']) == 2
        context['line_pred'] = [CP.copy(planted_lines(crop.shape)) for crop in context['cropped_monochrome']]
    system.components.insert(names.index('ParagraphCrop'), RawFunctionComponent(plant_paragraphs))
    system.components.insert(names.index('LineCrop') + 1, RawFunctionComponent(plant_lines))
    calls = []
    original = runtime.call
    monkeypatch.setattr(runtime, 'call', lambda name, *args: (calls.append(name), original(name, *args))[1])
    context = {}
    text = predict_text(page, system, context=context)
    monkeypatch.undo()
    assert text is context['text'] and not [key for key in context if key.endswith('_cpu')]
    crops, preds = context['cropped_2_monochrome'], context['char_pred']
    assert [len(p) for p in crops] == [2, 2], 'two paragraphs of two lines each'
    assert [len(p) for p in text] == [len(p) for p in crops] == [len(p) for p in preds]
    for p, per_line in enumerate(preds):
        for l, pred in enumerate(per_line):
            assert isinstance(pred, DeviceArray) and pred.shape == (crops[p][l].shape[2], N_CHARS)
            assert isinstance(text[p][l], str)
            assert text[p][l] == ''.join(CHARS[i] for i in pred_to_text_rules(CP.asnumpy(pred))), f'text[{p}][{l}]'
    angles = system.components[names.index('ParagraphCrop') + 1].stage.angles if find_rotation else [None, None]
    if find_rotation:
        assert angles[0] is None and angles[1] is not None, angles
    assert calls.count('uocr_rotated_extent') == (14 if find_rotation else 0)
    assert calls.count('uocr_rotate_crop') == (1 if find_rotation else 0)
    assert calls.count('uocr_line_crop') == 1 and calls.count('uocr_pred_to_text') in (1, 2)


@pytest.mark.parametrize('case', ['no paragraph', 'last paragraph without lines'])
def test_predict_system_where_stages_find_nothing(case, rt):
    """a page on which the Paragraph net marks nothing reads []; a paragraph in which the Line net marks nothing reads []
    even at the end of the page, where the Char net files no entry for it"""
    from univer_ocr_amd.my_model.model import make_predict_system
    from univer_ocr_amd.nn.model_system import RawFunctionComponent
    CP, _ = rt
    shape = (1, 80, 112, 1)
    system, _, names = make_predict_system(shape, find_rotation=False)

    def plant_paragraphs(context):
        context['paragraph_pred'] = CP.copy(np.zeros(shape) if case == 'no paragraph' else planted_paragraphs(shape))

    def plant_lines(context):
        crops = context['cropped_monochrome']
        context['line_pred'] = [CP.copy(planted_lines(crop.shape) * (p == 0)) for p, crop in enumerate(crops)]
    system.components.insert(names.index('ParagraphCrop'), RawFunctionComponent(plant_paragraphs))
    if case != 'no paragraph':
        system.components.insert(names.index('LineCrop') + 1, RawFunctionComponent(plant_lines))
    context = {'monochrome_X': CP.copy(np.random.default_rng(3).random(shape))}
    system.predict(context)
    if case == 'no paragraph':
        assert context['cropped_monochrome'] == [] and context['cropped_2_monochrome'] == [] and context['text'] == []
        assert 'line_pred' not in context and 'char_pred' not in context
    else:
        assert [len(p) for p in context['cropped_2_monochrome']] == [2, 0] and len(context['char_pred']) == 1
        assert [len(p) for p in context['text']] == [2, 0] and all(isinstance(t, str) for t in context['text'][0])
