"""The packed Char pass on the GPU: uocr_pack_lines and uocr_zero_gaps (csrc/pack_lines.hip) against a NumPy restatement,
bit for bit in every dtype, at sizes derived from the kernel's own block and launch sizes; then Model.forward(keep_columns=)
on the lines of fixture (b) of tests/golden/pred_to_text.npz laid side by side against the reference's per-line
predictions and the float64 oracle, and PackedLinesComponent / make_predict_system(char_batching='page') against the pass
per line."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden, rel_linf
from test_pred_to_text_host import N_CHARS, PAGE

pytestmark = pytest.mark.gpu

DTYPES = ('float32', 'float64', 'float16')
BITS = {'float32': np.uint32, 'float64': np.uint64, 'float16': np.uint16}
WIDTHS = [8, 9, 17, 24, 40, 1, 131]
CHAR_BOUND = 5e-4            # of the reference's char_pred: half the margin of the row maxima fixture (b) guarantees


@pytest.fixture(scope='module')
def g():
    return load_golden('pred_to_text')


@pytest.fixture
def rt():
    from univer_ocr_amd.nn import CP
    CP.use_gpu(0)
    CP.set_dtype('float32')
    yield CP, CP.runtime()
    CP.set_dtype('float32')


def gapped(widths, gap=4, before=0):
    """x0 of lines `widths` wide with `gap` columns between neighbours, and the width of the strip that ends with the last"""
    x0 = [before + sum(widths[:k]) + gap * k for k in range(len(widths))]
    return x0, x0[-1] + widths[-1]


EVEN = (WIDTHS,) + gapped(WIDTHS)                                   # (w, x0, strip_w): 4 columns between neighbours
UNEVEN = ([8, 9, 17, 1], [11, 19, 31, 50], 58)                      # 11 before the first, 0 between two lines, 7 behind the last


def pack_rules(lines, x0, strip_w):
    """what uocr_pack_lines writes: the lines at their columns, +0.0 everywhere else"""
    _, h, _, c = lines[0].shape
    strip = np.zeros((1, h, strip_w, c), lines[0].dtype)
    for x, start in zip(lines, x0):
        strip[:, :, start:start + x.shape[2]] = x
    return strip


def gap_mask(x0, w, strip_w):
    mask = np.ones(strip_w, bool)
    for start, width in zip(x0, w):
        mask[start:start + width] = False
    return mask


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(BITS[str(a.dtype)]), b.view(BITS[str(b.dtype)]))


def random_lines(rng, widths, h, c, dtype):
    """multiples of 1/64 of either sign, a -0.0 in every line: the same numbers in every dtype"""
    lines = [(rng.integers(-64, 65, (1, h, w, c)) / 64.0).astype(dtype) for w in widths]
    for x in lines:
        x[0, h // 2, 0, 0] = -0.0
    return lines


_ptrs = lambda values: None if values is None else (C.c_void_p * len(values))(*values)
_ints = lambda values: None if values is None else (C.c_int * len(values))(*[int(v) for v in values])


def _code(dtype):
    from univer_ocr_amd.hip import lib as hiplib
    return dtype if isinstance(dtype, int) else hiplib.dtype_code(dtype)


def raw_pack(runtime, dtype, src, w, h, c, x0, strip, strip_w, n_lines=None):
    """uocr_pack_lines on lists (device addresses for src; None = a null entry, a list given as None = a null array)"""
    runtime.call('uocr_pack_lines', _code(dtype), len(w) if n_lines is None else n_lines, _ptrs(src), _ints(w), h, c, _ints(x0),
                 strip, strip_w)


def raw_zero(runtime, dtype, x, h, strip_w, c, x0, w, n_lines=None):
    runtime.call('uocr_zero_gaps', _code(dtype), x, h, strip_w, c, len(w) if n_lines is None else n_lines, _ints(x0), _ints(w))


def nan_strip(CP, h, strip_w, c, dtype):
    return CP.copy(np.full((1, h, strip_w, c), np.nan), dtype)


def run_pack(rt, lines, x0, strip_w, what=''):
    """ONE uocr_pack_lines call on host lines into a strip full of NaN: the strip EQUALS the restatement bit for bit and
    the sources are as they were"""
    CP, runtime = rt
    dtype = str(lines[0].dtype)
    _, h, _, c = lines[0].shape
    dev = [CP.copy(x, dtype) for x in lines]
    strip = nan_strip(CP, h, strip_w, c, dtype)
    raw_pack(runtime, dtype, [a.ptr for a in dev], [x.shape[2] for x in lines], h, c, x0, strip.ptr, strip_w)
    got = CP.asnumpy(strip)
    assert not np.isnan(got).any(), f'{what} {dtype}: an element of the strip was not written'
    assert same_bits(got, pack_rules(lines, x0, strip_w)), f'{what} {dtype}: the strip differs from the restatement'
    assert all(same_bits(CP.asnumpy(a), x) for a, x in zip(dev, lines)), f'{what} {dtype}: a source changed'
    return strip


def run_zero(rt, shape, x0, w, dtype, what=''):
    """ONE uocr_zero_gaps call on a tensor with NaN, infinities and finite numbers in its gaps: the gaps are +0.0
    afterwards, every element of a segment has the bits it had"""
    CP, runtime = rt
    _, h, strip_w, c = shape
    rng = np.random.default_rng(strip_w + h)
    host = (rng.integers(-64, 65, shape) / 64.0).astype(dtype)
    host[0, 0, :, 0] = -0.0
    junk = np.resize(np.array([np.nan, np.inf, -np.inf, -0.0, 3.5], dtype), shape)
    gaps = gap_mask(x0, w, strip_w)
    host[:, :, gaps] = junk[:, :, gaps]
    x = CP.copy(host, dtype)
    raw_zero(runtime, dtype, x.ptr, h, strip_w, c, x0, w)
    got = CP.asnumpy(x)
    assert (got[:, :, gaps].view(BITS[dtype]) == 0).all(), f'{what} {shape} {dtype}: a gap element is not +0.0'
    assert same_bits(got[:, :, ~gaps], host[:, :, ~gaps]), f'{what} {shape} {dtype}: an element of a segment changed'


@pytest.fixture
def sizes(rt):
    """(elements of an entry per block at most, entries per launch) of the library"""
    run_pack(rt, random_lines(np.random.default_rng(0), [8], 32, 1, 'float32'), [0], 8)
    chunk, per_launch, launches = rt[1].last_pack_lines()
    assert chunk > 64 and per_launch > 1 and launches == 1
    return chunk, per_launch


# ---- 1: pack ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_pack_equals_the_restatement(dtype, rt):
    rng = np.random.default_rng(1)
    w, x0, strip_w = EVEN
    assert strip_w == sum(WIDTHS) + 4 * (len(WIDTHS) - 1)
    run_pack(rt, random_lines(rng, w, 32, 1, dtype), x0, strip_w, 'gap 4')
    assert rt[1].last_pack_lines()[2] == 1, 'one launch for the page'
    w, x0, strip_w = UNEVEN
    run_pack(rt, random_lines(rng, w, 3, 5, dtype), x0, strip_w, 'uneven gaps, 3 rows of 5 channels')
    run_pack(rt, random_lines(rng, [5], 2, 3, dtype), [0], 5, 'one line that is the strip')


# ---- 2: zero gaps ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_zero_gaps_writes_the_gaps_and_nothing_else(dtype, rt):
    w, x0, strip_w = EVEN
    for h, c in ((14, 64), (5, 64), (1, 64), (32, 1)):
        run_zero(rt, (1, h, strip_w, c), x0, w, dtype)
        assert rt[1].last_pack_lines()[2] == 1
    w, x0, strip_w = UNEVEN
    run_zero(rt, (1, 3, strip_w, 5), x0, w, dtype, 'uneven gaps')
    # a strip without a gap: nothing to write, nothing launched
    CP, runtime = rt
    host = (np.random.default_rng(2).integers(-64, 65, (1, 5, 17, 64)) / 64.0).astype(dtype)
    x = CP.copy(host, dtype)
    raw_zero(runtime, dtype, x.ptr, 5, 17, 64, [0, 8], [8, 9])
    assert same_bits(CP.asnumpy(x), host) and runtime.last_pack_lines()[2] == 0


# ---- 3: sizes derived from the library's own --------------------------------------------------------------------------------
def test_more_lines_than_one_launch_takes(sizes, rt):
    CP, runtime = rt
    _, per_launch = sizes
    rng = np.random.default_rng(3)
    for n in (per_launch + 1, per_launch):
        widths = [8] * n
        x0, strip_w = gapped(widths)
        lines = random_lines(rng, widths, 32, 1, 'float32')
        assert len({x.tobytes() for x in lines}) == n, 'the lines differ'
        run_pack(rt, lines, x0, strip_w, f'{n} lines')
        assert runtime.last_pack_lines()[2] == -(-n // per_launch)
        # n + 1 gaps, the first and the last without columns: a group that holds only those is not launched
        run_zero(rt, (1, 2, strip_w, 64), x0, widths, 'float32', f'{n} lines')
        assert runtime.last_pack_lines()[2] == -(-n // per_launch)


@pytest.mark.parametrize('dtype', DTYPES)
def test_a_line_of_several_blocks_next_to_a_line_of_one_column(dtype, sizes, rt):
    chunk, _ = sizes
    rng = np.random.default_rng(4)
    widths = [chunk // 32 + 5, 1]                                   # more elements than a block takes, in whole rows
    assert 32 * widths[0] > chunk
    x0, strip_w = gapped(widths)
    run_pack(rt, random_lines(rng, widths, 32, 1, dtype), x0, strip_w, 'rows shared among blocks')
    for widths in ([chunk + 37, 1], [1, 2 * chunk + 1], [chunk - 4, 1]):   # rows longer than a block takes: cut into pieces
        x0, strip_w = gapped(widths, before=3)
        run_pack(rt, random_lines(rng, widths, 3, 1, dtype), x0, strip_w + 2, f'rows of {widths[0]} elements')
    widths = [chunk // 5 + 3, 1]
    x0, strip_w = gapped(widths)
    run_pack(rt, random_lines(rng, widths, 2, 5, dtype), x0, strip_w, '5 channels, a row longer than a block takes')
    run_zero(rt, (1, 3, 2 * chunk + 40, 1), [chunk + 20], [7], dtype, 'gaps longer than a block takes')
    run_zero(rt, (1, 40, 300, 64), [3, 200], [100, 60], dtype, 'gaps of several blocks of rows')


# ---- 4: arguments ----------------------------------------------------------------------------------------------------------
def test_argument_errors_write_nothing(rt):
    from univer_ocr_amd.hip import HipError
    CP, runtime = rt
    rng = np.random.default_rng(5)
    lines = [CP.copy(x, np.float32) for x in random_lines(rng, [8, 9], 4, 1, 'float32')]
    strip = nan_strip(CP, 4, 24, 1, 'float32')
    src = [a.ptr for a in lines]
    untouched = lambda: np.isnan(CP.asnumpy(strip)).all()
    good = dict(dtype='float32', src=src, w=[8, 9], h=4, c=1, x0=[2, 14], strip=strip.ptr, strip_w=24, n_lines=2)
    segments = [(dict(x0=[2, 9]), -1), (dict(x0=[14, 2]), -1), (dict(x0=[2, 16]), -1), (dict(x0=[-1, 14]), -1),
                (dict(w=[8, 0]), -1), (dict(w=[-8, 9]), -1), (dict(w=None), -1), (dict(x0=None), -1), (dict(strip=None), -1),
                (dict(strip=strip.ptr + 2), -1), (dict(n_lines=-1), -1), (dict(h=0), -1), (dict(c=0), -1), (dict(strip_w=0), -1),
                (dict(dtype=7), -2)]
    sources = [(dict(src=None), -1), (dict(src=[src[0], None]), -1), (dict(src=[src[0], src[1] + 2]), -1)]
    for change, code in segments + sources:
        with pytest.raises(HipError, match=rf'\({code}\)'):
            raw_pack(runtime, **dict(good, **change))
        assert untouched(), f'pack {change}: the strip was touched'
    zero = lambda **change: (lambda a: raw_zero(runtime, a['dtype'], a['strip'], a['h'], a['strip_w'], a['c'], a['x0'], a['w'],
                                                a['n_lines']))(dict(good, **change))
    for change, code in segments:
        with pytest.raises(HipError, match=rf'\({code}\)'):
            zero(**change)
        assert untouched(), f'zero gaps {change}: the tensor was touched'
    run_pack(rt, random_lines(rng, [8], 4, 1, 'float32'), [0], 8)
    before = runtime.last_pack_lines()
    assert before[2] == 1
    raw_pack(runtime, **dict(good, n_lines=0))                     # nothing to do: OK, no launch
    raw_pack(runtime, 'float32', None, None, 4, 1, None, None, 24, n_lines=0)   # ... whatever else is passed
    zero(n_lines=0)
    raw_zero(runtime, 'float32', None, 4, 24, 1, None, None, n_lines=0)
    assert untouched() and runtime.last_pack_lines() == before
    raw_pack(runtime, **good)
    host = CP.asnumpy(strip)
    assert same_bits(host, pack_rules([CP.asnumpy(a) for a in lines], [2, 14], 24))


# ---- 5: capture ------------------------------------------------------------------------------------------------------------
def test_capture_and_replay(rt):
    """both calls are asynchronous and capturable: a replayed graph reads what the sources hold then"""
    import torch
    CP, runtime = rt
    rng = np.random.default_rng(6)
    w, x0, strip_w = EVEN
    versions = [random_lines(rng, w, 32, 1, 'float32') for _ in range(2)]
    dev = [CP.copy(x, np.float32) for x in versions[0]]
    strip = nan_strip(CP, 32, strip_w, 1, 'float32')
    kept = [i for i in range(len(w)) if i != 3]                    # the segments of the second call: line 3 becomes a gap
    with runtime.capture(torch.cuda.MemPool()) as graph:
        raw_pack(runtime, 'float32', [a.ptr for a in dev], w, 32, 1, x0, strip.ptr, strip_w)
        raw_zero(runtime, 'float32', strip.ptr, 32, strip_w, 1, [x0[i] for i in kept], [w[i] for i in kept])
    for lines in versions[::-1] + versions:
        for a, x in zip(dev, lines):
            a.set(x)
        strip.set(np.full(strip.shape, np.nan, np.float32))
        graph.replay()
        expected = pack_rules(lines, x0, strip_w)
        expected[:, :, x0[3]:x0[3] + w[3]] = 0.0
        assert same_bits(CP.asnumpy(strip), expected)


# ---- 6: the model on a strip -----------------------------------------------------------------------------------------------
def page_lines(g):
    return [g[f'system/mono{p}_{l}'] for p, l in PAGE]


def packed_forward(CP, char, lines, keep=True):
    """the lines laid side by side with 4 columns between them through ONE forward; the views of the lines' rows"""
    from univer_ocr_amd.nn import ops
    from univer_ocr_amd.nn.gpu import DeviceArray
    (segments, strip_w), = ops.pack_layout([x.shape[2] for x in lines])
    strip = ops.pack_lines([CP.copy(x) for x in lines], (segments, strip_w))
    out, = char.forward(strip, keep_columns=[(x0, w) for _, x0, w in segments] if keep else None)
    assert out.shape == (strip_w, N_CHARS)
    return [CP.asnumpy(DeviceArray(out.t[x0:x0 + w])) for _, x0, w in segments]


@pytest.mark.parametrize('fused', [False, True], ids=['layer by layer', 'fused graph'])
def test_forward_with_keep_columns_gives_every_line_its_own_prediction(fused, g, rt):
    from test_gpu_models import set_analytic_weights
    from univer_ocr_amd.my_model.model import make_char
    CP, _ = rt
    lines = page_lines(g)
    assert [x.shape[2] for x in lines] == [24, 40, 17]
    char = make_char(lines[0].shape)
    if fused:
        char.enable_fusion()
    set_analytic_weights(char)
    assert len(char._wins_used) == fused
    refs = [g[f'system/char_pred{p}_{l}'] for p, l in PAGE]
    errs = [rel_linf(pred, ref) for pred, ref in zip(packed_forward(CP, char, lines), refs)]
    print('packed, gaps re-zeroed: rel_linf ' + ', '.join(f'{e:.2e}' for e in errs))
    assert max(errs) < CHAR_BOUND, 'a line on the strip is further from the reference than the line alone may be'
    stale = [rel_linf(pred, ref) for pred, ref in zip(packed_forward(CP, char, lines, keep=False), refs)]
    print('packed, gaps left as they are: rel_linf ' + ', '.join(f'{e:.2e}' for e in stale))
    assert max(stale) >= CHAR_BOUND, 'the bound does not see what the gaps hold: the test above shows nothing'
    # a strip that is one line of 8 columns: as wide as its own windows, no gap, the same launches as without segments
    narrow = CP.copy(lines[0][:, :, :8])
    alone = CP.asnumpy(char.forward(narrow)[0])
    assert np.array_equal(CP.asnumpy(char.forward(narrow, keep_columns=[(0, 8)])[0]), alone) and alone.shape == (8, N_CHARS)


def test_forward_with_keep_columns_in_float64_against_the_oracle(g, rt):
    from oracle import nn_oracle as O
    from test_gpu_models import PASS_TOL, set_analytic_weights
    from univer_ocr_amd.my_model.model import make_char
    CP, _ = rt
    CP.set_dtype('float64')
    lines = page_lines(g)
    char = make_char(lines[0].shape)
    set_analytic_weights(char)
    net = O.make_net('Char')
    refs = [net.forward(np.asarray(x, np.float64)) for x in lines]
    errs = [rel_linf(pred, ref) for pred, ref in zip(packed_forward(CP, char, lines), refs)]
    print('float64, packed against the oracle line by line: rel_linf ' + ', '.join(f'{e:.2e}' for e in errs))
    assert max(errs) <= PASS_TOL['float64'], "beyond the tolerance of the Char net's float64 forward (tests/test_gpu_models.py)"


# ---- 7, 8: the component ---------------------------------------------------------------------------------------------------
def char_system(g, CP, **packing):
    from test_gpu_models import set_analytic_weights
    from univer_ocr_amd.my_model.model import CharSelector, PackedLinesComponent, make_char, make_pred_to_text_component
    from univer_ocr_amd.nn.model_system import ModelSystem
    char = make_char(g['system/mono0_0'].shape)
    set_analytic_weights(char)
    component = PackedLinesComponent('Char', char, CharSelector('cropped_2_monochrome', None, 'char_pred'), delist_result=True,
                                     **packing)
    context = {'cropped_2_monochrome': [[CP.copy(g['system/mono0_0']), CP.copy(g['system/mono0_1'])], [CP.copy(g['system/mono1_0'])]]}
    return ModelSystem([component, make_pred_to_text_component()]), char, context


def recorded(runtime, monkeypatch):
    calls = []
    original = runtime.call
    monkeypatch.setattr(runtime, 'call', lambda name, *args: (calls.append(name), original(name, *args))[1])
    return calls


def check_page(g, CP, context):
    from univer_ocr_amd.nn.gpu import DeviceArray
    assert [len(p) for p in context['char_pred']] == [2, 1]
    for p, l in PAGE:
        pred, ref = context['char_pred'][p][l], g[f'system/char_pred{p}_{l}']
        assert isinstance(pred, DeviceArray) and pred.shape == ref.shape == (g[f'system/mono{p}_{l}'].shape[2], N_CHARS)
        assert pred.t.is_contiguous()
        err = rel_linf(CP.asnumpy(pred), ref)
        print(f'char_pred[{p}][{l}]: rel_linf {err:.2e}')
        assert err < CHAR_BOUND
    assert context['text'] == [[str(g['system/text0_0']), str(g['system/text0_1'])], [str(g['system/text1_0'])]]
    last, = context['prediction']['Char']
    assert last.ptr == context['char_pred'][1][0].ptr and last.shape == context['char_pred'][1][0].shape, 'the last line, as per line'


def test_packed_component_and_pred_to_text_give_the_reference_texts(g, rt, monkeypatch):
    CP, runtime = rt
    system, char, context = char_system(g, CP)
    calls = recorded(runtime, monkeypatch)
    char.forward(context['cropped_2_monochrome'][0][1])
    one_forward = calls.count('uocr_conv2d_fwd')
    assert one_forward >= 3 and 'uocr_zero_gaps' not in calls and 'uocr_pack_lines' not in calls
    del calls[:]
    system.predict(context)
    monkeypatch.undo()
    check_page(g, CP, context)
    assert calls.count('uocr_pack_lines') == 1 and calls.count('uocr_zero_gaps') == 3
    assert calls.count('uocr_conv2d_fwd') == one_forward, 'one pass for the page, not one per line'


@pytest.mark.parametrize('max_columns,strips', [(64, 2), (48, 3)])
def test_packed_component_takes_several_strips(max_columns, strips, g, rt, monkeypatch):
    """24 + 4 + 40 columns do not fit 64, 40 + 4 + 17 do: [24] [40, 17]; at 48 no two lines share a strip"""
    from univer_ocr_amd.nn.ops import pack_layout
    CP, runtime = rt
    assert len(pack_layout([24, 40, 17], max_columns=max_columns)) == strips
    system, _, context = char_system(g, CP, max_columns=max_columns)
    calls = recorded(runtime, monkeypatch)
    system.predict(context)
    monkeypatch.undo()
    check_page(g, CP, context)
    assert calls.count('uocr_pack_lines') == strips


# ---- 9: the PREDICT system -------------------------------------------------------------------------------------------------
def test_predict_system_page_pass_reads_what_the_line_passes_read(rt):
    from test_gpu_models import set_analytic_weights
    from test_gpu_pred_to_text import planted_lines, planted_paragraphs
    from univer_ocr_amd.my_model.model import PackedLinesComponent, make_divisible_by, make_predict_system
    from univer_ocr_amd.my_model.predict import predict_text
    from univer_ocr_amd.my_model.synthetic import make_page_batch
    from univer_ocr_amd.nn.model_system import RawFunctionComponent
    CP, _ = rt
    page = make_page_batch(1, 64, 96, seed=7)['image']
    framed = make_divisible_by(page, 16, 16).shape
    contexts = {}
    for form in ('line', 'page'):
        system, models, names = make_predict_system(framed, find_rotation=False, char_batching=form)
        assert isinstance(system.components[names.index('Char')], PackedLinesComponent) == (form == 'page')
        for model in models.values():
            set_analytic_weights(model)

        def plant_paragraphs(context):
            context['paragraph_pred'] = CP.copy(planted_paragraphs(framed))

        def plant_lines(context):
            context['line_pred'] = [CP.copy(planted_lines(crop.shape)) for crop in context['cropped_monochrome']]
        system.components.insert(names.index('ParagraphCrop'), RawFunctionComponent(plant_paragraphs))
        system.components.insert(names.index('LineCrop') + 1, RawFunctionComponent(plant_lines))
        contexts[form] = {}
        predict_text(page, system, context=contexts[form])
    line, packed = contexts['line'], contexts['page']
    assert [len(p) for p in packed['char_pred']] == [len(p) for p in line['char_pred']] == [2, 2]
    for p, per_line in enumerate(line['char_pred']):
        for l, ref in enumerate(per_line):
            pred = packed['char_pred'][p][l]
            assert pred.shape == ref.shape == (packed['cropped_2_monochrome'][p][l].shape[2], N_CHARS)
            err = rel_linf(CP.asnumpy(pred), CP.asnumpy(ref))
            print(f'char_pred[{p}][{l}] {pred.shape}: page pass against line pass, rel_linf {err:.2e}')
            assert err < CHAR_BOUND
    assert packed['text'] == line['text'] and [len(p) for p in packed['text']] == [2, 2]


@pytest.mark.parametrize('case', ['no paragraph', 'last paragraph without lines'])
def test_predict_system_page_pass_where_stages_find_nothing(case, rt, monkeypatch):
    from test_gpu_pred_to_text import planted_lines, planted_paragraphs
    from univer_ocr_amd.my_model.model import make_predict_system
    from univer_ocr_amd.nn.model_system import RawFunctionComponent
    CP, runtime = rt
    shape = (1, 80, 112, 1)
    system, _, names = make_predict_system(shape, find_rotation=False, char_batching='page')

    def plant_paragraphs(context):
        context['paragraph_pred'] = CP.copy(np.zeros(shape) if case == 'no paragraph' else planted_paragraphs(shape))

    def plant_lines(context):
        crops = context['cropped_monochrome']
        context['line_pred'] = [CP.copy(planted_lines(crop.shape) * (p == 0)) for p, crop in enumerate(crops)]
    system.components.insert(names.index('ParagraphCrop'), RawFunctionComponent(plant_paragraphs))
    if case != 'no paragraph':
        system.components.insert(names.index('LineCrop') + 1, RawFunctionComponent(plant_lines))
    context = {'monochrome_X': CP.copy(np.random.default_rng(3).random(shape))}
    calls = recorded(runtime, monkeypatch)
    system.predict(context)
    monkeypatch.undo()
    if case == 'no paragraph':
        assert context['cropped_monochrome'] == [] and context['cropped_2_monochrome'] == [] and context['text'] == []
        assert 'line_pred' not in context and 'char_pred' not in context
        assert 'uocr_pack_lines' not in calls and 'uocr_zero_gaps' not in calls and 'Char' not in context['prediction']
    else:
        assert [len(p) for p in context['cropped_2_monochrome']] == [2, 0] and len(context['char_pred']) == 1
        assert [len(p) for p in context['text']] == [2, 0] and all(isinstance(t, str) for t in context['text'][0])
        assert calls.count('uocr_pack_lines') == 1
