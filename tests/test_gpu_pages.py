"""The page generator on the GPU (csrc/page_gen.hip) against the NumPy restatement of its rules (tests/page_rules.py, checked
by tests/test_pages_host.py).  Everything is integer arithmetic and table look-ups, so every comparison is `array_equal`,
in float32, float64 and binary16.  Outputs start as NaN between two sentinel borders (the guard regions of
test_gpu_bounds): every element must be written, and nothing outside."""
import ctypes as C

import numpy as np
import pytest

import page_rules as R
from test_gpu_bounds import GUARD, SENTINEL

pytestmark = pytest.mark.gpu

DTYPES = ('float32', 'float64', 'float16')
TABLE_NAMES = ('paragraphs', 'lines', 'glyphs', 'counts')
ERR_ARG, ERR_DTYPE = -1, -2


@pytest.fixture
def rt():
    from univer_ocr_amd.nn import CP
    CP.use_gpu(0)
    CP.set_dtype('float32')
    return CP, CP.runtime()


@pytest.fixture(scope='module')
def atlas():
    return R.load_atlas()


@pytest.fixture
def device_atlas(rt):
    from univer_ocr_amd.my_model.pages import GlyphAtlas
    return GlyphAtlas.shared()


@pytest.fixture(scope='module')
def generated(atlas):
    """two pages of 256 x 512 from the restatement and their layers in float64, made once"""
    pages = [R.layout_page(atlas, 21, (1 << 32) + 40 + i, 256, 512) for i in range(2)]
    assert all(len(page['lines']) >= 3 for page in pages)
    layers = R.render_pages(atlas, pages, 256, 512, R.make_lut(np.float64))
    for tag in layers:
        layers[tag].setflags(write=False)
    return pages, layers


class Outputs:
    """the five outputs of a render call for n pages, each NaN between two borders of GUARD sentinels, its first element
    `offsets[i]` elements behind the border (an odd offset takes the output off every vector border)"""

    def __init__(self, CP, n, height, width, dtype, offsets=(0, 0, 0, 0, 0)):
        self.CP, self.dtype, self.offsets = CP, np.dtype(dtype), offsets
        self.shapes = [(n, height, width, c) for _, c in R.LAYERS]
        self.buffers = []
        for shape, offset in zip(self.shapes, offsets):
            host = np.full(2 * GUARD + offset + int(np.prod(shape)), SENTINEL, self.dtype)
            host[GUARD + offset:len(host) - GUARD] = np.nan
            self.buffers.append(CP.copy(host, self.dtype))

    def pointers(self):
        return [b.ptr + (GUARD + offset) * self.dtype.itemsize for b, offset in zip(self.buffers, self.offsets)]

    def read(self, written=True):
        """{layer: (n, H, W, C)} after checking the borders; written=False: every element must still be NaN"""
        out = {}
        for (tag, _), shape, offset, buffer in zip(R.LAYERS, self.shapes, self.offsets, self.buffers):
            host = self.CP.asnumpy(buffer)
            assert np.all(host[:GUARD + offset] == self.dtype.type(SENTINEL)), f'{tag}: written in front of the output'
            assert np.all(host[len(host) - GUARD:] == self.dtype.type(SENTINEL)), f'{tag}: written behind the output'
            payload = host[GUARD + offset:len(host) - GUARD]
            assert np.isnan(payload).all() if not written else not np.isnan(payload).any(), \
                f'{tag}: ' + ('touched' if not written else f'{int(np.isnan(payload).sum())} elements not written')
            out[tag] = payload.reshape(shape)
        return out


def upload_tables(CP, packed):
    return {name: CP.copy(packed[name], np.int32) for name in TABLE_NAMES}


def render_args(device_atlas, tables, outputs, n, height, width, dtype):
    """the argument list of uocr_page_render behind the context"""
    from univer_ocr_amd.hip import lib as hiplib
    a = device_atlas.device()
    return [hiplib.dtype_code(dtype), n, height, width, *(tables[name].ptr for name in TABLE_NAMES), a['metrics'].shape[0],
            a['metrics'].ptr, a['adv'].ptr, a['offset'].ptr, a['cells'].ptr, a['cells'].shape[0], device_atlas.lut(dtype).ptr,
            *outputs.pointers()]


def render(rt, device_atlas, pages, height, width, dtype, offsets=(0, 0, 0, 0, 0)):
    CP, runtime = rt
    outputs = Outputs(CP, len(pages), height, width, dtype, offsets)
    tables = upload_tables(CP, R.pack_tables(pages))
    runtime.call('uocr_page_render', *render_args(device_atlas, tables, outputs, len(pages), height, width, dtype))
    return outputs.read()


def assert_layers_equal(got, expected, dtype, what=''):
    for tag, _ in R.LAYERS:
        exp = expected[tag].astype(dtype)
        assert got[tag].dtype == np.dtype(dtype) and got[tag].shape == exp.shape, f'{what}{tag}'
        if not np.array_equal(got[tag], exp):
            where = np.argwhere(got[tag] != exp)
            raise AssertionError(f'{what}{tag} {dtype}: {len(where)} elements differ, the first at {where[0].tolist()}: '
                                 f'{got[tag][tuple(where[0])]} != {exp[tuple(where[0])]}')


# ---- layout --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', [3, 2 ** 64 - 59])
@pytest.mark.parametrize('size,n_pages', [((256, 512), 4), ((64, 128), 24)])
def test_layout_equals_the_rules(size, n_pages, seed, rt, atlas, device_atlas):
    from univer_ocr_amd.nn import ops
    CP, runtime = rt
    height, width = size
    first_page = (1 << 32) + 1234567
    tables = {name: a.numpy() for name, a in ops.page_layout(device_atlas.device(), seed, first_page, n_pages, height, width).items()}
    assert runtime.last_page_gen()[2:] == (256, 1)
    paragraphs = 0
    for i in range(n_pages):
        expected = R.layout_page(atlas, seed, first_page + i, height, width)
        assert tables['counts'][i].tolist() == R.counts_of(expected).tolist(), f'page {i}: counts'
        for name in TABLE_NAMES[:3]:
            assert np.array_equal(tables[name][i, :len(expected[name])], expected[name]), f'page {i}: {name}'
        paragraphs += len(expected['paragraphs'])
    assert paragraphs > 0, 'the pages of the test hold text'


def test_layout_stays_inside_its_tables(rt, atlas, device_atlas):
    """three pages at page numbers past 2^63, every table between two sentinel borders; rows past the counts stay as they were"""
    CP, runtime = rt
    n_pages, height, width, seed, first_page = 3, 256, 512, 17, 2 ** 63 + 5
    sizes = {'paragraphs': R.MAX_PARAGRAPHS * 8, 'lines': R.MAX_LINES * 5, 'glyphs': R.MAX_GLYPHS * 2, 'counts': 4}
    assert GUARD % 4 == 0, 'the tables keep their 16-byte alignment behind the border'
    buffers = {name: CP.copy(np.full(2 * GUARD + n_pages * size, -777, np.int32), np.int32) for name, size in sizes.items()}
    a = device_atlas.device()
    runtime.call('uocr_page_layout', seed, first_page, n_pages, height, width, a['metrics'].shape[0], a['metrics'].ptr, a['adv'].ptr,
                 *(buffers[name].ptr + 4 * GUARD for name in TABLE_NAMES))
    for name, size in sizes.items():
        host = buffers[name].numpy()
        assert np.all(host[:GUARD] == -777) and np.all(host[GUARD + n_pages * size:] == -777), f'{name}: written outside the table'
        table = host[GUARD:GUARD + n_pages * size].reshape(n_pages, -1)
        for i in range(n_pages):
            expected = R.layout_page(atlas, seed, first_page + i, height, width)
            rows = (R.counts_of(expected) if name == 'counts' else expected[name]).reshape(-1)
            assert np.array_equal(table[i, :len(rows)], rows), f'{name} of page {i}'
            assert np.all(table[i, len(rows):] == -777), f'{name} of page {i}: rows past the counts were written'


# ---- render ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_render_equals_the_rules_on_generated_pages(dtype, rt, atlas, device_atlas, generated):
    pages, layers = generated
    expected = layers if dtype == 'float64' else R.render_pages(atlas, pages, 256, 512, R.make_lut(dtype))
    assert_layers_equal(render(rt, device_atlas, pages, 256, 512, dtype), expected, dtype)


def hand_pages(atlas, height, width, tile_h, tile_w):
    """the hand-built pages of one call, face 0 (15 rows high): one paragraph lines only -- two lines take 36 rows"""
    adv = atlas['adv'][0]
    narrow, wide = int(np.argmin(adv[1:])) + 1, int(np.argmax(adv))
    cell_h = int(atlas['metrics'][0, R.HEIGHT])
    width_of = lambda ids: int(adv[ids].sum())
    text = [78, 79, 1, 80]
    assert tile_h >= cell_h + 1 and tile_w >= width_of(text) and height >= tile_h + cell_h and width >= tile_w + width_of(text)
    return [
        # a box that ends on the tile border in both directions, one that starts on it, one across it
        R.hand_page(atlas, [(tile_w - width_of(text), tile_h - cell_h, 0, [text]), (tile_w, tile_h, 0, [text])]),
        R.hand_page(atlas, [(tile_w - width_of(text) // 2, tile_h - cell_h // 2, 0, [text])]),
        # the last rows and columns of the page; the first ones
        R.hand_page(atlas, [(width - width_of(text), height - cell_h, 0, [text]), (0, 0, 0, [[wide]])]),
        # a one-glyph line; the narrowest cell next to itself; adjacent equal characters
        R.hand_page(atlas, [(3, 1, 0, [[narrow]]), (20, 16, 0, [[narrow, narrow, narrow, 90, 90]])]),
        # an empty page
        R.hand_page(atlas, []),
        # a bold face with a wider cell
        R.hand_page(atlas, [(5, 7, 4, [[104, 161, 2]])]),
    ]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('width,offsets', [(64, (0, 0, 0, 0, 0)), (61, (1, 3, 5, 7, 1)), (64, (3, 1, 7, 1, 5))])
def test_render_hand_built_tables(width, offsets, dtype, rt, atlas, device_atlas):
    _, runtime = rt
    render(rt, device_atlas, [R.hand_page(atlas, [])], 32, width, dtype)
    tile_h, tile_w, per_launch, launches = runtime.last_page_gen()
    assert launches == 1 and 32 % tile_h == 0 and tile_h < 32 and tile_w < width, 'a 32-row page has more than one tile'
    pages = hand_pages(atlas, 32, width, tile_h, tile_w)
    got = render(rt, device_atlas, pages, 32, width, dtype, offsets)
    assert_layers_equal(got, R.render_pages(atlas, pages, 32, width, R.make_lut(dtype)), dtype)
    assert got['monochrome'][:4].max() > 0.9 and got['char'][:4, :, :, 8].max() == 1, 'ink and spacing were drawn'
    assert got['paragraph'][4].max() == 0 and got['image'][4].min() == 1, 'the empty page is white'


@pytest.mark.parametrize('dtype', DTYPES)
def test_render_past_one_launch_group(dtype, rt, atlas, device_atlas):
    _, runtime = rt
    render(rt, device_atlas, [R.hand_page(atlas, [])], 32, 64, dtype)
    tile_h, tile_w, per_launch, _ = runtime.last_page_gen()
    kinds = hand_pages(atlas, 32, 64, tile_h, tile_w)
    order = [(3 * i + i // 7) % len(kinds) for i in range(per_launch + 3)]
    got = render(rt, device_atlas, [kinds[k] for k in order], 32, 64, dtype)
    assert runtime.last_page_gen() == (tile_h, tile_w, per_launch, 2)
    expected = R.render_pages(atlas, kinds, 32, 64, R.make_lut(dtype))
    assert_layers_equal(got, {tag: expected[tag][order] for tag in expected}, dtype)


def test_tables_that_hold_anything_are_only_read(rt, atlas, device_atlas):
    """counts, faces, line and glyph indices far outside their tables: pixels without a line or a glyph, all written"""
    page = R.hand_page(atlas, [(2, 1, 0, [[78, 79]]), (30, 2, 0, [[80]]), (2, 17, 0, [[81]]), (40, 17, 0, [[82]])])
    packed = R.pack_tables([page])
    packed['counts'][0] = [2 ** 30, -5, 7, 0]
    packed['paragraphs'][0, 0, 4] = 2 ** 30                 # a face that does not exist: the last one is taken
    packed['paragraphs'][0, 1, 6] = 2 ** 31 - 1             # first_line outside the table
    packed['lines'][0, 2, 3:5] = [2 ** 31 - 1, 2 ** 31 - 1]  # glyphs outside the table
    packed['glyphs'][0, 4, 1] = 2 ** 30                     # the glyph of the fourth paragraph: an id that is none
    CP, runtime = rt
    outputs = Outputs(CP, 1, 32, 64, 'float32')
    runtime.call('uocr_page_render', *render_args(device_atlas, upload_tables(CP, packed), outputs, 1, 32, 64, 'float32'))
    got = outputs.read()
    assert np.array_equal(got['paragraph'], R.render_pages(atlas, [page], 32, 64, R.make_lut('float32'))['paragraph'])
    assert got['char'][0, :, 30:].max() == 0 and got['monochrome'][0, :, 30:].max() == 0


# ---- errors ----------------------------------------------------------------------------------------------------------------
def test_errors_return_their_code_and_write_nothing(rt, atlas, device_atlas):
    CP, runtime = rt
    page = R.hand_page(atlas, [(3, 1, 0, [[78]])])
    tables = upload_tables(CP, R.pack_tables([page]))
    outputs = Outputs(CP, 1, 32, 64, 'float32')
    good = render_args(device_atlas, tables, outputs, 1, 32, 64, 'float32')
    fn = runtime.lib.uocr_page_render

    def code(index, value):
        args = list(good)
        args[index] = value
        return fn(runtime.ctx, *args)

    pointers = [4, 5, 6, 7, 9, 10, 11, 12, 14, 15, 16, 17, 18, 19]
    for index in pointers:
        assert code(index, None) == ERR_ARG, f'argument {index} null'
    assert fn(None, *good) == ERR_ARG
    assert code(0, 7) == ERR_DTYPE
    for index, value in ((1, -1), (2, 0), (3, 0), (2, 2 ** 24 + 1), (8, 0), (8, 257), (13, -1)):
        assert code(index, value) == ERR_ARG, f'argument {index} = {value}'
    for index in range(14, 20):
        assert code(index, good[index] + 2) == ERR_ARG, f'argument {index} off its alignment'
    before = runtime.last_page_gen()
    assert code(1, 0) == 0 and runtime.last_page_gen() == before, 'no page: nothing is launched'
    assert fn(runtime.ctx, good[0], 0, 32, 64, *[None] * 4, 0, *[None] * 4, 0, *[None] * 6) == 0
    runtime.synchronize()
    outputs.read(written=False)
    # the layout call
    a = device_atlas.device()
    layout = runtime.lib.uocr_page_layout
    good = [5, 1 << 40, 1, 32, 64, 16, a['metrics'].ptr, a['adv'].ptr, *(tables[name].ptr for name in TABLE_NAMES)]
    held = {name: tables[name].numpy() for name in TABLE_NAMES}
    for index in range(6, 12):
        assert layout(runtime.ctx, *good[:index], None, *good[index + 1:]) == ERR_ARG
    for index, value in ((2, -1), (3, 0), (4, 0), (5, 0), (5, 257), (8, good[8] + 4), (11, good[11] + 4)):
        assert layout(runtime.ctx, *good[:index], value, *good[index + 1:]) == ERR_ARG, f'argument {index} = {value}'
    assert layout(None, *good) == ERR_ARG and layout(runtime.ctx, 5, 0, 0, 32, 64, 16, *[None] * 6) == 0
    runtime.synchronize()
    for name in TABLE_NAMES:
        assert np.array_equal(tables[name].numpy(), held[name]), name
    assert runtime.lib.uocr_ctx_last_page_gen(None, *[None] * 4) == -1


def test_the_report_of_a_new_context_is_zero_and_null_pointers_are_refused():
    """what tests/test_gpu_launch_reports.py asks of the per-launcher getters, for uocr_ctx_last_page_gen"""
    from univer_ocr_amd.hip import lib as hiplib
    lib = hiplib.get_lib()
    handle = C.c_void_p()
    assert lib.uocr_ctx_create(0, 0, C.byref(handle)) == 0
    try:
        outs = [C.c_int(-1) for _ in range(4)]
        assert lib.uocr_ctx_last_page_gen(handle, *[C.byref(out) for out in outs]) == 0
        assert [out.value for out in outs] == [0, 0, 0, 0]
        for null in range(4):
            outs = [C.c_int(-1) for _ in range(4)]
            args = [None if k == null else C.byref(out) for k, out in enumerate(outs)]
            assert lib.uocr_ctx_last_page_gen(handle, *args) == ERR_ARG, f'null pointer {null} was accepted'
            assert all(out.value == -1 for out in outs), f'wrote before refusing null pointer {null}'
    finally:
        lib.uocr_ctx_destroy(handle)


# ---- determinism and capture ---------------------------------------------------------------------------------------------
def test_two_calls_and_a_replayed_capture_give_equal_bytes(rt, atlas, device_atlas):
    import torch
    from univer_ocr_amd.nn import ops
    CP, runtime = rt
    device, lut = device_atlas.device(), device_atlas.lut('float32')
    first = ops.page_render(device, ops.page_layout(device, 9, 1 << 35, 2, 256, 512), 256, 512, lut)
    again = ops.page_render(device, ops.page_layout(device, 9, 1 << 35, 2, 256, 512), 256, 512, lut)
    first = {tag: a.numpy() for tag, a in first.items()}
    for tag in first:
        assert first[tag].tobytes() == again[tag].numpy().tobytes(), tag
    with runtime.capture(torch.cuda.MemPool()) as graph:
        captured = ops.page_render(device, ops.page_layout(device, 9, 1 << 35, 2, 256, 512), 256, 512, lut)
    for _ in range(2):
        for a in captured.values():
            a.t.fill_(float('nan'))
        graph.replay()
        for tag in first:
            assert first[tag].tobytes() == captured[tag].numpy().tobytes(), tag
    assert first['monochrome'].max() > 0.9


# ---- GeneratedPages ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_generated_pages_are_a_function_of_seed_and_index(dtype, rt, atlas):
    from univer_ocr_amd.my_model.crop import CHARS
    from univer_ocr_amd.my_model.pages import LAYER_TAGS, GeneratedPages, PagesWithText
    CP, _ = rt
    source = GeneratedPages(2, 96, 384, seed=77, length=3, dtype=dtype)
    assert len(source) == 3 and LAYER_TAGS == tuple(tag for tag, _ in R.LAYERS)
    batches = [{tag: a.numpy() for tag, a in source.get(index).items()} for index in (0, 1, 0, 2 ** 40)]
    expected = [[R.layout_page(atlas, 77, 2 * index + i, 96, 384) for i in range(2)] for index in (0, 1)]
    for got, pages in zip(batches, expected):
        assert_layers_equal(got, R.render_pages(atlas, pages, 96, 384, R.make_lut(dtype)), dtype)
    assert all(np.array_equal(batches[0][tag], batches[2][tag]) for tag in LAYER_TAGS), 'the same batch again'
    assert not np.array_equal(batches[0]['image'], batches[1]['image']) and not np.array_equal(batches[0]['image'], batches[3]['image'])
    assert not np.array_equal(batches[0]['image'][0], batches[0]['image'][1]), 'the pages of a batch differ'
    other = GeneratedPages(2, 96, 384, seed=78, dtype=dtype).get(0, ['image', 'char'])
    assert sorted(other) == ['char', 'image'] and not np.array_equal(other['image'].numpy(), batches[0]['image'])
    assert source.texts(1) == [R.texts(page, CHARS) for page in expected[1]]
    # the pages with text, one at a time: made alone, the bytes they have in their batch
    alone = PagesWithText(source, 3)
    for i in range(3):
        number = alone.page_of(i)
        assert number == i, 'every one of these pages holds text'
        one = alone.get(i, ['image', 'char'])
        assert sorted(one) == ['char', 'image'] and one['char'].shape == (1, 96, 384, 9)
        for tag in one:
            assert np.array_equal(one[tag].numpy()[0], batches[number // 2][tag][number % 2]), tag
        assert alone.texts(i) == R.texts(expected[number // 2][number % 2], CHARS)
    assert sum(len(paragraph) for page in source.texts(1) for paragraph in page) > 0


# ---- the device stages read what was typed ---------------------------------------------------------------------------------
def collapse(ids):
    """runs of equal ids between zeros, one id per run"""
    out, last = [], 0
    for i in ids:
        if i != 0 and i != last:
            out.append(i)
        last = i
    return out


def test_device_stages_read_a_generated_page_as_typed_and_the_char_net_steps(rt):
    from univer_ocr_amd.my_model.crop import CHARS
    from univer_ocr_amd.my_model.model import BITS_COUNT, N_CHARS, make_train_char_context_maker, make_train_char_system
    from univer_ocr_amd.my_model.pages import GeneratedPages, PagesWithText
    from univer_ocr_amd.nn import ops
    from univer_ocr_amd.nn.optimizers import Momentum
    CP, _ = rt
    np.random.seed(0)
    source = GeneratedPages(1, 256, 512, seed=31, length=1)
    pages = PagesWithText(source, 1)
    system, models, names = make_train_char_system((1, 32, 64, 1), Momentum(lr=0.001, momentum=0))
    assert names == ['ParagraphCrop', 'LineCrop', 'CharLabel', 'Char']
    context = make_train_char_context_maker()(pages.get, (0,))
    system.train(context)
    boxes = source.tables(None, first_page=pages.page_of(0), n_pages=1)['paragraphs'].numpy()[0]
    typed = pages.texts(0)
    reading_order = sorted(range(len(typed)), key=lambda p: (boxes[p, 1], boxes[p, 0]))       # the order of the labelling
    assert len(typed) >= 2 and [len(p) for p in context['cropped_2_char']] == [len(typed[p]) for p in reading_order]
    flat = [line for paragraph in context['cropped_2_char'] for line in paragraph]
    _, ids = ops.char_label(flat, BITS_COUNT, N_CHARS, want_ids=True)
    read = [''.join(CHARS[i] for i in collapse(a.numpy().tolist())) for a in ids]
    assert read == [line for p in reading_order for line in typed[p]]
    labels = [a.numpy() for paragraph in context['char_labels'] for a in paragraph]
    assert all(np.array_equal(np.argmax(label, axis=1), i.numpy()) for label, i in zip(labels, ids))
    losses = [float(v) for v in context['losses']['Char']['output_losses']]
    assert len(losses) == len(flat) and np.isfinite(losses).all() and all(v > 0 for v in losses)


def test_train_model_on_generated_pages(rt, tmp_path, monkeypatch):
    import json

    from univer_ocr_amd.my_model import train as train_mod
    path = tmp_path / 'model_weights.json'
    monkeypatch.setattr(train_mod, 'MODEL_WEIGHTS_FILE_PATH', path)
    monkeypatch.setattr(train_mod.load_weights, '__defaults__', (path,))      # every stage resumes from the stage before
    np.random.seed(0)
    results = train_mod.train_model(True, epochs_scale=0.011, batch=1, height=64, width=256, data='generated')
    assert list(results) == ['TRAIN_MONOCHROME', 'TRAIN_PARAGRAPH', 'TRAIN_LINE', 'TRAIN_CHAR']
    for stage, (best, _) in results.items():
        assert all(np.isfinite(v).all() for v in best.values()), stage
    weights = json.loads(path.read_text())
    assert {'Monochrome/conv_1', 'Char/dense_block/dense_3'} <= set(weights)
    assert {name.split('/')[0] for name in weights} == {'Monochrome', 'Paragraph', 'Line', 'Char'}
    assert all(np.isfinite(np.array(v)).all() for layer in weights.values() for v in layer.values())
