"""Line crops on the GPU (csrc/line_crop.hip) against the reference's CropRotateAndZoomLines results in
tests/golden/line_crop.npz and, at sizes derived from the kernel's own block and launch sizes, against the NumPy
restatement that tests/test_line_crop_host.py pins to that fixture and to scipy.  The stage is an index map from output
element to source element or zero, and every input is a multiple of 1/64 -- the same number in binary16, float32 and
float64 -- so every comparison is for equality (`array_equal`, no tolerance).  Sources are NaN outside the box and
outputs start as NaN: a NaN in a result is a read outside the box or an element that was not written.  The TRAIN_CHAR
model system runs against the reference's Char net with the tolerances of tests/test_gpu_label.py."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden, rel_linf
from test_gpu_char_label import Packed
from test_gpu_label import SYSTEM_TOL
from test_line_crop_host import (LINES_OF_THE_PAGE, MINIMAL_WIDTH, ROTATIONS, STAGE_NAMES, ZOOMED_HEIGHT, f64, gather_cases,
                                 line_crop_rules, stage_lines)

pytestmark = pytest.mark.gpu

DTYPES = ('float32', 'float64', 'float16')
NAMES = ('src', 'src_h', 'src_w', 'c', 'y0', 'x0', 'box_h', 'box_w', 'quarter_turns', 'zoom_h', 'zoom_w', 'out', 'out_w')


@pytest.fixture(scope='module')
def g():
    return load_golden('line_crop')


@pytest.fixture
def rt():
    from univer_ocr_amd.nn import CP
    CP.use_gpu(0)
    CP.set_dtype('float32')
    return CP, CP.runtime()


def raw_call(runtime, dtype, n_entries=None, **arrays):
    """uocr_line_crop on lists (device addresses for src / out; None = a null entry, a list given as None = a null array);
    dtype: a NumPy dtype name, or the ABI's integer code as it is"""
    from univer_ocr_amd.hip import lib as hiplib
    n = len(arrays['src_h']) if n_entries is None else n_entries
    pointers = lambda values: None if values is None else (C.c_void_p * len(values))(*values)
    ints = lambda values: None if values is None else (C.c_int * len(values))(*values)
    runtime.call('uocr_line_crop', dtype if isinstance(dtype, int) else hiplib.dtype_code(dtype), n,
                 *[(pointers if name in ('src', 'out') else ints)(arrays[name]) for name in NAMES])


def only_the_box(image, y0, x0, bh, bw):
    """the image with NaN everywhere outside the box"""
    out = np.full(image.shape, np.nan)
    out[:, y0:y0 + bh, x0:x0 + bw] = image[:, y0:y0 + bh, x0:x0 + bw]
    return out


def sizes_of(entry, zoomed_height=ZOOMED_HEIGHT, minimal_width=MINIMAL_WIDTH):
    from univer_ocr_amd.nn.ops import line_crop_shape
    _, _, _, bh, bw, turns = entry
    return line_crop_shape(bh, bw, turns, zoomed_height, minimal_width)


def arguments(entries, dev, outs, shapes):
    return dict(src=[a.ptr for a in dev], src_h=[e[0].shape[1] for e in entries], src_w=[e[0].shape[2] for e in entries],
                c=[e[0].shape[3] for e in entries], y0=[e[1] for e in entries], x0=[e[2] for e in entries],
                box_h=[e[3] for e in entries], box_w=[e[4] for e in entries], quarter_turns=[e[5] for e in entries],
                zoom_h=[s[0] for s in shapes], zoom_w=[s[1] for s in shapes], out=[a.ptr for a in outs],
                out_w=[s[2] for s in shapes])


def crop_entries(rt, entries, dtype='float32', zoomed_height=ZOOMED_HEIGHT, minimal_width=MINIMAL_WIDTH):
    """ONE uocr_line_crop call on entries (host image (1, H, W, C), y0, x0, box_h, box_w, quarter_turns); every source is
    NaN outside its box and every output starts as NaN -> the outputs on the host"""
    CP, runtime = rt
    dev = [CP.copy(only_the_box(*e[:5]), dtype) for e in entries]
    shapes = [sizes_of(e, zoomed_height, minimal_width) for e in entries]
    outs = [CP.copy(np.full((1, zh, ow, e[0].shape[3]), np.nan), dtype) for e, (zh, _, ow) in zip(entries, shapes)]
    raw_call(runtime, dtype, **arguments(entries, dev, outs, shapes))
    return [CP.asnumpy(a) for a in outs]


def check_entries(rt, entries, dtype='float32', expected=None, what='', **sizes):
    got = crop_entries(rt, entries, dtype, **sizes)
    for i, (e, out) in enumerate(zip(entries, got)):
        exp = expected[i] if expected is not None else line_crop_rules(e[0], *e[1:5], 90 * e[5], **sizes)
        where = f'{what} entry {i}: box {e[3]} x {e[4]} at ({e[1]}, {e[2]}) of {e[0].shape}, {e[5]} turns, {dtype}'
        assert out.dtype == np.dtype(dtype) and out.shape == exp.shape, f'{where}: {out.shape} != {exp.shape}'
        assert not np.isnan(out).any(), f'{where}: read outside the box or left elements unwritten at {np.argwhere(np.isnan(out))[:4].tolist()}'
        assert np.array_equal(out, exp.astype(dtype)), f'{where}: differs at {np.argwhere(out != exp.astype(dtype))[:4].tolist()}'
    return got


def random_image(rng, h, w, c):
    return rng.integers(1, 65, (1, h, w, c)) / 64.0


@pytest.fixture
def sizes(rt):
    """(output elements per block, bytes per vector store, entries per launch) of the library"""
    check_entries(rt, [(random_image(np.random.default_rng(0), 6, 7, 2), 1, 2, 3, 4, 1)])
    chunk, store_bytes, per_launch, launches = rt[1].last_line_crop()
    assert chunk >= 64 and chunk % 32 == 0 and store_bytes == 16 and per_launch > 1 and launches == 1
    return chunk, store_bytes, per_launch


# ---- fixture (a): the reference's crops ------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_gather_cases_equal_the_reference(dtype, g, rt):
    """every box, channel count and rotation of the fixture in ONE call"""
    cases = list(gather_cases(g))
    entries = [(image, *box, rotation // 90) for _, _, rotation, image, box, _ in cases]
    check_entries(rt, entries, dtype, expected=[expected for *_, expected in cases], what='golden')
    per_launch = rt[1].last_line_crop()[2]
    assert rt[1].last_line_crop()[3] == -(-len(entries) // per_launch)


def test_python_wrapper_allocates_and_returns_device_arrays(g, rt):
    from univer_ocr_amd.nn import ops
    CP, _ = rt
    cases = [case for case in gather_cases(g) if case[0] in (2, 3, 6, 7)]
    for dtype in DTYPES:
        images, entries = {}, []
        for _, c, rotation, image, box, _ in cases:
            if (c, image.shape) not in images:
                images[c, image.shape] = CP.copy(image, dtype)
            entries.append((images[c, image.shape], *box, rotation // 90))
        outs = ops.line_crop(entries)
        assert len(outs) == len(cases)
        for out, (case, c, rotation, _, box, expected) in zip(outs, cases):
            assert out.dtype == np.dtype(dtype) and out.shape == expected.shape
            assert np.array_equal(CP.asnumpy(out), expected.astype(dtype)), f'case {case} c={c} rotation {rotation}'
        empty = ops.line_crop([(entries[0][0], 1, 1, 64, 1, 0), entries[0]], minimal_width=None)    # zoomed to 32 x 0
        assert empty[0].shape == (1, ZOOMED_HEIGHT, 0, entries[0][0].shape[3])
        assert np.array_equal(CP.asnumpy(empty[1])[:, :, :5], cases[0][5].astype(dtype)[:, :, :5])
        small = ops.line_crop(entries[:3], zoomed_height=None, minimal_width=None)
        for out, (_, _, rotation, image, box, _) in zip(small, cases[:3]):
            assert np.array_equal(CP.asnumpy(out), np.rot90(image[:, box[0]:box[0] + box[2], box[1]:box[1] + box[3]],
                                                             rotation // 90, axes=(1, 2)).astype(dtype))


# ---- sizes derived from the library's own ----------------------------------------------------------------------------------
_EXPECTED = {}


def entries_around_the_block(chunk):
    """widths of one column less than a block, exactly a block and one column more (32 x edge x 1 elements are one
    block); boxes whose height is that number; each at all four turns, with 1, 2 and 9 channels; expected values once"""
    if chunk not in _EXPECTED:
        rng = np.random.default_rng(50)
        edge = chunk // ZOOMED_HEIGHT
        entries = []
        for c in (1, 2, 9):
            for w in (edge - 1, edge, edge + 1):
                image, tall = random_image(rng, 40, w + 5, c), random_image(rng, w + 4, 26, c)
                for turns in range(4):
                    entries.append((image, 3, 2, 32, w, turns))    # zf = 1 when upright: 32 x w x c outputs
                    entries.append((tall, 1, 3, w, 20, turns))
        _EXPECTED[chunk] = entries, [line_crop_rules(e[0], *e[1:5], 90 * e[5]) for e in entries]
    return _EXPECTED[chunk]


@pytest.mark.parametrize('dtype', DTYPES)
def test_sizes_around_the_block(dtype, sizes, rt):
    """72 entries around the block size mixed in ONE call, then other zoomed heights and minimal widths"""
    chunk = sizes[0]
    rng = np.random.default_rng(56)
    entries, expected = entries_around_the_block(chunk)
    check_entries(rt, entries, dtype, expected=expected, what='around the block')
    # other zoomed heights and minimal widths, among them outputs of chunk - 1, chunk and chunk + 1 elements exactly
    for zoomed_height, minimal_width, box in ((1, chunk - 1, (5, 9)), (1, chunk, (9, 5)), (1, chunk + 1, (3, 3)), (7, 3, (29, 11)),
                                              (64, 8, (20, 33))):
        image = random_image(rng, box[0] + 3, box[1] + 4, 1)
        check_entries(rt, [(image, 2, 1, *box, turns) for turns in range(4)], dtype, what=f'zoomed height {zoomed_height}',
                      zoomed_height=zoomed_height, minimal_width=minimal_width)


def mixed_entries(rng, count):
    shapes = [(32, 40), (5, 8), (33, 31), (64, 10), (64, 1), (12, 70), (1, 1), (32, 3), (17, 129)]
    entries = []
    for i in range(count):
        bh, bw = shapes[i % len(shapes)]
        entries.append((random_image(rng, bh + 3, bw + 5, (1, 9, 2, 3)[i % 4]), i % 3, i % 5, bh, bw, (i + i // 4) % 4))
    return entries


def test_more_entries_than_one_launch_takes(sizes, rt):
    """the second launch starts its blocks over: every entry must come out by ITS descriptor"""
    _, _, per_launch = sizes
    entries = mixed_entries(np.random.default_rng(51), per_launch + 1)
    expected = [line_crop_rules(e[0], *e[1:5], 90 * e[5]) for e in entries]
    check_entries(rt, entries, expected=expected, what='many')
    assert rt[1].last_line_crop()[3] == 2, 'two launches'
    check_entries(rt, entries[:per_launch], expected=expected[:per_launch], what='exactly one launch')
    assert rt[1].last_line_crop()[3] == 1
    check_entries(rt, entries[-1:] + entries[:per_launch], 'float16', expected=expected[-1:] + expected[:per_launch], what='float16')


def test_second_call_after_a_larger_one_and_repeatability(sizes, rt):
    chunk = sizes[0]
    rng = np.random.default_rng(52)
    big = [(random_image(rng, 40, 3 * chunk // 32 + 9, 9), 2, 3, 32, 3 * chunk // 32 + 1, turns) for turns in (0, 2)]
    big += mixed_entries(rng, 7)
    small = [(random_image(rng, 9, 12, 9), 1, 1, 5, 8, 3)]
    first = check_entries(rt, big, what='big')
    check_entries(rt, small, what='small after big')
    again = crop_entries(rt, big)
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()


def test_capture_and_replay(sizes, rt):
    """the call is asynchronous and capturable: a replayed graph crops what the source buffers hold then"""
    import torch
    CP, runtime = rt
    rng = np.random.default_rng(53)
    boxes = [(40, 150, 9, 3, 2, 32, 140, 0), (70, 20, 1, 2, 4, 64, 10, 1), (12, 30, 9, 1, 1, 5, 8, 3)]
    versions = [[random_image(rng, h, w, c) for h, w, c, *_ in boxes] for _ in range(2)]
    entries = [(versions[0][i], *box[3:]) for i, box in enumerate(boxes)]
    shapes = [sizes_of(e) for e in entries]
    dev = [CP.copy(x, np.float32) for x in versions[0]]
    outs = [CP.zeros((1, zh, ow, e[0].shape[3]), np.float32) for e, (zh, _, ow) in zip(entries, shapes)]
    with runtime.capture(torch.cuda.MemPool()) as graph:
        raw_call(runtime, 'float32', **arguments(entries, dev, outs, shapes))
    for images in versions[::-1] + versions:
        for a, x in zip(dev, images):
            a.set(x)
        graph.replay()
        for i, (x, box) in enumerate(zip(images, boxes)):
            assert np.array_equal(CP.asnumpy(outs[i]), line_crop_rules(x, *box[3:7], 90 * box[7]).astype(np.float32)), f'entry {i}'


# ---- bounds --------------------------------------------------------------------------------------------------------------------
def test_everything_stays_inside_its_buffers(sizes, rt):
    """sources and outputs of every entry sit between sentinel borders, off 16-byte alignment (the scalar heads and tails
    of the 16-byte stores), at ragged sizes; boxes touch the borders of their sources"""
    CP, runtime = rt
    chunk = sizes[0]
    rng = np.random.default_rng(54)
    edge = chunk // ZOOMED_HEIGHT
    made = [(34, edge + 2, 1, 0, 0, 32, edge + 1, 0), (32, edge + 1, 1, 0, 2, 32, edge - 1, 2), (64, 10, 9, 0, 0, 64, 10, 1),
            (5, 8, 9, 0, 0, 5, 8, 3), (70, 3, 2, 6, 2, 64, 1, 0), (33, 31, 3, 0, 0, 33, 31, 0), (1, 1, 1, 0, 0, 1, 1, 1),
            (40, 9, 1, 8, 6, 32, 3, 2), (19, 141, 9, 2, 12, 17, 129, 3)]
    entries = [(random_image(rng, h, w, c), *rest) for h, w, c, *rest in made]
    shapes = [sizes_of(e) for e in entries]
    src = Packed(CP, [e[0].size for e in entries])
    out = Packed(CP, [zh * ow * e[0].shape[3] for e, (zh, _, ow) in zip(entries, shapes)])
    assert any(4 * at % 16 for at, _ in out.offsets) and any(4 * (at + n) % 16 for at, n in out.offsets)
    args = arguments(entries, [], [], shapes)
    args['src'], args['out'] = src.upload([only_the_box(*e[:5]) for e in entries]), out.upload()
    raw_call(runtime, 'float32', **args)
    got = out.check('out')
    src.check('src', expect_written=False)
    for i, (e, (zh, _, ow)) in enumerate(zip(entries, shapes)):
        exp = line_crop_rules(e[0], *e[1:5], 90 * e[5]).astype(np.float32)
        assert np.array_equal(got[i].reshape(exp.shape), exp), f'entry {i}'


# ---- arguments -----------------------------------------------------------------------------------------------------------------
def test_argument_errors_write_nothing(rt):
    from univer_ocr_amd.hip import HipError
    CP, runtime = rt
    h, w, c = 12, 20, 3
    src = [CP.copy(random_image(np.random.default_rng(55), h, w, c), np.float32) for _ in range(2)]
    outs = [CP.copy(np.full((1, 32, 64, c), np.nan), np.float32) for _ in range(2)]
    good = dict(src=[a.ptr for a in src], src_h=[h, h], src_w=[w, w], c=[c, c], y0=[1, 2], x0=[2, 1], box_h=[8, 10],
                box_w=[16, 5], quarter_turns=[0, 1], zoom_h=[32, 32], zoom_w=[64, 64], out=[a.ptr for a in outs],
                out_w=[64, 64], n_entries=2)
    bad = [dict({name: None}) for name in NAMES] + [
        dict(n_entries=-1), dict(src=[src[0].ptr, None]), dict(out=[None, outs[1].ptr]), dict(src=[src[0].ptr, src[1].ptr + 2]),
        dict(out=[outs[0].ptr + 2, outs[1].ptr]), dict(c=[c, 0]), dict(src_h=[h, 0]), dict(src_w=[0, w]),
        dict(y0=[1, -1]), dict(x0=[-1, 1]), dict(y0=[5, 2]), dict(x0=[2, 16]), dict(box_h=[8, 11]), dict(box_w=[19, 5]),
        dict(box_h=[0, 10]), dict(box_w=[16, 0]), dict(box_h=[8, -3]), dict(quarter_turns=[0, 4]), dict(quarter_turns=[-1, 1]),
        dict(zoom_h=[32, 0]), dict(zoom_w=[64, -1]), dict(out_w=[63, 64]), dict(zoom_w=[65, 64])]
    for change in bad:
        with pytest.raises(HipError, match=r'\(-1\)'):
            raw_call(runtime, 'float32', **dict(good, **change))
        for a in outs:
            assert np.isnan(CP.asnumpy(a)).all(), f'{change}: an output was touched'
    with pytest.raises(HipError, match=r'\(-2\)'):
        raw_call(runtime, 7, **good)
    assert all(np.isnan(CP.asnumpy(a)).all() for a in outs)
    before = runtime.last_line_crop()
    raw_call(runtime, 'float32', **dict(good, n_entries=0))      # nothing to do: OK, no launch
    raw_call(runtime, 'float32', n_entries=0, **{name: None for name in NAMES})   # ... whatever else is passed
    assert all(np.isnan(CP.asnumpy(a)).all() for a in outs) and runtime.last_line_crop() == before
    raw_call(runtime, 'float32', **dict(good, zoom_w=[0, 64], out_w=[0, 64]))   # an output without elements is no error
    assert np.isnan(CP.asnumpy(outs[0])).all() and not np.isnan(CP.asnumpy(outs[1])).any()


# ---- fixture (b): CropLines --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_crop_lines_equals_the_reference_on_the_stage_cases(dtype, g, rt):
    """all four paragraphs as ONE page: rotation, line order, shapes and arrays of both companions"""
    from univer_ocr_amd.my_model.crop import CropLines
    CP, runtime = rt
    masks = [CP.copy(f64(g[f'stage/{name}/mask']), dtype) for name in STAGE_NAMES]
    arrays = [[CP.copy(f64(g[f'stage/{name}/img{c}']), dtype) for name in STAGE_NAMES] for c in (1, 9)]
    crop_lines = CropLines()
    found = crop_lines.find_lines(masks)
    for name, (rotation, boxes) in zip(STAGE_NAMES, found):
        assert (rotation or 0) == int(g[f'stage/{name}/rotation']), name
        assert np.array_equal(np.array(boxes), g[f'stage/{name}/boxes']), name
    result = crop_lines(masks, arrays)
    assert runtime.last_line_crop()[3] == 1, 'one launch for the page'
    assert len(result) == 2 and all(len(per_array) == len(STAGE_NAMES) for per_array in result)
    for c, per_array in zip((1, 9), result):
        for name, lines in zip(STAGE_NAMES, per_array):
            expected = stage_lines(g, name, c)
            assert len(lines) == len(expected), name
            for l, (line, exp) in enumerate(zip(lines, expected)):
                got = CP.asnumpy(line)
                assert got.dtype == np.dtype(dtype) and got.shape == exp.shape, f'{name} c={c} line {l}'
                assert np.array_equal(got, exp.astype(dtype)), f'{name} c={c} line {l}'


def test_crop_lines_yields_no_lines_where_the_reference_raises(g, rt):
    """no top component, no bottom component: the paragraph stays empty, its neighbours keep their lines"""
    from univer_ocr_amd.my_model.crop import CropLines
    CP, _ = rt
    mask = f64(g['stage/turned/mask'])
    no_top, no_bottom, flat = mask.copy(), mask.copy(), np.full(mask.shape, 0.5)
    no_top[..., 0], no_bottom[..., 1] = 1 / 64, 0.25
    image = f64(g['stage/turned/img9'])
    result = CropLines()([CP.copy(m) for m in (no_top, mask, no_bottom, flat)], [[CP.copy(image) for _ in range(4)]])
    assert [len(lines) for lines in result[0]] == [0, 2, 0, 0]
    for line, exp in zip(result[0][1], stage_lines(g, 'turned', 9)):
        assert np.array_equal(CP.asnumpy(line), exp.astype(np.float32))
    assert CropLines()([], [[], []]) == [[], []]


# ---- fixture (c): the TRAIN_CHAR model system ------------------------------------------------------------------------------
@pytest.mark.parametrize('opt_tag,dtype', [('sgd', 'float32'), ('sgd', 'float64'), ('adam', 'float64')])
def test_train_char_system_equals_the_reference(opt_tag, dtype, g, rt):
    """[ParagraphCrop, LineCrop, CharLabel, Char] on the page of fixture (c): the cropped lines and the labels equal the
    reference's exactly; losses, char_pred[p][l] and the weights after the three steps (one per line) equal the reference
    Char net's to the tolerances of DESIGN 3.  (Adam in float64 only: float32 Adam weights cannot be held to a normalised
    bound after more than one step.)"""
    from test_gpu_models import check_sampled, set_analytic_weights
    from univer_ocr_amd.my_model.model import make_train_char_context_maker, make_train_char_system
    from univer_ocr_amd.nn.optimizers import Adam, Momentum
    CP, _ = rt
    CP.set_dtype(dtype)
    try:
        opt = Momentum(lr=0.01, momentum=0) if opt_tag == 'sgd' else Adam(lr=0.0015)
        system, models, names = make_train_char_system(g['system/mono0_0'].shape, opt)
        assert names == ['ParagraphCrop', 'LineCrop', 'CharLabel', 'Char']
        char = models['Char']
        set_analytic_weights(char)
        layers = {tag: f64(g[f'system/page/{tag}']) for tag in ('monochrome', 'paragraph', 'line', 'char')}
        context = make_train_char_context_maker()(lambda layer_tags: {tag: layers[tag] for tag in layer_tags})
        system.train(context)
        for key, what in (('cropped_2_monochrome', 'mono'), ('cropped_2_char', 'char'), ('char_labels', 'labels')):
            assert [len(p) for p in context[key]] == [2, 1], key
            for p, l in LINES_OF_THE_PAGE:
                got = CP.asnumpy(context[key][p][l])
                assert got.dtype == np.dtype(dtype) and np.array_equal(got, g[f'system/{what}{p}_{l}'].astype(dtype)), f'{key}[{p}][{l}]'
        tol, weight_tol = SYSTEM_TOL[dtype]
        entry = context['losses']['Char']
        assert len(entry['output_losses']) == 3 and [len(p) for p in context['char_pred']] == [2, 1]
        prefix = f'system/{opt_tag}'
        errs = {'losses': rel_linf(np.array([float(v) for v in entry['output_losses']]), g[f'{prefix}/train/Char/output_losses']),
                'reg': rel_linf(np.array(float(entry['regularization_loss'])), g[f'{prefix}/train/Char/regularization_loss'])}
        for p, l in LINES_OF_THE_PAGE:
            pred, key = CP.asnumpy(context['char_pred'][p][l]), f'{prefix}/train/char_pred{p}_{l}'
            errs[f'pred{p}_{l}'] = (rel_linf(pred, g[key]) if key in g.files
                                    else rel_linf(pred.reshape(-1)[::5], g[key + '@stride5']))
        print(f'{opt_tag}/{dtype}: ' + ', '.join(f'{k} {v:.2e}' for k, v in errs.items()))
        for what, err in errs.items():
            assert err <= tol, f'{what}: rel_linf={err:.3e} > {tol:.1e}'
        werrs = {pn: check_sampled(pn, p.value, g, f'{prefix}/final', weight_tol) for pn, p in char.params().items()}
        print(f'{opt_tag}/{dtype}: weights {max(werrs.values()):.2e} ({max(werrs, key=werrs.get)})')
    finally:
        CP.set_dtype('float32')
