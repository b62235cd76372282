"""The rotation search on the device (csrc/rotate.hip: uocr_rotation_search) against the reference's own traces and
angles in tests/golden/rotation.npz and, at sizes derived from the kernels' band, wave and launch sizes, against the NumPy
restatement `search_rules` that tests/test_rotation_search_host.py pins to that fixture.

Leaves and heights are integers and the device evaluates the geometry of nn/ops.py: search_geometry bit for bit: every
comparison is an equality.  The crops of the stage are compared under the bounds of tests/test_gpu_rotation.py.  Results
start as UNTOUCHED: a value left over is an element that was not written."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden
from test_gpu_rotation import DTYPES, bound, ints
from test_rotation_host import STAGE_PARAGRAPHS, compare_sampled, stage_page
from test_rotation_search_host import NODES, ROUNDS, search_rules, trace_rules

pytestmark = pytest.mark.gpu

UNTOUCHED = -7
BAND, WAVE = 8, 64                                                   # output rows per block, pixels per wave step


@pytest.fixture(scope='module')
def g():
    return load_golden('rotation')


@pytest.fixture
def rt():
    from univer_ocr_amd.nn import CP
    CP.use_gpu(0)
    CP.set_dtype('float32')
    return CP, CP.runtime()


# ---- uocr_rotation_search ------------------------------------------------------------------------------------------------
def workspace_ints(paragraphs):
    from univer_ocr_amd.hip import lib as hiplib
    size = C.c_size_t()
    assert hiplib.get_lib().uocr_rotation_search_workspace(paragraphs, C.byref(size)) == 0 and size.value % 4 == 0
    return size.value // 4


def device_table(CP, eps=1.0):
    from univer_ocr_amd.nn.ops import search_table
    rounds, table = search_table(eps)
    return rounds, CP.copy(np.array(table), np.float64)


def search_arguments(labels_dev, paragraphs, table_dev, rounds=ROUNDS, image_index=0):
    """paragraphs: (label, box (y0, x0, h, w)) -> the arguments of uocr_rotation_search but result and workspace"""
    n, h, w = labels_dev.shape
    return dict(labels=labels_dev.ptr, n=n, h=h, w=w, image_index=image_index, n_paragraphs=len(paragraphs),
                label_id=[k for k, _ in paragraphs], box=[v for _, box in paragraphs for v in box], rounds=rounds,
                table=table_dev.ptr)


def raw_search(runtime, result_ptr, workspace_ptr, labels, n, h, w, image_index, n_paragraphs, label_id, box, rounds, table):
    runtime.call('uocr_rotation_search', labels, n, h, w, image_index, n_paragraphs, ints(label_id), ints(box), rounds, table,
                 result_ptr, workspace_ptr)


def search_of(rt, labels, paragraphs, image_index=0):
    """ONE uocr_rotation_search call on the (H, W) or (N, H, W) labels; result and workspace start as UNTOUCHED"""
    CP, runtime = rt
    labels = labels if labels.ndim == 3 else labels[None]
    labels_dev = CP.copy(labels.astype(np.int32), np.int32)
    rounds, table = device_table(CP)
    result = CP.copy(np.full((len(paragraphs), 1 + 2 * rounds), UNTOUCHED, np.int32), np.int32)
    workspace = CP.copy(np.full((workspace_ints(len(paragraphs)),), UNTOUCHED, np.int32), np.int32)
    raw_search(runtime, result.ptr, workspace.ptr, **search_arguments(labels_dev, paragraphs, table, rounds, image_index))
    return CP.asnumpy(result)


def expected_rows(labels, paragraphs):
    """what the call writes, by the rules: per paragraph the leaf, then height_a, height_b of every round"""
    rows = []
    for k, box in paragraphs:
        leaf, heights = search_rules(labels, k, box)
        rows.append([leaf] + heights.reshape(-1).tolist())
    return np.array(rows, np.int32).reshape(len(paragraphs), 1 + 2 * ROUNDS)


def check_search(rt, labels, paragraphs, what, image_index=0, expected=None):
    got = search_of(rt, labels, paragraphs, image_index)
    expected = expected_rows(labels if labels.ndim == 2 else labels[image_index], paragraphs) if expected is None else expected
    for i, (k, box) in enumerate(paragraphs):
        assert got[i].tolist() == expected[i].tolist(), f'{what} paragraph {i}: label {k}, box {box}'
    return got


def planes_on_the_path(box_shape, row):
    """the rotated planes (out_h, out_w) of the 2 * ROUNDS probes a search met, from its heights"""
    from univer_ocr_amd.nn.ops import search_geometry, search_table
    _, table = search_table(1.0)
    node, planes = 0, []
    for height_a, height_b in np.asarray(row[1:]).reshape(ROUNDS, 2):
        ca, sa, cb, sb = table[node].tolist()
        planes += [search_geometry(*box_shape, ca, sa)[2], search_geometry(*box_shape, cb, sb)[2]]
        node = 2 * node + (1 if height_a < height_b else 2)
    return planes


def test_fixture_page_in_one_call(g, rt):
    """the page of four paragraphs through the wrapper: the reference's 13-round traces and its angles"""
    from univer_ocr_amd.nn import ops
    CP, runtime = rt
    paragraph, _, _, _, angles = stage_page(g)
    components = ops.label_components(CP.copy(paragraph, 'float32'), 'mean')
    assert int(components.count[0]) == STAGE_PARAGRAPHS
    before = runtime.launches
    got_angles, traces = ops.rotation_search(components, 0, range(1, STAGE_PARAGRAPHS + 1))
    assert runtime.launches - before == 1, 'one C call'
    assert got_angles == angles
    for p in range(STAGE_PARAGRAPHS):
        assert traces[p].dtype == np.float64 and np.array_equal(traces[p], g[f'stage/{p}/trace']), f'paragraph {p}'
    rounds, per_launch, launches = runtime.last_rotation_search()
    assert rounds == ROUNDS and per_launch >= STAGE_PARAGRAPHS and launches == 2 * ROUNDS
    assert ops.rotation_search(components, 0, []) == ([], [])
    with pytest.raises(ValueError, match='components 1'):
        ops.rotation_search(components, 0, [STAGE_PARAGRAPHS + 1])


def test_small_boxes_and_planes_around_the_band_and_the_wave(rt):
    """solid boxes of 1 x 1, 1 x 7, 7 x 1, 2 x 2 and 16 x 16 (a square: the rotated plane is largest against the bound
    the grid is sized by), and boxes whose probes meet rotated planes of 7, 8, 9, 16 and 17 rows -- one block, its edge,
    two, their edge, three -- and of 63, 64, 65 and 129 columns; then the same boxes filled at random"""
    r = np.random.default_rng(440)
    shapes = [(1, 1), (1, 7), (7, 1), (2, 2), (16, 16), (7, 5), (17, 3), (3, 63), (3, 64), (3, 65), (3, 129)]
    labels = np.zeros((24 * 3, 140), np.int32)
    paragraphs, y, x = [], 0, 0
    for k, (h, w) in enumerate(shapes, 1):
        if x + w > labels.shape[1]:
            y, x = y + 18, 0
        labels[y:y + h, x:x + w] = k
        paragraphs.append((k, (y, x, h, w)))
        x += w + 1
    got = check_search(rt, labels, paragraphs, 'solid')
    planes = [plane for (_, box), row in zip(paragraphs, got) for plane in planes_on_the_path(box[2:], row)]
    assert {BAND - 1, BAND, BAND + 1, 2 * BAND, 2 * BAND + 1} <= {oh for oh, _ in planes}, 'planes of 7, 8, 9, 16 and 17 rows'
    assert {WAVE - 1, WAVE, WAVE + 1, 2 * WAVE + 1} <= {ow for _, ow in planes}, 'planes of 63, 64, 65 and 129 columns'
    assert max(oh for oh, _ in planes_on_the_path((16, 16), got[4])) == 23, 'int(hypot(16, 16)) + 1: the square near 45 degrees'
    sparse = np.where(r.random(labels.shape) < 0.35, labels, 0)
    for k, (y, x, h, w) in paragraphs:                                  # (the corners stay: the box is the component's)
        sparse[[y, y, y + h - 1, y + h - 1], [x, x + w - 1, x, x + w - 1]] = k
    check_search(rt, sparse, paragraphs, 'sparse')


def test_other_components_in_the_box_nothing_found_and_the_second_image(rt):
    r = np.random.default_rng(441)
    page = np.zeros((40, 60), np.int32)
    page[3:30, 5:50] = np.where(r.random((27, 45)) < 0.5, 2, 3)          # two components interleaved in one box
    page[3:30, 5] = page[3:30, 49] = 2
    page[3, 5:50] = page[29, 5:50] = 3
    page[33:38, 8:30] = 1
    box = (3, 5, 27, 45)
    paragraphs = [(2, box), (3, box), (1, (33, 8, 5, 22)), (7, box), (1, box)]
    got = check_search(rt, page, paragraphs, 'ids')
    assert got[0].tolist() != got[1].tolist(), 'the two components of the box are told apart'
    for row in got[3:]:
        assert row[0] == 2 * NODES and not row[1:].any(), 'no pixel of that label in the box: 0 < 0 is false, low = a every round'
    other = np.where(r.random(page.shape) < 0.5, page, 0)
    other[3:30, 5:50] = np.where(other[3:30, 5:50] == 2, 3, 2)
    both = np.stack([other, page])
    check_search(rt, both, paragraphs[:3], 'image 1 of 2', image_index=1)
    first = check_search(rt, both, paragraphs[:3], 'image 0 of 2', image_index=0)
    assert first.tolist() != got[:3].tolist()


@pytest.fixture(scope='module')
def specks():
    """29 specks of 3 x 5 on a 64 x 128 page, every one its own pattern, and their expected rows (computed once)"""
    r = np.random.default_rng(442)
    labels = np.zeros((64, 128), np.int32)
    paragraphs = []
    for k in range(1, 30):
        y, x = 1 + 20 * ((k - 1) // 8), 1 + 16 * ((k - 1) % 8)
        labels[y:y + 3, x:x + 5] = np.where(r.random((3, 5)) < 0.6, k, 0)
        labels[y + int(r.integers(0, 3)), x + int(r.integers(0, 5))] = k
        paragraphs.append((k, (y, x, 3, 5)))
    return labels, paragraphs, expected_rows(labels, paragraphs)


@pytest.mark.parametrize('count', [1, 14, 15, 29])
def test_paragraphs_around_the_launch(count, specks, rt):
    """one launch, exactly one, one more than one, more than two; the last speck sits in the page's last rows"""
    labels, paragraphs, expected = specks
    assert paragraphs[-1][1][0] + 3 == labels.shape[0] and len({tuple(row) for row in expected.tolist()}) > 5
    got = check_search(rt, labels, paragraphs[-count:], f'{count} specks', expected=expected[-count:])
    rounds, per_launch, launches = rt[1].last_rotation_search()
    assert per_launch == 14 and launches == 2 * rounds * -(-count // per_launch)
    again = search_of(rt, labels, paragraphs[-count:])
    assert again.tobytes() == got.tobytes(), 'integer atomics only: identical bytes'


def test_capture_and_replay(specks, rt):
    """the call is asynchronous and capturable: the replayed graph walks the search of whatever the labels hold then --
    there is no host step between the rounds"""
    import torch
    CP, runtime = rt
    labels, paragraphs, expected = specks
    paragraphs = paragraphs[:16]
    r = np.random.default_rng(443)
    second = np.zeros_like(labels)                                      # other specks in the same boxes
    for k, (y, x, h, w) in paragraphs:
        second[y:y + h, x:x + w] = np.where(r.random((h, w)) < 0.5, k, 0)
        second[y + 1, x + int(r.integers(0, w))] = k
    versions = [(labels, expected[:16]), (second, expected_rows(second, paragraphs))]
    assert versions[0][1].tolist() != versions[1][1].tolist()
    labels_dev = CP.copy(labels[None], np.int32)
    rounds, table = device_table(CP)
    result = CP.copy(np.full((16, 1 + 2 * rounds), UNTOUCHED, np.int32), np.int32)
    workspace = CP.copy(np.full((workspace_ints(16),), UNTOUCHED, np.int32), np.int32)
    with runtime.capture(torch.cuda.MemPool()) as graph:
        raw_search(runtime, result.ptr, workspace.ptr, **search_arguments(labels_dev, paragraphs, table, rounds))
    for image, rows in versions[::-1] + versions:
        labels_dev.set(image[None])
        result.set(np.full(result.shape, UNTOUCHED, np.int32))
        graph.replay()
        assert CP.asnumpy(result).tolist() == rows.tolist()


def test_argument_errors_write_nothing(rt):
    from univer_ocr_amd.hip import HipError
    CP, runtime = rt
    labels = np.zeros((12, 20), np.int32)
    labels[2:9, 3:15] = 1
    labels[10:12, 16:20] = 2
    labels_dev = CP.copy(labels[None], np.int32)
    rounds, table = device_table(CP)
    result = CP.copy(np.full((2, 1 + 2 * rounds), UNTOUCHED, np.int32), np.int32)
    workspace = CP.copy(np.full((workspace_ints(2),), UNTOUCHED, np.int32), np.int32)
    paragraphs = [(1, (2, 3, 7, 12)), (2, (10, 16, 2, 4))]
    good = search_arguments(labels_dev, paragraphs, table, rounds)
    bad = [dict({name: None}) for name in ('labels', 'label_id', 'box', 'table')] + [
        dict(n_paragraphs=-1), dict(n=0), dict(h=0), dict(w=0), dict(image_index=1), dict(image_index=-1),
        dict(rounds=0), dict(rounds=17), dict(rounds=-3), dict(label_id=[1, 0]), dict(label_id=[-2, 2]),
        dict(box=[2, 3, 7, 12, -1, 16, 2, 4]), dict(box=[2, 3, 7, 12, 10, -16, 2, 4]), dict(box=[2, 3, 7, 12, 10, 16, 3, 4]),
        dict(box=[2, 3, 7, 18, 10, 16, 2, 4]), dict(box=[2, 3, 0, 12, 10, 16, 2, 4]), dict(box=[2, 3, 7, 12, 10, 16, 2, -1]),
        dict(box=[12, 3, 1, 12, 10, 16, 2, 4]), dict(table=table.ptr + 4)]
    for change in bad:
        with pytest.raises(HipError, match=r'\(-1\)'):
            raw_search(runtime, result.ptr, workspace.ptr, **dict(good, **change))
        assert (CP.asnumpy(result) == UNTOUCHED).all() and (CP.asnumpy(workspace) == UNTOUCHED).all(), f'{change}: something was written'
    for pointers in ((None, workspace.ptr), (result.ptr, None), (result.ptr + 2, workspace.ptr), (result.ptr, workspace.ptr + 2)):
        with pytest.raises(HipError, match=r'\(-1\)'):
            raw_search(runtime, *pointers, **good)
    assert (CP.asnumpy(result) == UNTOUCHED).all() and (CP.asnumpy(workspace) == UNTOUCHED).all()
    before = runtime.last_rotation_search()
    raw_search(runtime, result.ptr, workspace.ptr, **dict(good, n_paragraphs=0))      # nothing to do: OK, no launch
    raw_search(runtime, None, None, **dict(good, n_paragraphs=0, labels=None, label_id=None, box=None, table=None))
    assert (CP.asnumpy(result) == UNTOUCHED).all() and runtime.last_rotation_search() == before
    raw_search(runtime, result.ptr, workspace.ptr, **good)
    assert CP.asnumpy(result).tolist() == expected_rows(labels, paragraphs).tolist()
    # a shorter search walks the top of the same table
    short = CP.copy(np.full((2, 1 + 2 * 3), UNTOUCHED, np.int32), np.int32)
    raw_search(runtime, short.ptr, workspace.ptr, **dict(good, rounds=3))
    full = expected_rows(labels, paragraphs)
    assert CP.asnumpy(short)[:, 1:].tolist() == full[:, 1:7].tolist() and runtime.last_rotation_search()[0] == 3
    assert [(leaf + 1) >> (ROUNDS - 3) for leaf in full[:, 0].tolist()] == [leaf + 1 for leaf in CP.asnumpy(short)[:, 0].tolist()]


# ---- CropAndRotateParagraphs(search='device') ------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_stage_with_the_device_search_equals_the_reference(dtype, g, rt, monkeypatch):
    """the page of four paragraphs: the angles of the host search and of the reference, its crops in the 16-frame, one
    search call, one extent call and one crop call"""
    from univer_ocr_amd.my_model.crop import CropAndRotateParagraphs
    CP, runtime = rt
    paragraph, arrays, _, _, angles = stage_page(g)
    mask = CP.copy(paragraph, dtype)
    dev = [CP.copy(a, dtype) for a in arrays]
    stage = CropAndRotateParagraphs(search='device')
    calls = []
    original = runtime.call
    monkeypatch.setattr(runtime, 'call', lambda name, *args: (calls.append(name), original(name, *args))[1])
    result = stage(mask, dev, divisible_by=(16, 16))
    monkeypatch.undo()
    assert calls.count('uocr_rotation_search') == 1 and calls.count('uocr_rotated_extent') == 1 and calls.count('uocr_rotate_crop') == 1
    assert runtime.last_rotation_search() == (ROUNDS, 14, 2 * ROUNDS) and runtime.last_rotate()[3] == 1
    host = CropAndRotateParagraphs(search='host')
    by_host = host(mask, dev, divisible_by=(16, 16))
    assert stage.angles == host.angles == angles
    assert len(result) == 2 and all(len(per_array) == STAGE_PARAGRAPHS for per_array in result)
    for c, per_array, per_array_host in zip((1, 2), result, by_host):
        for p, crop in enumerate(per_array):
            got = CP.asnumpy(crop)
            assert got.dtype == np.dtype(dtype)
            compare_sampled(got, g[f'stage/{p}/c{c}'], 1, bound(dtype), f'paragraph {p} c={c} {dtype}')
            assert got.tobytes() == CP.asnumpy(per_array_host[p]).tobytes(), 'the same angles, the same geometry: the same crop'


# ---- the PREDICT system --------------------------------------------------------------------------------------------------
def predict_page(rt, rotation_search, monkeypatch):
    """the 64 x 96 synthetic page of tests/test_gpu_pred_to_text.py: test_predict_system_page_in_text_out, built here the
    same way: the paragraph and line masks are planted behind the Paragraph and Line nets.  Returns (text, angles, calls)."""
    from test_gpu_models import set_analytic_weights
    from test_gpu_pred_to_text import planted_lines, planted_paragraphs
    from univer_ocr_amd.my_model.model import make_divisible_by, make_predict_system
    from univer_ocr_amd.my_model.predict import predict_text
    from univer_ocr_amd.my_model.synthetic import make_page_batch
    from univer_ocr_amd.nn.model_system import RawFunctionComponent
    CP, runtime = rt
    page = make_page_batch(1, 64, 96, seed=7)['image']
    framed = make_divisible_by(page, 16, 16).shape
    system, models, names = make_predict_system(framed, rotation_search=rotation_search)
    for model in models.values():
        set_analytic_weights(model)

    def plant_paragraphs(context):
        context['paragraph_pred'] = CP.copy(planted_paragraphs(framed))

    def plant_lines(context):
        context['line_pred'] = [CP.copy(planted_lines(crop.shape)) for crop in context['cropped_monochrome']]
    system.components.insert(names.index('ParagraphCrop'), RawFunctionComponent(plant_paragraphs))
    system.components.insert(names.index('LineCrop') + 1, RawFunctionComponent(plant_lines))
    calls = []
    original = runtime.call
    monkeypatch.setattr(runtime, 'call', lambda name, *args: (calls.append(name), original(name, *args))[1])
    text = predict_text(page, system)
    monkeypatch.undo()
    return text, system.components[names.index('ParagraphCrop') + 1].stage.angles, calls


def test_predict_system_gives_the_same_text_with_either_search(rt, monkeypatch):
    text, angles, calls = predict_page(rt, 'device', monkeypatch)
    host_text, host_angles, host_calls = predict_page(rt, 'host', monkeypatch)
    assert text == host_text and [len(p) for p in text] == [2, 2] and all(isinstance(t, str) for p in text for t in p)
    assert angles == host_angles and angles[0] is None and angles[1] is not None
    assert calls.count('uocr_rotation_search') == 1 and calls.count('uocr_rotated_extent') == 1 and calls.count('uocr_rotate_crop') == 1
    assert host_calls.count('uocr_rotation_search') == 0 and host_calls.count('uocr_rotated_extent') == 14
