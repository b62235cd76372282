"""Connected-component labelling, the component table and the masked crop on the GPU (csrc/label.hip) against the
reference's results in tests/golden/paragraph_crop.npz and, at sizes derived from the kernel's own tile, against the
NumPy flood fill that tests/test_label_host.py pins to that fixture.  Everything is exact: labels, counts and tables
are integers, crops are compared bit for bit with `expected.astype(dtype)`.  The TRAIN_LINE model system runs against
the reference's Line net with the tolerances of DESIGN.md section 3 (test_model_system_lists_of_differently_sized_crops):
normalised max error 1e-5 for losses / predictions and 5e-5 for weights in float32, 1e-12 / 1e-10 in float64."""
import numpy as np
import pytest

from conftest import load_golden, rel_linf
from test_gpu_bounds import GUARD, SENTINEL, Guarded
from test_label_host import RULES, flood_fill, threshold_of

pytestmark = pytest.mark.gpu

DTYPES = ('float32', 'float64', 'float16')
MODES = {'mean': 0, 'mean_max': 1, 'value': 2}


@pytest.fixture(scope='module')
def g():
    return load_golden('paragraph_crop')


@pytest.fixture
def rt():
    from univer_ocr_amd.nn import CP
    CP.use_gpu(0)
    CP.set_dtype('float32')
    return CP, CP.runtime()


def label_raw(rt, x, rule='value', value=0.5, max_components=4096):
    """uocr_label_components on a host array (N, H, W) or (N, H, W, 1) -> labels (N, H, W), table (N, max, 8), count (N,)"""
    from univer_ocr_amd.hip import lib as hiplib
    CP, runtime = rt
    x = np.asarray(x)
    n, h, w = x.shape[:3]
    dev = CP.copy(x.reshape(n, h, w, 1), x.dtype)
    labels = CP.full((n, h, w), -7, np.int32)
    table = CP.full((n, max_components, 8), -7, np.int64)
    count = CP.full((n,), -7, np.int32)
    runtime.call('uocr_label_components', hiplib.dtype_code(x.dtype), dev.ptr, n, h, w, MODES[rule], float(value),
                 labels.ptr, table.ptr, max_components, count.ptr)
    return CP.asnumpy(labels), CP.asnumpy(table), CP.asnumpy(count)


def check_against_flood_fill(rt, mask, dtype='float32', what=''):
    mask = np.asarray(mask, bool)
    labels, table, count = label_raw(rt, mask[None].astype(dtype))
    exp_labels, exp_table = flood_fill(mask)
    assert count[0] == len(exp_table), f'{what}: count {count[0]} != {len(exp_table)}'
    assert np.array_equal(labels[0], exp_labels), f'{what}: labels differ'
    assert np.array_equal(table[0, :count[0]], exp_table), f'{what}: table differs'
    assert not table[0, count[0]:].any(), f'{what}: table entries past the count are not zero'
    return labels, table, count


@pytest.fixture
def tile_size(rt):
    """(H, W) = (2 TH + 3, 2 TW + 5) of the labelling kernels' tile: two full tiles and a ragged one each way"""
    label_raw(rt, np.ones((1, 4, 4), np.float32))
    th, tw, launches = rt[1].last_label()
    assert th > 0 and tw > 0 and launches > 0
    return 2 * th + 3, 2 * tw + 5


# ---- fixture (a): the reference's labels ---------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('rule', RULES)
def test_labels_and_table_equal_the_reference(rule, dtype, g, rt):
    for name in (str(s) for s in g['mask_names']):
        x = g[f'{name}/x'].astype(dtype)
        labels, table, count = label_raw(rt, x, rule, float(g[f'{name}/value_t']))
        expected = g[f'{name}/{rule}/table']
        assert count[0] == len(expected), f'{name}: count'
        assert np.array_equal(labels[0], g[f'{name}/{rule}/labels']), f'{name}: labels'
        assert np.array_equal(table[0, :count[0]], expected), f'{name}: table'
        assert not table[0, count[0]:].any(), f'{name}: table entries past the count are not zero'


def test_python_wrapper_reports_boxes_areas_and_centres(g, rt):
    from univer_ocr_amd.nn import ops
    CP, _ = rt
    for name, rule in (('soft_a', 'mean_max'), ('comb', 'mean'), ('soft_b', 'value')):
        threshold = float(g[f'{name}/value_t']) if rule == 'value' else rule
        comps = ops.label_components(CP.copy(g[f'{name}/x']), threshold)
        expected = g[f'{name}/{rule}/table']
        assert comps.labels.shape == g[f'{name}/x'].shape[:3] and comps.labels.dtype == np.int32
        assert comps.count.tolist() == [len(expected)]
        assert np.array_equal(comps.boxes[0], expected[:, 2:6]) and np.array_equal(comps.area[0], expected[:, 1])
        assert np.allclose(comps.center_of_mass[0], g[f'{name}/{rule}/centers'], rtol=1e-13, atol=0)
        assert np.array_equal(CP.asnumpy(comps.labels)[0], g[f'{name}/{rule}/labels'])


# ---- shapes at the tile-derived size ----------------------------------------------------------------------------------------
def serpentine(h, w):
    """one 1-pixel path through every tile: full rows every second row, joined alternately at the right and left end"""
    m = np.zeros((h, w), bool)
    m[::2] = True
    for i, y in enumerate(range(1, h, 2)):
        m[y, w - 1 if i % 2 == 0 else 0] = True
    return m


def spiral(h, w):
    m = np.zeros((h, w), bool)
    top, left, bottom, right = 0, 0, h - 1, w - 1
    while bottom - top > 3 and right - left > 3:
        m[top, left:right + 1] = m[top:bottom + 1, right] = True
        m[bottom, left + 2:right + 1] = m[top + 2:bottom + 1, left + 2] = True
        m[top + 2, left + 2:left + 4] = True
        top, left, bottom, right = top + 2, left + 2, bottom - 2, right - 2
    return m


def u_shapes(h, w):
    """prongs that begin in different tiles (rows 1 / h // 2, far apart columns) and join only in the last rows, plus a
    component that starts between them: the numbering has to follow the first pixel, not the joining order"""
    m = np.zeros((h, w), bool)
    m[h // 2:h - 1, 2] = m[1:h - 1, w - 3] = m[h - 2, 2:w - 2] = True        # left prong starts later than the right one
    m[3:h - 4, w // 2] = m[h - 5, 6:w // 2] = m[h // 3:h - 4, 6] = True       # nested, disjoint
    m[0, 0:4] = m[5, w // 3:w // 3 + 3] = True
    return m


def staircase(h, w):
    m = np.zeros((h, w), bool)
    m[np.arange(h), np.arange(h) * (w - 1) // (h - 1)] = True                  # W > 2 H: never edge neighbours
    return m


def test_all_background_and_all_foreground(tile_size, rt):
    h, w = tile_size
    labels, table, count = check_against_flood_fill(rt, np.zeros((h, w)), what='background')
    assert count[0] == 0 and not labels.any()
    labels, table, count = check_against_flood_fill(rt, np.ones((h, w)), what='foreground')
    assert count[0] == 1 and (labels == 1).all()
    assert table[0, 0].tolist() == [0, h * w, 0, h, 0, w, w * h * (h - 1) // 2, h * w * (w - 1) // 2]


@pytest.mark.parametrize('shape', ['corners', 'serpentine', 'spiral', 'u_shapes', 'staircase'])
def test_shapes_across_tile_borders(shape, tile_size, rt):
    h, w = tile_size
    if shape == 'corners':
        mask = np.zeros((h, w), bool)
        mask[0, 0] = mask[0, -1] = mask[-1, 0] = mask[-1, -1] = True
    else:
        mask = globals()[shape](h, w)
    labels, table, count = check_against_flood_fill(rt, mask, what=shape)
    expected_count = {'corners': 4, 'serpentine': 1, 'spiral': 1, 'u_shapes': 4, 'staircase': h}[shape]
    assert count[0] == expected_count


@pytest.mark.parametrize('seed', [1, 2, 3])
@pytest.mark.parametrize('density', [0.3, 0.5, 0.59, 0.7])
def test_random_masks(density, seed, tile_size, rt):
    h, w = tile_size
    mask = np.random.default_rng(1000 * seed + int(100 * density)).random((h, w)) < density
    check_against_flood_fill(rt, mask, what=f'density {density} seed {seed}')


def test_checkerboard_fills_and_overflows_the_table(rt):
    from univer_ocr_amd.hip import HipError
    from univer_ocr_amd.nn import ops
    CP, _ = rt
    yy, xx = np.mgrid[:32, :64]
    mask = (yy + xx) % 2 == 0
    exp_labels, exp_table = flood_fill(mask)
    assert len(exp_table) == 1024
    x = mask[None].astype(np.float32)
    labels, table, count = label_raw(rt, x, max_components=1024)
    assert count[0] == 1024 and np.array_equal(labels[0], exp_labels) and np.array_equal(table[0], exp_table)
    labels, table, count = label_raw(rt, x, max_components=100)
    assert count[0] == 1024, 'the count is the true number of components'
    assert np.array_equal(table[0], exp_table[:100]), 'the table holds the first max_components'
    assert np.array_equal(labels[0], exp_labels), 'the labels stay complete'
    comps = ops.label_components(CP.copy(x.reshape(1, 32, 64, 1)), 0.5, max_components=100)
    assert np.array_equal(CP.asnumpy(comps.labels)[0], exp_labels)
    with pytest.raises(HipError, match='1024 components'):
        comps.count


def test_images_of_a_batch_are_labelled_on_their_own(tile_size, rt):
    h, w = tile_size
    rng = np.random.default_rng(5)
    a, b = rng.random((h, w)) < 0.55, rng.random((h, w)) < 0.45
    a[-1], b[0] = True, True                       # full rows that would join across images in a 3-D labelling
    labels, table, count = label_raw(rt, np.stack([a, b, a]).astype(np.float32))
    for i, mask in enumerate((a, b, a)):
        exp_labels, exp_table = flood_fill(mask)
        assert count[i] == len(exp_table) and np.array_equal(labels[i], exp_labels)
        assert np.array_equal(table[i, :count[i]], exp_table)
    assert np.array_equal(labels[0], labels[2]) and np.array_equal(table[0], table[2])


def test_degenerate_images(tile_size, rt):
    _, w = tile_size
    h = 3 * w // 2
    for value in (0.0, 1.0):
        labels, table, count = check_against_flood_fill(rt, np.full((1, 1), value), what='1 x 1')
        assert count[0] == int(value)
    rng = np.random.default_rng(6)
    check_against_flood_fill(rt, rng.random((1, w)) < 0.6, what='1 x W')
    check_against_flood_fill(rt, rng.random((h, 1)) < 0.6, what='H x 1')
    check_against_flood_fill(rt, np.ones((h, 1)), what='H x 1 foreground')


def test_second_call_after_a_larger_one_and_repeatability(tile_size, rt):
    """stale workspace of a larger image must not leak into a smaller one; two calls give the same bits"""
    h, w = tile_size
    rng = np.random.default_rng(7)
    big = rng.random((2, 3 * h, 2 * w)) < 0.6
    first = label_raw(rt, big.astype(np.float32))
    small = rng.random((h - 4, w - 9)) < 0.5
    check_against_flood_fill(rt, small, what='small after big')
    check_against_flood_fill(rt, np.zeros((h - 4, w - 9)), what='empty after big')
    again = label_raw(rt, big.astype(np.float32))
    for a, b in zip(first, again):
        assert np.array_equal(a, b)
    for i in range(2):
        exp_labels, exp_table = flood_fill(big[i])
        assert np.array_equal(first[0][i], exp_labels) and np.array_equal(first[1][i, :first[2][i]], exp_table)


def test_threshold_rules_at_the_tile_size(tile_size, rt):
    """mean and (mean + max) / 2 of a multi-block reduction; values keep clear of both thresholds"""
    h, w = tile_size
    rng = np.random.default_rng(8)
    x = rng.random((2, h, w))
    for rule in ('mean', 'mean_max'):
        t = threshold_of(x, rule)
        x[np.abs(x - t) < 5e-3] += 0.02
    for dtype in DTYPES:
        xd = x.astype(dtype)
        for rule in ('mean', 'mean_max'):
            t = threshold_of(xd, rule)
            assert np.min(np.abs(xd.astype(np.float64) - t)) > 1e-3
            labels, table, count = label_raw(rt, xd, rule)
            for i in range(2):
                exp_labels, exp_table = flood_fill(xd[i].astype(np.float64) > t)
                assert count[i] == len(exp_table) and np.array_equal(labels[i], exp_labels), f'{dtype}/{rule}'
                assert np.array_equal(table[i, :count[i]], exp_table), f'{dtype}/{rule}'


def test_statistics_hand_off_three_calls_in_a_row(tile_size, rt):
    """The statistics launch hands its block sums to the last block to arrive through a counter that must be back at zero
    for the next call.  Three `mean_max` calls on one runtime, the outputs filled with a sentinel before each (label_raw):
    every call equals the flood fill at the float64 threshold and all three have the same bits.  A counter left non-zero
    would leave the threshold unwritten -- a failed comparison, nothing waits.  So that an unwritten threshold cannot be
    the previous call's (equal) value, a larger all-foreground image is labelled with the `value` rule in between: no
    statistics launch, and its root plane (all zero) lies over the smaller call's workspace."""
    h, w = tile_size
    x = np.random.default_rng(11).random((2, h, w))
    t = threshold_of(x, 'mean_max')
    x[np.abs(x - t) < 5e-3] += 0.02
    x = x.astype(np.float32)
    t = threshold_of(x, 'mean_max')
    assert np.min(np.abs(x.astype(np.float64) - t)) > 1e-3
    expected = [flood_fill(x[i].astype(np.float64) > t) for i in range(2)]
    assert all(len(exp_table) > 1 for _, exp_table in expected)
    results = []
    for call in range(3):
        labels, table, count = label_raw(rt, x, 'mean_max')
        for i, (exp_labels, exp_table) in enumerate(expected):
            assert count[i] == len(exp_table) and np.array_equal(labels[i], exp_labels), f'call {call}, image {i}'
            assert np.array_equal(table[i, :count[i]], exp_table), f'call {call}, image {i}'
        results.append((labels, table, count))
        _, _, big_count = label_raw(rt, np.ones((1, 3 * h, 3 * w), np.float32))
        assert big_count[0] == 1
    for again in results[1:]:
        for a, b in zip(results[0], again):
            assert a.tobytes() == b.tobytes()


def test_capture_and_replay(tile_size, rt):
    """both calls are asynchronous and capturable: a replayed graph labels and crops what the buffers hold then"""
    import torch
    from univer_ocr_amd.hip import lib as hiplib
    CP, runtime = rt
    h, w = tile_size
    rng = np.random.default_rng(9)
    masks = [rng.random((h, w)) < 0.55 for _ in range(2)]
    x = CP.copy(masks[0].reshape(1, h, w, 1).astype(np.float32), np.float32)
    labels, table, count = CP.zeros((1, h, w), np.int32), CP.zeros((1, 64, 8), np.int64), CP.zeros((1,), np.int32)
    out = CP.zeros((1, h, w, 1), np.float32)
    with runtime.capture(torch.cuda.MemPool()) as graph:
        runtime.call('uocr_label_components', hiplib.F32, x.ptr, 1, h, w, MODES['mean'], 0.0, labels.ptr, table.ptr, 64,
                     count.ptr)
        runtime.call('uocr_masked_crop', hiplib.F32, x.ptr, labels.ptr, 1, h, w, 1, 0, 1, 0, 0, h, w, out.ptr, h, w)
    for mask in masks[::-1]:
        x.set(mask.reshape(1, h, w, 1))
        graph.replay()
        exp_labels, exp_table = flood_fill(mask)
        assert np.array_equal(CP.asnumpy(labels)[0], exp_labels) and CP.asnumpy(count)[0] == len(exp_table)
        assert np.array_equal(CP.asnumpy(out)[0, :, :, 0], (exp_labels == 1).astype(np.float32))


# ---- masked crop -------------------------------------------------------------------------------------------------------------
def pad_centred(crop, out_h, out_w):
    """make_divisible_by's placement (my_model/model.py:26-34 of the reference): the crop in the middle of a zero frame"""
    _, h, w, c = crop.shape
    out = np.zeros((1, out_h, out_w, c), crop.dtype)
    py, px = (out_h - h) // 2, (out_w - w) // 2
    out[:, py:py + h, px:px + w] = crop
    return out


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('c', [1, 2, 4, 3])
def test_masked_crops_equal_the_reference(c, dtype, g, rt):
    from univer_ocr_amd.my_model.model import make_divisible_by
    from univer_ocr_amd.nn import ops
    CP, _ = rt
    for name in (str(s) for s in g['crop_masks']):
        comps = ops.label_components(CP.copy(g[f'{name}/x'], dtype), 'mean')
        image = g[f'{name}/img{c}'] if c != 3 else g[f'{name}/img4'][..., :3]
        dev = CP.copy(image, dtype)
        assert comps.count[0] == len(g[f'{name}/mean/table'])
        for k in range(1, comps.count[0] + 1):
            expected = g[f'{name}/crop{c}/{k}'] if c != 3 else g[f'{name}/crop4/{k}'][..., :3]
            crop = ops.masked_crop(dev, comps, 0, k)
            assert same_bits(CP.asnumpy(crop), expected.astype(dtype)), f'{name} component {k}'
            padded = ops.masked_crop(dev, comps, 0, k, divisible_by=(16, 16))
            exp_padded = make_divisible_by(expected, 16, 16)
            assert padded.shape == exp_padded.shape and padded.shape[1] % 16 == 0 and padded.shape[2] % 16 == 0
            assert padded.shape[1] > expected.shape[1] and padded.shape[2] > expected.shape[2]
            assert same_bits(CP.asnumpy(padded), exp_padded.astype(dtype)), f'{name} component {k} padded'


def test_masked_crop_writes_all_of_out_and_only_its_component(g, rt):
    """out is filled with NaN first: the frame comes out zero, a pixel of another component inside the box too"""
    from univer_ocr_amd.hip import lib as hiplib
    CP, runtime = rt
    labels, table = g['u_shapes/mean/labels'], g['u_shapes/mean/table']
    # the box of the second U holds all of the U nested inside it (component 4 inside component 3's box)
    outer = next(k for k, (_, _, y0, y1, x0, x1, _, _) in enumerate(table, 1)
                 if any(j != k and np.any(labels[y0:y1, x0:x1] == j) for j in range(1, len(table) + 1)))
    _, _, y0, y1, x0, x1, _, _ = (int(v) for v in table[outer - 1])
    assert np.any((labels[y0:y1, x0:x1] != outer) & (labels[y0:y1, x0:x1] != 0))
    image = g['u_shapes/img2'] + 1.0                                      # no zero among the inputs
    h, w = labels.shape
    dev, dev_labels = CP.copy(image, np.float32), CP.copy(labels[None], np.int32)
    out_h, out_w = y1 - y0 + 5, x1 - x0 + 2
    out = CP.copy(np.full((1, out_h, out_w, 2), np.nan), np.float32)
    runtime.call('uocr_masked_crop', hiplib.F32, dev.ptr, dev_labels.ptr, 1, h, w, 2, 0, outer, y0, x0, y1 - y0, x1 - x0,
                 out.ptr, out_h, out_w)
    expected = pad_centred((image[0] * (labels == outer)[:, :, None])[None, y0:y1, x0:x1], out_h, out_w)
    host = CP.asnumpy(out)
    assert not np.isnan(host).any(), 'out is not fully written'
    assert same_bits(host, expected.astype(np.float32))
    assert not host[0, :2].any() and not host[0, -3:].any() and not host[0, :, :1].any() and not host[0, :, -1:].any()


def test_masked_crop_argument_errors_leave_out_untouched(rt):
    from univer_ocr_amd.hip import HipError
    from univer_ocr_amd.hip import lib as hiplib
    CP, runtime = rt
    n, h, w, c = 2, 12, 20, 2
    image, labels = CP.zeros((n, h, w, c), np.float32), CP.zeros((n, h, w), np.int32)
    out = CP.copy(np.full((1, 8, 8, c), np.nan), np.float32)
    good = dict(image=image.ptr, labels=labels.ptr, n=n, h=h, w=w, c=c, index=1, k=1, y0=2, x0=3, ch=6, cw=7, out=out.ptr,
                out_h=8, out_w=8)
    bad = [dict(image=None), dict(labels=None), dict(out=None), dict(h=-1), dict(c=-2), dict(index=2), dict(index=-1),
           dict(k=0), dict(y0=-1), dict(x0=-1), dict(y0=7), dict(x0=14), dict(ch=11), dict(cw=18), dict(out_h=5),
           dict(out_w=6), dict(ch=-1)]
    for change in bad:
        a = dict(good, **change)
        with pytest.raises(HipError, match=r'\(-1\)'):
            runtime.call('uocr_masked_crop', hiplib.F32, a['image'], a['labels'], a['n'], a['h'], a['w'], a['c'], a['index'],
                         a['k'], a['y0'], a['x0'], a['ch'], a['cw'], a['out'], a['out_h'], a['out_w'])
        assert np.isnan(CP.asnumpy(out)).all(), f'{change}: out was touched'
    a = good
    runtime.call('uocr_masked_crop', hiplib.F32, a['image'], a['labels'], a['n'], a['h'], a['w'], a['c'], a['index'], a['k'],
                 a['y0'], a['x0'], a['ch'], a['cw'], a['out'], a['out_h'], a['out_w'])
    assert not CP.asnumpy(out).any()
    x = CP.zeros((1, 4, 4, 1), np.float32)
    table, count = CP.zeros((1, 4, 8), np.int64), CP.zeros((1,), np.int32)
    for args in ((None, 1, 4, 4, 0, 0.0, labels.ptr, table.ptr, 4, count.ptr),
                 (x.ptr, 1, 4, 4, 0, 0.0, None, table.ptr, 4, count.ptr),
                 (x.ptr, 1, 4, 4, 0, 0.0, labels.ptr, None, 4, count.ptr),
                 (x.ptr, 1, 4, 4, 0, 0.0, labels.ptr, table.ptr, 4, None),
                 (x.ptr, 1, -4, 4, 0, 0.0, labels.ptr, table.ptr, 4, count.ptr),
                 (x.ptr, 1, 4, 4, 3, 0.0, labels.ptr, table.ptr, 4, count.ptr),
                 (x.ptr, 1, 4, 4, 0, 0.0, labels.ptr, table.ptr, -1, count.ptr)):
        with pytest.raises(HipError, match=r'\(-1\)'):
            runtime.call('uocr_label_components', hiplib.F32, *args)


# ---- bounds ------------------------------------------------------------------------------------------------------------------
def test_everything_stays_inside_its_buffers(tile_size, rt):
    """inputs and outputs sit between sentinel borders (tests/test_gpu_bounds.py) at the ragged tile-derived size"""
    from univer_ocr_amd.hip import lib as hiplib
    CP, runtime = rt
    h, w = tile_size
    n, max_components = 2, 37
    rng = np.random.default_rng(10)
    masks = rng.random((n, h, w)) < 0.45
    x = Guarded(CP, n * h * w)
    x.buf.set(np.concatenate([np.full(GUARD, SENTINEL), masks.reshape(-1), np.full(GUARD, SENTINEL)]).astype(np.float32))
    labels, table, count = Guarded(CP, n * h * w), Guarded(CP, n * max_components * 8 * 2), Guarded(CP, n)
    runtime.call('uocr_label_components', hiplib.F32, x.ptr, n, h, w, MODES['mean'], 0.0, labels.ptr, table.ptr,
                 max_components, count.ptr)
    got_labels = labels.check('labels').view(np.int32).reshape(n, h, w)
    got_table = table.check('table').view(np.int64).reshape(n, max_components, 8)
    got_count = count.check('count').view(np.int32)
    x.check('x', expect_written=False)
    boxes = []
    for i in range(n):
        exp_labels, exp_table = flood_fill(masks[i])
        assert got_count[i] == len(exp_table) > max_components
        assert np.array_equal(got_labels[i], exp_labels) and np.array_equal(got_table[i], exp_table[:max_components])
        boxes.append(exp_table)
    # crops of the component with the largest box of image 1, every channel count, into guarded buffers
    k = int(np.argmax((boxes[1][:, 3] - boxes[1][:, 2]) * (boxes[1][:, 5] - boxes[1][:, 4]))) + 1
    _, _, y0, y1, x0, x1, _, _ = (int(v) for v in boxes[1][k - 1])
    dev_labels = CP.copy(got_labels, np.int32)
    for c in (1, 2, 3, 4):
        image = rng.integers(1, 64, (n, h, w, c)) / 64.0
        src = Guarded(CP, n * h * w * c)
        src.buf.set(np.concatenate([np.full(GUARD, SENTINEL), image.reshape(-1), np.full(GUARD, SENTINEL)]).astype(np.float32))
        for out_h, out_w in ((y1 - y0, x1 - x0), (y1 - y0 + 16 - (y1 - y0) % 16, x1 - x0 + 16 - (x1 - x0) % 16)):
            out = Guarded(CP, out_h * out_w * c)
            runtime.call('uocr_masked_crop', hiplib.F32, src.ptr, dev_labels.ptr, n, h, w, c, 1, k, y0, x0, y1 - y0, x1 - x0,
                         out.ptr, out_h, out_w)
            got = out.check(f'crop c={c}').reshape(1, out_h, out_w, c)
            expected = pad_centred((image[1] * (got_labels[1] == k)[:, :, None])[None, y0:y1, x0:x1], out_h, out_w)
            assert same_bits(got, expected.astype(np.float32)), f'crop c={c} {out_h} x {out_w}'


# ---- the TRAIN_LINE model system -----------------------------------------------------------------------------------------
SYSTEM_TOL = {'float32': (1e-5, 5e-5), 'float64': (1e-12, 1e-10)}      # (losses and predictions, weights)


def page_context(g, paragraph=None):
    from univer_ocr_amd.my_model.model import Modes, make_context_maker
    layers = {tag: g[f'page/{tag}'] for tag in ('monochrome', 'paragraph', 'line')}
    if paragraph is not None:
        layers['paragraph'] = paragraph
    return make_context_maker(Modes.TRAIN_LINE)(lambda layer_tags: {tag: layers[tag] for tag in layer_tags})


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('opt_tag', ['sgd', 'adam'])
def test_train_line_system_equals_the_reference(opt_tag, dtype, g, rt):
    """[ParagraphCrop, Line] on the page of fixture (b): the crops equal the reference's exactly; losses, line_pred[p] and
    the weights after the two steps (one per paragraph) equal the reference Line net's to the tolerances of DESIGN 3"""
    from test_gpu_models import set_analytic_weights
    from univer_ocr_amd.my_model.model import Modes, make_model_system
    from univer_ocr_amd.nn.optimizers import Adam, Momentum
    CP, _ = rt
    CP.set_dtype(dtype)
    try:
        opt = Momentum(lr=0.01, momentum=0) if opt_tag == 'sgd' else Adam(lr=0.0015)
        system, models, names = make_model_system((1, 80, 192, 1), opt, mode=Modes.TRAIN_LINE)
        assert names == ['ParagraphCrop', 'Line']
        set_analytic_weights(models['Line'])
        context = page_context(g)
        system.train(context)
        for key in ('cropped_monochrome', 'cropped_line'):
            assert len(context[key]) == 2
            for p in range(2):
                assert same_bits(CP.asnumpy(context[key][p]), g[f'{key}{p}'].astype(dtype)), f'{key}[{p}]'
        tol, weight_tol = SYSTEM_TOL[dtype]
        entry = context['losses']['Line']
        errs = {'losses': rel_linf(np.array([float(v) for v in entry['output_losses']]), g[f'{opt_tag}/train/Line/output_losses']),
                'reg': rel_linf(np.array(float(entry['regularization_loss'])), g[f'{opt_tag}/train/Line/regularization_loss'])}
        assert len(context['line_pred']) == 2
        for p in range(2):
            pred, key = CP.asnumpy(context['line_pred'][p]), f'{opt_tag}/train/line_pred{p}'
            errs[f'pred{p}'] = (rel_linf(pred, g[key]) if key in g.files
                                else rel_linf(pred.reshape(-1)[::5], g[key + '@stride5']))
        werrs = {pn: rel_linf(CP.asnumpy(p.value), g[f'{opt_tag}/final/{pn}']) for pn, p in models['Line'].params().items()}
        print(f'{opt_tag}/{dtype}: ' + ', '.join(f'{k} {v:.2e}' for k, v in errs.items()) +
              f', weights {max(werrs.values()):.2e} ({max(werrs, key=werrs.get)})')
        for what, err in errs.items():
            assert err <= tol, f'{what}: rel_linf={err:.3e} > {tol:.1e}'
        for what, err in werrs.items():
            assert err <= weight_tol, f'{what}: rel_linf={err:.3e} > {weight_tol:.1e}'
    finally:
        CP.set_dtype('float32')


def test_page_without_paragraphs_trains_nothing(g, rt):
    from univer_ocr_amd.my_model.model import Modes, make_model_system
    CP, _ = rt
    system, models, _ = make_model_system((1, 80, 192, 1), mode=Modes.TRAIN_LINE)
    before = {pn: CP.asnumpy(p.value).copy() for pn, p in models['Line'].params().items()}
    context = page_context(g, paragraph=np.zeros_like(g['page/paragraph']))
    system.train(context)
    assert context['cropped_monochrome'] == [] and context['cropped_line'] == []
    assert context['losses'] == {} and 'line_pred' not in context
    for pn, p in models['Line'].params().items():
        assert np.array_equal(CP.asnumpy(p.value), before[pn])
