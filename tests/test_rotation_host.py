"""Host side of the paragraph-rotation feature: the fixture tests/golden/rotation.npz (made from the reference's
rotate_array, FindObjectHeightInRotated._func and CropAndRotateSingleParagraph._func by
tests/golden/make_golden_rotation.py), the NumPy restatement `rotate_rules` of ndimage.rotate(.., axes=(2, 1),
reshape=True) at orders 0 and 1 that the GPU tests use as expected value at sizes the fixture cannot know (trusted only
because it is pinned to the fixture here and, where scipy is installed, to scipy over a sweep of boxes and angles), the
host search of my_model/crop.py, the stage's call pattern with the device operations replaced, the model systems'
assembly and the ABI names.  Nothing here needs a GPU.

Tolerances.  Extents and shapes are integers: equality.  Order-1 values: the restatement and scipy differ only in the
order of a four-term sum of products of numbers below 1 -- observed 1.4e-14 -- so 1e-12 leaves two decades."""

import numpy as np
import pytest

from conftest import load_golden
from test_line_crop_host import label_rules

NEW_SYMBOLS = ('uocr_rotated_extent', 'uocr_rotate_crop', 'uocr_ctx_last_rotate')
ORDER1_TOL = 1e-12
SHIFT = 1e-9
STAGE_PARAGRAPHS = 4


# ---- the restatement ---------------------------------------------------------------------------------------------------
def geometry_rules(ih, iw, angle):
    """what scipy computes in Python: M, offset, (out_h, out_w)"""
    c, s = np.cos(np.deg2rad(angle)), np.sin(np.deg2rad(angle))
    M = np.array([[c, s], [-s, c]])
    out_shape = (np.ptp(M @ [[0, 0, ih, ih], [0, iw, 0, iw]], axis=1) + 0.5).astype(int)
    offset = (np.array([ih, iw]) - 1) / 2 - M @ ((out_shape - 1) / 2)
    return M, offset, (int(out_shape[0]), int(out_shape[1]))


def rotate_rules(plane, angle, order, shift=0.0):
    """ndimage.rotate(plane, angle, order=order, reshape=True, mode='constant', cval=0) of a (h, w) or (h, w, c) plane
    rotated in its first two axes; `shift` is added to every source coordinate (the tie condition of the fixture).
    Coordinates in float64, every product and sum rounded on its own: (offset + oy * m0) + ox * m1.  A coordinate outside
    [0, n - 1] gives 0.  Order 0 reads floor(c + 0.5).  Order 1: weights 1 - t and 1 - (1 - t) over floor(c) and
    floor(c) + 1, the four terms (value * wy) * wx added row-major, the neighbour at index n never read."""
    ih, iw = plane.shape[:2]
    M, offset, (oh, ow) = geometry_rules(ih, iw, angle)
    oy, ox = np.mgrid[:oh, :ow].astype(np.float64)
    cy = (offset[0] + oy * M[0, 0]) + ox * M[0, 1] + shift
    cx = (offset[1] + oy * M[1, 0]) + ox * M[1, 1] + shift
    inside = (cy >= 0) & (cy <= ih - 1) & (cx >= 0) & (cx <= iw - 1)
    tail = (slice(None),) * 2 + (None,) * (plane.ndim - 2)
    if order == 0:
        sy, sx = np.floor(cy + 0.5).astype(int).clip(0, ih - 1), np.floor(cx + 0.5).astype(int).clip(0, iw - 1)
        return np.where(inside[tail], plane[sy, sx], np.zeros((), plane.dtype))
    fy, fx = np.floor(cy), np.floor(cx)
    wy, wx = [1.0 - (cy - fy)], [1.0 - (cx - fx)]
    wy.append(1.0 - wy[0]), wx.append(1.0 - wx[0])
    iy, ix = fy.astype(int).clip(0, ih - 1), fx.astype(int).clip(0, iw - 1)
    out = np.zeros((oh, ow) + plane.shape[2:], np.float64)
    for dy in (0, 1):
        for dx in (0, 1):
            y, x = iy + dy, ix + dx
            read = inside & (y < ih) & (x < iw)
            value = plane[np.minimum(y, ih - 1), np.minimum(x, iw - 1)].astype(np.float64)
            out += np.where(read[tail], (value * wy[dy][tail]) * wx[dx][tail], 0.0)
    return out


def extent_rules(mask, angle, shift=0.0):
    """find_objects of the order-0 rotation of a boolean (h, w) mask: (y0, y1, x0, x1), zeros when no pixel is set"""
    ys, xs = np.nonzero(rotate_rules(mask, angle, 0, shift))
    return (int(ys.min()), int(ys.max()) + 1, int(xs.min()), int(xs.max()) + 1) if len(ys) else (0, 0, 0, 0)


def framed(crop, divisible_by):
    """make_divisible_by (my_model/model.py:26-34) on (h, w, c): at least one row and column of zeros, the crop centred"""
    if divisible_by is None:
        return crop
    h, w = crop.shape[:2]
    oh, ow = h + divisible_by[0] - h % divisible_by[0], w + divisible_by[1] - w % divisible_by[1]
    out = np.zeros((oh, ow) + crop.shape[2:], crop.dtype)
    out[(oh - h) // 2:(oh - h) // 2 + h, (ow - w) // 2:(ow - w) // 2 + w] = crop
    return out


def crop_rules(image, labels, k, box, angle, divisible_by=None, region=None):
    """interpreter.py:303-308 and :340-346 for one array: image (1, H, W, c), labels (H, W), box (y0, x0, h, w) of
    component k -> (1, h', w', c) float64.  Nothing outside the box is looked at."""
    y, x, h, w = box
    mask = labels[y:y + h, x:x + w] == k
    plane = np.where(mask[:, :, None], image[0, y:y + h, x:x + w, :], 0.0)
    y0, y1, x0, x1 = extent_rules(mask, angle) if region is None else region
    return framed(rotate_rules(plane, angle, 1)[y0:y1, x0:x1], divisible_by)[None]


# ---- the fixture -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def g():
    return load_golden('rotation')


def f64(a):
    return np.asarray(a, np.float64)


def probe_cases(g):
    """(name, labels int32 (H, W) of its page, label, box, angles, extents, out_shapes) per mask of fixture (a)"""
    for name in g['probe/names']:
        p = f'probe/{name}'
        yield (str(name), g[f'probe/page{int(g[p + "/page"])}/labels'].astype(np.int32), int(g[p + '/label']),
               tuple(int(v) for v in g[p + '/box']), g[p + '/angles'], g[p + '/extents'], g[p + '/out_shapes'])


def rotation_cases(g):
    """(name, c, labels, label, box, angle, image (1, H, W, c) float64, expected, stride) per crop of fixture (b):
    expected is the whole crop (stride 1) or every 5th element of it"""
    by_name = {case[0]: case for case in probe_cases(g)}
    for name in g['rot/names']:
        _, labels, k, box, *_ = by_name[str(name)]
        for c in (1, 2, 4):
            image = f64(g[f'rot/{name}/img{c}'])
            for i, angle in enumerate(g[f'rot/{name}/angles']):
                key = f'rot/{name}/c{c}/{i}'
                stride = 1 if key in g.files else 5
                yield str(name), c, labels, k, box, float(angle), image, g[key if stride == 1 else key + '@stride5'], stride


def compare_sampled(got, expected, stride, tol_of, what):
    """got against the stored crop or its every 5th element; tol_of(expected) -> the bound per element"""
    if stride == 1:
        assert got.shape == expected.shape, f'{what}: {got.shape} != {expected.shape}'
    else:
        got = got.reshape(-1)[::stride]
        assert got.shape == expected.shape, f'{what}: {got.shape} sampled elements, expected {expected.shape}'
    assert not np.isnan(got).any(), f'{what}: NaN at {np.argwhere(np.isnan(got))[:4].tolist()}'
    excess = np.abs(f64(got) - expected) - tol_of(expected)
    assert (excess <= 0).all(), f'{what}: off by {np.abs(f64(got) - expected).max():.3e} at {np.argwhere(excess > 0)[:4].tolist()}'


def stage_page(g):
    """paragraph (1, H, W, 1), [img1, img2], labels (H, W), boxes [(y0, x0, h, w)] in label order, angles (None or degrees)"""
    paragraph = f64(g['stage/paragraph'])
    labels, count = label_rules(paragraph[0, :, :, 0] > np.mean(paragraph))
    assert count == STAGE_PARAGRAPHS
    boxes = []
    for k in range(1, count + 1):
        ys, xs = np.nonzero(labels == k)
        boxes.append((int(ys.min()), int(xs.min()), int(ys.max() - ys.min() + 1), int(xs.max() - xs.min() + 1)))
    angles = [None if np.isnan(g[f'stage/{p}/angle']) else float(g[f'stage/{p}/angle']) for p in range(count)]
    return paragraph, [f64(g['stage/img1']), f64(g['stage/img2'])], labels, boxes, angles


def replay(trace, eps=1.0):
    """interpreter.py:321-336 on a recorded trace: checks every probe angle, returns the final angle"""
    low, high = 0.0, 180.0
    for a, b, height_a, height_b in trace:
        assert high - low > eps
        assert a == low + (high - low) / 3 and b == high - (high - low) / 3
        if height_a < height_b:
            high = b
        else:
            low = a
    assert not high - low > eps
    angle = (high + low) / 2
    return angle if eps <= angle <= 180.0 - eps else None


def test_fixture_is_consistent(g):
    names = [str(n) for n in g['probe/names']]
    assert len(names) >= 10 and set(str(n) for n in g['rot/names']) <= set(names)
    for name, labels, k, box, angles, extents, out_shapes in probe_cases(g):
        y, x, h, w = box
        mask = labels == k
        ys, xs = np.nonzero(mask)
        assert (ys.min(), xs.min(), ys.max() + 1, xs.max() + 1) == (y, x, y + h, x + w), f'{name}: the box is the component\'s'
        assert len(angles) == 34 and extents.shape == (34, 4) and out_shapes.shape == (34, 2)
        assert (extents[:, 1] > extents[:, 0]).all() and (extents[:, 1] <= out_shapes[:, 0]).all() and (extents[:, 3] <= out_shapes[:, 1]).all()
        # the first 26 angles are the mask's own search: replayed from the stored heights
        heights = extents[:26, 1] - extents[:26, 0]
        replay(np.column_stack([angles[0:26:2], angles[1:26:2], heights[0::2], heights[1::2]]))
    boxes_overlap = lambda a, b: a[0] < b[0] + b[2] and b[0] < a[0] + a[2] and a[1] < b[1] + b[3] and b[1] < a[1] + a[3]
    page1 = [case[3] for case in probe_cases(g) if int(g[f'probe/{case[0]}/page']) == 1]
    assert any(boxes_overlap(a, b) for i, a in enumerate(page1) for b in page1[i + 1:]), 'two components whose boxes overlap'
    paragraph, arrays, labels, boxes, angles = stage_page(g)
    assert paragraph.shape == (1, 96, 160, 1) and [a.shape[3] for a in arrays] == [1, 2]
    assert angles[0] is None and sum(a is not None for a in angles) >= 2
    for p in range(STAGE_PARAGRAPHS):
        trace = g[f'stage/{p}/trace']
        assert trace.shape == (13, 4)
        assert replay(trace) == angles[p]
        for c in (1, 2):
            crop = g[f'stage/{p}/c{c}']
            assert crop.dtype == np.float64 and crop.shape[0] == 1 and crop.shape[3] == c
            assert crop.shape[1] % 16 == 0 and crop.shape[2] % 16 == 0
    for a in [g[k] for k in g.files if '/img' in k]:
        assert np.array_equal(f64(a) * 64, np.round(f64(a) * 64)) and f64(a).min() >= 0 and f64(a).max() < 1


# ---- the restatement against the fixture -----------------------------------------------------------------------------------
def test_rules_reproduce_the_probes_exactly(g):
    """(a): every extent and out shape, also with every coordinate shifted by +-1e-9 (the fixture's condition)"""
    count = 0
    for name, labels, k, (y, x, h, w), angles, extents, out_shapes in probe_cases(g):
        mask = labels[y:y + h, x:x + w] == k
        for angle, extent, out_shape in zip(angles, extents, out_shapes):
            assert geometry_rules(h, w, angle)[2] == tuple(out_shape), f'{name} at {angle}'
            for shift in (0.0, SHIFT, -SHIFT):
                assert extent_rules(mask, angle, shift) == tuple(extent), f'{name} at {angle}, shift {shift}'
            count += 1
    assert count >= 340


def test_rules_reproduce_the_rotated_crops(g):
    """(b): order 1, region cut, within 1e-12"""
    worst = 0.0
    for name, c, labels, k, box, angle, image, expected, stride in rotation_cases(g):
        got = crop_rules(image, labels, k, box, angle)
        compare_sampled(got, expected, stride, lambda e: ORDER1_TOL, f'{name} c={c} at {angle}')
        worst = max(worst, np.abs((got if stride == 1 else got.reshape(-1)[::stride]) - expected).max())
    print(f'rules against the reference\'s order-1 crops: max difference {worst:.2e}')


def test_rules_reproduce_the_stage(g):
    """(c): angle None is the upright masked crop, the others order-1 crops; all in make_divisible_by's frame"""
    _, arrays, labels, boxes, angles = stage_page(g)
    for p, (box, angle) in enumerate(zip(boxes, angles)):
        for image in arrays:
            c = image.shape[3]
            if angle is None:
                y, x, h, w = box
                got = framed(np.where((labels[y:y + h, x:x + w] == p + 1)[:, :, None], image[0, y:y + h, x:x + w], 0.0), (16, 16))[None]
                assert np.array_equal(got, g[f'stage/{p}/c{c}'])
            else:
                got = crop_rules(image, labels, p + 1, box, angle, (16, 16))
                compare_sampled(got, g[f'stage/{p}/c{c}'], 1, lambda e: ORDER1_TOL, f'paragraph {p} c={c}')


def test_rules_equal_scipy_over_a_sweep():
    """200 random boxes of 3..40 pixels a side at random angles: out shapes and order-1 values agree for every case; the
    extent of the order-0 rotation is compared unless shifting every coordinate by +-1e-9 changes it (a pixel chosen by a
    tie, which cannot be pinned to the bit) -- at most 5 % of the cases"""
    ndimage = pytest.importorskip('scipy.ndimage')
    r = np.random.default_rng(410)
    skipped, worst = 0, 0.0
    cases = 200
    for case in range(cases):
        h, w = (int(v) for v in r.integers(3, 41, 2))
        angle = float(r.uniform(0, 180))
        mask = r.random((h, w)) < 0.5
        mask[r.integers(0, h), r.integers(0, w)] = True
        plane = r.integers(0, 64, (h, w, 2)) / 64.0
        what = f'case {case}: {h} x {w} at {angle}'
        smooth = ndimage.rotate(plane, angle, axes=(1, 0), order=1, reshape=True)
        got = rotate_rules(plane, angle, 1)
        assert got.shape == smooth.shape, what
        worst = max(worst, np.abs(got - smooth).max())
        assert np.abs(got - smooth).max() <= ORDER1_TOL, what
        if len({extent_rules(mask, angle, shift) for shift in (0.0, SHIFT, -SHIFT)}) > 1:
            skipped += 1
            continue
        ys, xs = np.nonzero(ndimage.rotate(mask, angle, axes=(1, 0), order=0, reshape=True))
        assert extent_rules(mask, angle) == (ys.min(), ys.max() + 1, xs.min(), xs.max() + 1), what
    print(f'sweep: {skipped} of {cases} extents skipped for a tie, order 1 max difference {worst:.2e}')
    assert skipped <= cases // 20


# ---- the host search ---------------------------------------------------------------------------------------------------
def test_search_angle_reproduces_the_traces(g):
    from univer_ocr_amd.my_model.crop import search_angle, search_steps
    *_, angles = stage_page(g)
    for p in range(STAGE_PARAGRAPHS):
        trace = g[f'stage/{p}/trace']
        heights = {float(a): h for a, b, ha, hb in trace for a, h in ((a, ha), (b, hb))}
        asked = []

        def height_of(angle):
            asked.append(angle)
            return heights[angle]                                   # (a KeyError: an angle the reference did not probe)
        assert search_angle(height_of) == angles[p]
        assert asked == [float(v) for row in trace for v in row[:2]]
    assert search_angle(lambda angle: angle) is None                # ends near 0
    assert search_angle(lambda angle: -angle) is None               # ends near 180
    assert search_angle(lambda angle: abs(angle - 40.0)) == pytest.approx(40.0, abs=1.0)
    steps = search_steps()
    rounds = 0
    next(steps)
    try:
        while True:
            rounds += 1
            steps.send((1, 1))
    except StopIteration:
        pass
    assert rounds == 13, 'the interval shrinks by a third whatever the heights'
    assert search_angle(lambda angle: 1 / 0, eps=180.0) is None     # no round at all, and 90 is outside [180, 0]


def test_rotation_geometry_equals_the_fixture(g):
    from univer_ocr_amd.nn.ops import rotation_geometry
    for name, _, _, (_, _, h, w), angles, _, out_shapes in probe_cases(g):
        for angle, out_shape in zip(angles, out_shapes):
            M, offset, shape = rotation_geometry(h, w, float(angle))
            assert shape == tuple(out_shape), f'{name} at {angle}'
            rules = geometry_rules(h, w, float(angle))
            assert M.dtype == np.float64 and np.array_equal(M, rules[0]) and np.array_equal(offset, rules[1])


# ---- the stage with the device operations replaced ---------------------------------------------------------------------
class FakeOps:
    """nn/ops.py as the stage sees it, on host arrays: counts the calls, computes extents by the rules"""

    def __init__(self):
        self.calls = []

    def as_device(self, a):
        return a

    def label_components(self, mask, threshold, max_components):
        labels, count = label_rules(mask[0, :, :, 0] > np.mean(mask))
        self.calls.append(('label', threshold))
        return type('Components', (), {'labels': labels, 'count': [count]})()

    def rotated_extent(self, components, image_index, probes):
        self.calls.append(('extent', len(probes)))
        out = []
        for k, angle in probes:
            ys, xs = np.nonzero(components.labels == k)
            out.append(extent_rules(components.labels[ys.min():ys.max() + 1, xs.min():xs.max() + 1] == k, angle))
        return np.array(out, np.int32)

    def rotate_crop(self, entries, divisible_by=None):
        self.calls.append(('crop', len(entries)))
        return [('turned', id(a), k, angle, tuple(region), divisible_by) for a, _, _, k, angle, region in entries]

    def masked_crop(self, array, components, image_index, k, divisible_by=None):
        self.calls.append(('masked', k))
        return ('upright', id(array), k, divisible_by)


def test_stage_makes_fourteen_extent_calls_and_one_crop_call(g, monkeypatch):
    from univer_ocr_amd.my_model import crop
    paragraph, arrays, labels, boxes, angles = stage_page(g)
    fake = FakeOps()
    monkeypatch.setattr(crop, 'ops', fake)
    stage = crop.CropAndRotateParagraphs()
    result = stage(paragraph, arrays, divisible_by=(16, 16))
    kinds = [kind for kind, _ in fake.calls]
    assert kinds.count('extent') == 14 and kinds.count('crop') == 1 and kinds.count('label') == 1
    assert [n for kind, n in fake.calls if kind == 'extent'] == [2 * STAGE_PARAGRAPHS] * 13 + [sum(a is not None for a in angles)]
    assert stage.angles == angles, 'the angles of the reference, None where it says None'
    assert len(result) == len(arrays) and all(len(per_array) == STAGE_PARAGRAPHS for per_array in result)
    for a, per_array in zip(arrays, result):
        for p, item in enumerate(per_array):
            if angles[p] is None:
                assert item == ('upright', id(a), p + 1, (16, 16))
            else:
                y, x, h, w = boxes[p]
                region = extent_rules(labels[y:y + h, x:x + w] == p + 1, angles[p])
                assert item == ('turned', id(a), p + 1, angles[p], region, (16, 16))
    # find_rotation=False: CropParagraphs' calls, nothing else
    fake.calls.clear()
    result = crop.CropAndRotateParagraphs(find_rotation=False)(paragraph, arrays)
    assert [kind for kind, _ in fake.calls] == ['label'] + ['masked'] * (2 * STAGE_PARAGRAPHS)
    assert result == [[('upright', id(a), p + 1, None) for p in range(STAGE_PARAGRAPHS)] for a in arrays]


def test_stage_makes_no_rotation_call_for_an_empty_page(monkeypatch):
    from univer_ocr_amd.my_model import crop
    fake = FakeOps()
    monkeypatch.setattr(crop, 'ops', fake)
    stage = crop.CropAndRotateParagraphs()
    assert stage(np.zeros((1, 8, 9, 1)), [np.zeros((1, 8, 9, 1)), np.zeros((1, 8, 9, 3))]) == [[], []]
    assert fake.calls == [('label', 'mean')] and stage.angles == []


def test_stage_refuses_what_does_not_fit(monkeypatch):
    from univer_ocr_amd.my_model import crop
    monkeypatch.setattr(crop, 'ops', FakeOps())
    for stage in (crop.CropAndRotateParagraphs(), crop.CropAndRotateParagraphs(find_rotation=False)):
        for mask in (np.zeros((2, 8, 9, 1)), np.zeros((1, 8, 9, 2)), np.zeros((8, 9))):
            with pytest.raises(ValueError, match=r'\(1, H, W, 1\)'):
                stage(mask, [])
        for array in (np.zeros((1, 8, 8, 1)), np.zeros((1, 9, 9, 1)), np.zeros((8, 9, 1)), np.zeros((2, 8, 9, 1))):
            with pytest.raises(ValueError, match='does not match the mask'):
                stage(np.zeros((1, 8, 9, 1)), [np.zeros((1, 8, 9, 4)), array])
    with pytest.raises(NotImplementedError, match='rotation search'):
        crop.CropParagraphs(find_rotation=True)


# ---- the ABI -------------------------------------------------------------------------------------------------------------
def test_library_exports_the_new_entry_points():
    from univer_ocr_amd.hip import lib as hiplib
    lib = hiplib.get_lib()
    assert lib.uocr_abi_version() == 4
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), f'{name} is not exported by {hiplib.lib_path()}'


# ---- the model systems ---------------------------------------------------------------------------------------------------
def test_find_rotation_puts_the_new_stage_into_the_systems():
    from univer_ocr_amd.my_model.crop import CropAndRotateParagraphs, CropParagraphs
    from univer_ocr_amd.my_model.model import _MISSING_STAGE, Modes, make_model_system, make_train_char_system
    for make, names in ((lambda **kw: make_model_system((1, 32, 48, 1), mode=Modes.TRAIN_LINE, **kw), ['ParagraphCrop', 'Line']),
                        (lambda **kw: make_train_char_system((1, 32, 16, 1), **kw), ['ParagraphCrop', 'LineCrop', 'CharLabel', 'Char'])):
        system, _, got = make()
        assert got == names and type(system.components[0].stage) is CropParagraphs, 'the default is unchanged'
        system, _, got = make(find_rotation=False)
        assert type(system.components[0].stage) is CropParagraphs
        system, _, got = make(find_rotation=True)
        assert got == names
        stage = system.components[0].stage
        assert type(stage) is CropAndRotateParagraphs and stage.find_rotation and stage.eps == 1.0
    with pytest.raises(ValueError, match='find_rotation'):
        make_model_system((1, 32, 48, 1), mode=Modes.TRAIN_PARAGRAPH, find_rotation=True)
    assert 'PredToText' in _MISSING_STAGE['PREDICT'] and 'find_rotation' not in _MISSING_STAGE['PREDICT']
    with pytest.raises(NotImplementedError, match='PredToText'):
        make_model_system((1, 32, 48, 1), mode=Modes.PREDICT)
