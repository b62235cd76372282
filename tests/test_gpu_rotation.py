"""Paragraph rotation on the GPU (csrc/rotate.hip) against the reference's results in tests/golden/rotation.npz and, at
sizes derived from the kernels' own band, block and launch sizes, against the NumPy restatement `rotate_rules` that
tests/test_rotation_host.py pins to that fixture and to scipy.

Extents are integers: equality.  Rotated crops: the device computes coordinates, weights and the four-term sum in
float64 for every dtype and rounds once, so |got - ref| <= 1e-12 + u * |ref| with u = 0 for float64, 2^-24 for float32 and
2^-11 for binary16 (plus 2^-25, half the spacing of its subnormals): one rounding of a double that equals the reference's
but for summation order (1e-12, tests/test_rotation_host.py).  Every companion is a multiple of 1/64, the same number in
every dtype.  Sources are NaN outside the box and outputs start as NaN: a NaN in a result is a read outside the box or an
element that was not written."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden
from test_rotation_host import (STAGE_PARAGRAPHS, compare_sampled, crop_rules, extent_rules, f64, probe_cases, rotation_cases,
                                stage_page)

pytestmark = pytest.mark.gpu

DTYPES = ('float64', 'float32', 'float16')
UNIT = {'float64': 0.0, 'float32': 2.0 ** -24, 'float16': 2.0 ** -11}
UNTOUCHED = -7                                                      # what an extent holds before the call


def bound(dtype):
    return lambda ref: 1e-12 + UNIT[dtype] * np.abs(ref) + (2.0 ** -25 if dtype == 'float16' else 0.0)


@pytest.fixture(scope='module')
def g():
    return load_golden('rotation')


@pytest.fixture
def rt():
    from univer_ocr_amd.nn import CP
    CP.use_gpu(0)
    CP.set_dtype('float32')
    return CP, CP.runtime()


def ints(values):
    return None if values is None else (C.c_int * len(values))(*[int(v) for v in values])


def doubles(values):
    return None if values is None else (C.c_double * len(values))(*[float(v) for v in values])


def pointers(values):
    return None if values is None else (C.c_void_p * len(values))(*values)


def flat(groups):
    return [v for group in groups for v in group]


# ---- uocr_rotated_extent -------------------------------------------------------------------------------------------------
def extent_arguments(labels_dev, probes):
    """probes: (label, box (y0, x0, h, w), angle) -> the arguments of uocr_rotated_extent as a dict of plain lists"""
    from univer_ocr_amd.nn.ops import rotation_geometry
    geometry = [rotation_geometry(box[2], box[3], angle) for _, box, angle in probes]
    n, h, w = labels_dev.shape
    return dict(labels=labels_dev.ptr, n=n, h=h, w=w, image_index=0, n_probes=len(probes),
                label_id=[k for k, _, _ in probes], box=flat(box for _, box, _ in probes),
                matrix=flat(M.reshape(-1) for M, _, _ in geometry), offset=flat(offset for _, offset, _ in geometry),
                out_shape=flat(shape for _, _, shape in geometry))


def raw_extent(runtime, extent_ptr, labels, n, h, w, image_index, n_probes, label_id, box, matrix, offset, out_shape):
    runtime.call('uocr_rotated_extent', labels, n, h, w, image_index, n_probes, ints(label_id), ints(box), doubles(matrix),
                 doubles(offset), ints(out_shape), extent_ptr)


def extents_of(rt, labels, probes):
    """ONE uocr_rotated_extent call on the (H, W) labels; the extents start as UNTOUCHED"""
    CP, runtime = rt
    labels_dev = CP.copy(labels[None].astype(np.int32), np.int32)
    extent = CP.copy(np.full((len(probes), 4), UNTOUCHED, np.int32), np.int32)
    raw_extent(runtime, extent.ptr, **extent_arguments(labels_dev, probes))
    return CP.asnumpy(extent)


def check_extents(rt, labels, probes, what):
    got = extents_of(rt, labels, probes)
    for i, (k, (y, x, h, w), angle) in enumerate(probes):
        expected = extent_rules(labels[y:y + h, x:x + w] == k, angle)
        assert tuple(got[i]) == expected, f'{what} probe {i}: label {k}, box {h} x {w} at ({y}, {x}), angle {angle}: {tuple(got[i])} != {expected}'
    return got


def one_page(g):
    """both pages of fixture (a) side by side as ONE page of labels (the second page's labels follow the first's) ->
    labels (H, W), [(label, box, angle)], expected extents"""
    cases = list(probe_cases(g))
    pages = {int(g[f'probe/{name}/page']): labels for name, labels, *_ in cases}
    labels = np.zeros((max(p.shape[0] for p in pages.values()), pages[0].shape[1] + pages[1].shape[1]), np.int32)
    labels[:pages[0].shape[0], :pages[0].shape[1]] = pages[0]
    labels[:pages[1].shape[0], pages[0].shape[1]:] = np.where(pages[1] > 0, pages[1] + pages[0].max(), 0)
    probes, expected = [], []
    for name, _, k, (y, x, h, w), angles, extents, _ in cases:
        second = int(g[f'probe/{name}/page']) == 1
        box = (y, x + pages[0].shape[1] * second, h, w)
        probes += [(k + int(pages[0].max()) * second, box, float(angle)) for angle in angles]
        expected += [tuple(e) for e in extents]
    return labels, probes, expected


def test_all_probes_of_the_fixture_in_one_call(g, rt):
    labels, probes, expected = one_page(g)
    got = extents_of(rt, labels, probes)
    wrong = [(i, probes[i], tuple(got[i]), expected[i]) for i in range(len(probes)) if tuple(got[i]) != expected[i]]
    assert not wrong, f'{len(wrong)} of {len(probes)} extents differ from the reference\'s, the first: {wrong[:3]}'
    band, _, per_launch, launches = rt[1].last_rotate()
    assert len(probes) == 34 * len(list(probe_cases(g))) >= 340 and launches == 2 * -(-len(probes) // per_launch) and band >= 1


@pytest.fixture
def sizes(rt):
    """(output rows per block of a probe, output pixels per block of an entry, probes / entries per launch)"""
    labels = np.zeros((6, 9), np.int32)
    labels[1:4, 2:7] = 1
    check_extents(rt, labels, [(1, (1, 2, 3, 5), 30.0)], 'sizes')
    band, block, per_launch, launches = rt[1].last_rotate()
    assert band >= 1 and block >= 64 and per_launch > 1 and launches == 2
    return band, block, per_launch


def test_extents_at_sizes_around_the_band_and_the_launch(sizes, rt):
    """a probe of at least three row bands whose width is no multiple of 64; more probes than one launch takes (the
    speck, repeated); probes without a set pixel; labels that touch the borders of their page"""
    band, _, per_launch = sizes
    r = np.random.default_rng(420)
    h, w = 3 * band + 1, 70
    labels = np.zeros((h + 4, w + 12), np.int32)
    labels[:h, :w] = np.where(r.random((h, w)) < 0.3, 1, 0)
    labels[0, :w] = labels[h - 1, :w] = 1
    labels[:h, 0] = labels[:h, w - 1] = 1
    labels[h + 1:h + 4, w + 1:w + 6] = 2                                # the speck, 3 x 5, in the page's last rows
    labels[h + 1:h + 2, 3:10] = 3                                       # a 1 x 7 bar
    big, speck, bar = (0, 0, h, w), (h + 1, w + 1, 3, 5), (h + 1, 3, 1, 7)
    probes = [(1, big, angle) for angle in (0.0, 12.5, 45.0, 77.7, 90.0, 133.3, 179.0, 180.0)]
    probes += [(2, speck, float(angle)) for angle in r.uniform(0, 180, per_launch + 1)]
    probes += [(3, bar, 30.0), (3, bar, 0.0), (7, big, 20.0), (2, big, 45.0)]
    got = check_extents(rt, labels, probes, 'sizes')
    assert rt[1].last_rotate()[3] == 2 * -(-len(probes) // per_launch)
    assert got[0][1] - got[0][0] >= 3 * band and (got[0][3] - got[0][2]) % 64
    assert tuple(got[-2]) == (0, 0, 0, 0) and tuple(got[-1]) == (0, 0, 0, 0), 'no pixel with that label in the box'
    again = extents_of(rt, labels, probes)
    assert again.tobytes() == got.tobytes()


def test_extent_argument_errors_write_nothing(rt):
    from univer_ocr_amd.hip import HipError
    CP, runtime = rt
    labels = np.zeros((12, 20), np.int32)
    labels[2:9, 3:15] = 1
    labels_dev = CP.copy(labels[None], np.int32)
    extent = CP.copy(np.full((2, 4), UNTOUCHED, np.int32), np.int32)
    good = extent_arguments(labels_dev, [(1, (2, 3, 7, 12), 33.0), (1, (2, 3, 7, 12), 120.0)])
    bad = [dict({name: None}) for name in ('labels', 'label_id', 'box', 'matrix', 'offset', 'out_shape')] + [
        dict(n_probes=-1), dict(n=0), dict(h=0), dict(w=0), dict(image_index=1), dict(image_index=-1), dict(label_id=[1, 0]),
        dict(box=[2, 3, 7, 12, -1, 3, 7, 12]), dict(box=[2, 3, 7, 12, 2, -3, 7, 12]), dict(box=[2, 3, 7, 12, 2, 3, 11, 12]),
        dict(box=[2, 3, 7, 18, 2, 3, 7, 12]), dict(box=[2, 3, 0, 12, 2, 3, 7, 12]), dict(box=[2, 3, 7, 12, 2, 3, 7, -1]),
        dict(out_shape=good['out_shape'][:3] + [0]), dict(out_shape=[-5] + good['out_shape'][1:]),
        dict(matrix=good['matrix'][:5] + [float('nan')] + good['matrix'][6:]), dict(offset=[float('inf')] + good['offset'][1:])]
    for change in bad:
        with pytest.raises(HipError, match=r'\(-1\)'):
            raw_extent(runtime, extent.ptr, **dict(good, **change))
        assert (CP.asnumpy(extent) == UNTOUCHED).all(), f'{change}: an extent was touched'
    with pytest.raises(HipError, match=r'\(-1\)'):
        raw_extent(runtime, None, **good)
    before = runtime.last_rotate()
    raw_extent(runtime, extent.ptr, **dict(good, n_probes=0))          # nothing to do: OK, no launch
    assert (CP.asnumpy(extent) == UNTOUCHED).all() and runtime.last_rotate() == before
    raw_extent(runtime, extent.ptr, **good)
    assert [tuple(e) for e in CP.asnumpy(extent)] == [extent_rules(labels[2:9, 3:15] == 1, a) for a in (33.0, 120.0)]


# ---- uocr_rotate_crop ----------------------------------------------------------------------------------------------------
NAMES = ('image', 'labels', 'dims', 'image_index', 'label_id', 'box', 'matrix', 'offset', 'plane', 'region', 'out', 'out_shape')
KINDS = dict(image=pointers, labels=pointers, out=pointers, matrix=doubles, offset=doubles)


def raw_crop(runtime, dtype, n_entries, **arrays):
    from univer_ocr_amd.hip import lib as hiplib
    runtime.call('uocr_rotate_crop', dtype if isinstance(dtype, int) else hiplib.dtype_code(dtype), n_entries,
                 *[KINDS.get(name, ints)(arrays[name]) for name in NAMES])


def out_shape_of(region, divisible_by):
    rh, rw = region[1] - region[0], region[3] - region[2]
    if divisible_by is None:
        return rh, rw
    return rh + divisible_by[0] - rh % divisible_by[0], rw + divisible_by[1] - rw % divisible_by[1]


def crop_arguments(entries, images_dev, labels_dev, outs, divisible_by):
    """entries: (image (1, H, W, c), labels (H, W), label, box, angle, region (y0, y1, x0, x1))"""
    from univer_ocr_amd.nn.ops import rotation_geometry
    geometry = [rotation_geometry(e[3][2], e[3][3], e[4]) for e in entries]
    return dict(n_entries=len(entries), image=[a.ptr for a in images_dev], labels=[a.ptr for a in labels_dev],
                dims=flat(e[0].shape for e in entries), image_index=[0] * len(entries), label_id=[e[2] for e in entries],
                box=flat(e[3] for e in entries), matrix=flat(M.reshape(-1) for M, _, _ in geometry),
                offset=flat(offset for _, offset, _ in geometry), plane=flat(shape for _, _, shape in geometry),
                region=flat((y0, x0, y1 - y0, x1 - x0) for *_, (y0, y1, x0, x1) in entries), out=[a.ptr for a in outs],
                out_shape=flat(out_shape_of(e[5], divisible_by) for e in entries))


def only_the_box(image, box):
    """the image with NaN everywhere outside the box"""
    y, x, h, w = box
    out = np.full(image.shape, np.nan)
    out[:, y:y + h, x:x + w] = image[:, y:y + h, x:x + w]
    return out


def crops_of(rt, entries, dtype, divisible_by=None):
    """ONE uocr_rotate_crop call; every source is NaN outside its box and every output starts as NaN"""
    CP, runtime = rt
    label_arrays = {}
    for e in entries:
        if id(e[1]) not in label_arrays:
            label_arrays[id(e[1])] = CP.copy(e[1][None].astype(np.int32), np.int32)
    images_dev = [CP.copy(only_the_box(e[0], e[3]), dtype) for e in entries]
    outs = [CP.copy(np.full((1, *out_shape_of(e[5], divisible_by), e[0].shape[3]), np.nan), dtype) for e in entries]
    raw_crop(runtime, dtype, **crop_arguments(entries, images_dev, [label_arrays[id(e[1])] for e in entries], outs, divisible_by))
    return [CP.asnumpy(a) for a in outs]


def with_regions(entries):
    """(image, labels, label, box, angle) -> with the region of the rotated mask"""
    return [(image, labels, k, box, angle, extent_rules(labels[box[0]:box[0] + box[2], box[1]:box[1] + box[3]] == k, angle))
            for image, labels, k, box, angle in entries]


def check_crops(rt, entries, dtype, divisible_by=None, what=''):
    got = crops_of(rt, entries, dtype, divisible_by)
    for i, ((image, labels, k, box, angle, region), out) in enumerate(zip(entries, got)):
        expected = crop_rules(image, labels, k, box, angle, divisible_by, region)
        where = f'{what} entry {i}: label {k}, box {box}, angle {angle}, region {region}, c = {image.shape[3]}, {dtype}'
        assert out.dtype == np.dtype(dtype), where
        compare_sampled(out, expected, 1, bound(dtype), where)
    return got


@pytest.mark.parametrize('divisible_by', [None, (16, 16)])
@pytest.mark.parametrize('dtype', DTYPES)
def test_rotated_crops_equal_the_reference(dtype, divisible_by, g, rt):
    """every mask, channel count and angle of fixture (b) in ONE call"""
    cases = list(rotation_cases(g))
    entries = with_regions([(image, labels, k, box, angle) for _, _, labels, k, box, angle, image, _, _ in cases])
    got = crops_of(rt, entries, dtype, divisible_by)
    per_launch, launches = rt[1].last_rotate()[2:]
    assert launches == -(-len(entries) // per_launch)
    for out, entry, (name, c, *_, angle, _, expected, stride) in zip(got, entries, cases):
        what = f'{name} c={c} at {angle} {dtype}'
        assert out.dtype == np.dtype(dtype) and out.shape == (1, *out_shape_of(entry[5], divisible_by), c), what
        if divisible_by is None:
            compare_sampled(out, expected, stride, bound(dtype), what)
        else:
            rh, rw = entry[5][1] - entry[5][0], entry[5][3] - entry[5][2]
            py, px = (out.shape[1] - rh) // 2, (out.shape[2] - rw) // 2
            inner = out[:, py:py + rh, px:px + rw]
            compare_sampled(inner, expected, stride, bound(dtype), what + ' framed')
            frame = out.copy()
            frame[:, py:py + rh, px:px + rw] = 0
            assert not frame.any() and not np.isnan(frame).any(), what + ': the frame is zero'


def test_python_wrappers_allocate_and_return_device_arrays(g, rt):
    from univer_ocr_amd.nn import ops
    CP, _ = rt
    name, labels, k, box, angles, extents, _ = next(case for case in probe_cases(g) if case[0] == 'ring')
    table = np.zeros((1, 8, 8), np.int64)
    for i in range(1, int(labels.max()) + 1):
        ys, xs = np.nonzero(labels == i)
        table[0, i - 1] = [0, len(ys), ys.min(), ys.max() + 1, xs.min(), xs.max() + 1, ys.sum(), xs.sum()]
    components = ops.Components(CP.copy(labels[None], np.int32), CP.copy(table, np.int64),
                                CP.copy(np.array([labels.max()], np.int32), np.int32), 8)
    got = ops.rotated_extent(components, 0, [(k, float(a)) for a in angles])
    assert got.dtype == np.int32 and np.array_equal(got, extents)
    assert ops.rotated_extent(components, 0, []).shape == (0, 4) and ops.rotate_crop([]) == []
    image = f64(g['rot/ring/img2'])
    angle = float(g['rot/ring/angles'][0])
    region = extent_rules(labels[box[0]:box[0] + box[2], box[1]:box[1] + box[3]] == k, angle)
    for dtype in DTYPES:
        dev = CP.copy(image, dtype)
        for divisible_by in (None, (16, 16)):
            out, = ops.rotate_crop([(dev, components, 0, k, angle, region)], divisible_by)
            assert out.dtype == np.dtype(dtype)
            compare_sampled(CP.asnumpy(out), crop_rules(image, labels, k, box, angle, divisible_by), 1, bound(dtype), f'{dtype} {divisible_by}')
    with pytest.raises(ValueError, match='rotated plane'):
        ops.rotate_crop([(dev, components, 0, k, angle, (0, 99, 0, 3))])
    with pytest.raises(ValueError, match='components 1'):
        ops.rotated_extent(components, 0, [(int(labels.max()) + 1, 10.0)])


def random_image(r, h, w, c):
    return r.integers(0, 64, (1, h, w, c)) / 64.0


def test_crops_at_sizes_around_the_block_and_the_launch(sizes, rt):
    """an entry of several blocks; more entries than one launch takes; regions of 1 x 1; 1, 2, 3 and 4 channels mixed in
    one call; boxes that touch the borders of their page"""
    _, block, per_launch = sizes
    r = np.random.default_rng(421)
    side = int(np.sqrt(3 * block)) + 3
    labels = np.zeros((side + 9, side + 14), np.int32)
    labels[:side, :side + 5] = np.where(r.random((side, side + 5)) < 0.7, 1, 0)
    labels[0, :side + 5] = labels[side - 1, :side + 5] = labels[:side, 0] = labels[:side, side + 4] = 1
    labels[side + 2:side + 9, side + 6:side + 14] = np.where(r.random((7, 8)) < 0.6, 2, 5)
    labels[side + 2, side + 6:side + 14] = labels[side + 8, side + 6:side + 14] = 2
    labels[side + 2:side + 9, side + 6] = labels[side + 2:side + 9, side + 13] = 2
    big, small = (0, 0, side, side + 5), (side + 2, side + 6, 7, 8)
    images = {c: random_image(r, *labels.shape, c) for c in (1, 2, 3, 4)}
    entries = with_regions([(images[c], labels, 1, big, angle) for c, angle in ((1, 31.0), (4, 90.0), (2, 147.3), (3, 0.0))] +
                           [(images[1 + i % 4], labels, 2, small, float(angle)) for i, angle in enumerate(r.uniform(1, 179, per_launch + 1))])
    assert (entries[0][5][1] - entries[0][5][0]) * (entries[0][5][3] - entries[0][5][2]) > 3 * block
    # regions of one pixel: a corner of the rotated mask's extent and a pixel inside it
    y0, y1, x0, x1 = entries[2][5]
    entries += [entries[2][:5] + ((y0, y0 + 1, x0, x0 + 1),), entries[2][:5] + (((y0 + y1) // 2, (y0 + y1) // 2 + 1, (x0 + x1) // 2, (x0 + x1) // 2 + 1),)]
    for dtype in DTYPES:
        check_crops(rt, entries, dtype, what='sizes')
        assert rt[1].last_rotate()[3] == -(-len(entries) // per_launch)
    got = check_crops(rt, entries, 'float32', (16, 16), what='framed')
    assert got[-1].shape == (1, 16, 16, 2)
    check_crops(rt, entries[:per_launch], 'float16', (5, 3), what='exactly one launch')
    assert rt[1].last_rotate()[3] == 1
    again = crops_of(rt, entries, 'float32', (16, 16))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))


def test_crop_argument_errors_write_nothing(rt):
    from univer_ocr_amd.hip import HipError
    from univer_ocr_amd.nn.ops import rotation_geometry
    CP, runtime = rt
    r = np.random.default_rng(422)
    labels = np.zeros((12, 20), np.int32)
    labels[2:9, 3:15] = 1
    box = (2, 3, 7, 12)
    entries = with_regions([(random_image(r, 12, 20, 3), labels, 1, box, angle) for angle in (33.0, 120.0)])
    images_dev = [CP.copy(e[0], np.float32) for e in entries]
    labels_dev = CP.copy(labels[None], np.int32)
    outs = [CP.copy(np.full((1, *out_shape_of(e[5], (16, 16)), 3), np.nan), np.float32) for e in entries]
    good = crop_arguments(entries, images_dev, [labels_dev] * 2, outs, (16, 16))
    plane = rotation_geometry(7, 12, 120.0)[2]
    second = lambda name, values: good[name][:len(good[name]) // 2] + list(values)
    bad = [dict({name: None}) for name in NAMES] + [
        dict(n_entries=-1), dict(image=[images_dev[0].ptr, None]), dict(labels=[None, labels_dev.ptr]), dict(out=[outs[0].ptr, None]),
        dict(image=[images_dev[0].ptr, images_dev[1].ptr + 2]), dict(out=[outs[0].ptr + 2, outs[1].ptr]),
        dict(labels=[labels_dev.ptr, labels_dev.ptr + 2]),
        dict(dims=second('dims', (0, 12, 20, 3))), dict(dims=second('dims', (1, 12, 20, 0))), dict(dims=second('dims', (1, 8, 20, 3))),
        dict(dims=second('dims', (1, 12, 14, 3))), dict(image_index=[0, 1]), dict(image_index=[-1, 0]), dict(label_id=[1, 0]),
        dict(box=second('box', (-1, 3, 7, 12))), dict(box=second('box', (2, 3, 0, 12))), dict(box=second('box', (2, 3, 7, 18))),
        dict(box=second('box', (6, 3, 7, 12))), dict(plane=second('plane', (0, plane[1]))), dict(plane=second('plane', (plane[0], 2))),
        dict(region=second('region', (0, 0, plane[0] + 1, 1))), dict(region=second('region', (plane[0], 0, 1, 1))),
        dict(region=second('region', (0, -1, 1, 1))), dict(region=second('region', (0, 0, 0, 1))), dict(region=second('region', (0, 1, 1, plane[1]))),
        dict(out_shape=second('out_shape', (good['region'][6] - 1, good['out_shape'][3]))),
        dict(out_shape=second('out_shape', (good['out_shape'][2], good['region'][7] - 1))),
        dict(matrix=second('matrix', (float('nan'), 0, 0, 1))), dict(offset=second('offset', (0.0, float('-inf'))))]
    for change in bad:
        with pytest.raises(HipError, match=r'\(-1\)'):
            raw_crop(runtime, 'float32', **dict(good, **change))
        for a in outs:
            assert np.isnan(CP.asnumpy(a)).all(), f'{change}: an output was touched'
    with pytest.raises(HipError, match=r'\(-2\)'):
        raw_crop(runtime, 7, **good)
    assert all(np.isnan(CP.asnumpy(a)).all() for a in outs)
    before = runtime.last_rotate()
    raw_crop(runtime, 'float32', **dict(good, n_entries=0))            # nothing to do: OK, no launch
    raw_crop(runtime, 'float32', n_entries=0, **{name: None for name in NAMES})
    assert all(np.isnan(CP.asnumpy(a)).all() for a in outs) and runtime.last_rotate() == before
    raw_crop(runtime, 'float32', **good)
    for e, a in zip(entries, outs):
        compare_sampled(CP.asnumpy(a), crop_rules(*e[:5], (16, 16)), 1, bound('float32'), 'after the errors')


# ---- fixture (c): CropAndRotateParagraphs --------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_stage_equals_the_reference(dtype, g, rt, monkeypatch):
    """the page of four paragraphs: the reference's angles (==, None where it says None), its crops in the 16-frame, 14
    extent calls and one crop launch; the upright paragraph and find_rotation=False equal CropParagraphs"""
    from univer_ocr_amd.my_model.crop import CropAndRotateParagraphs, CropParagraphs
    CP, runtime = rt
    paragraph, arrays, _, _, angles = stage_page(g)
    mask = CP.copy(paragraph, dtype)
    dev = [CP.copy(a, dtype) for a in arrays]
    stage = CropAndRotateParagraphs()
    calls = []
    original = runtime.call
    monkeypatch.setattr(runtime, 'call', lambda name, *args: (calls.append(name), original(name, *args))[1])
    result = stage(mask, dev, divisible_by=(16, 16))
    monkeypatch.undo()
    assert calls.count('uocr_rotated_extent') == 14 and calls.count('uocr_rotate_crop') == 1
    assert runtime.last_rotate()[3] == 1, 'one crop launch for the page'
    assert stage.angles == angles
    plain = CropParagraphs()(mask, dev, divisible_by=(16, 16))
    assert len(result) == 2 and all(len(per_array) == STAGE_PARAGRAPHS for per_array in result)
    for c, per_array, per_array_plain in zip((1, 2), result, plain):
        for p, crop in enumerate(per_array):
            got = CP.asnumpy(crop)
            assert got.dtype == np.dtype(dtype)
            compare_sampled(got, g[f'stage/{p}/c{c}'], 1, bound(dtype), f'paragraph {p} c={c} {dtype}')
            if angles[p] is None:
                assert np.array_equal(got, CP.asnumpy(per_array_plain[p])), f'paragraph {p} c={c}: the upright crop'
    for divisible_by in (None, (16, 16)):
        unrotated = CropAndRotateParagraphs(find_rotation=False)(mask, dev, divisible_by=divisible_by)
        for per_array, per_array_plain in zip(unrotated, CropParagraphs()(mask, dev, divisible_by=divisible_by)):
            assert len(per_array) == STAGE_PARAGRAPHS
            for a, b in zip(per_array, per_array_plain):
                assert np.array_equal(CP.asnumpy(a), CP.asnumpy(b))


def test_train_line_system_files_the_rotated_crops(g, rt):
    """[ParagraphCrop, Line] built with find_rotation=True on the page of fixture (c): one Line step per paragraph on the
    reference's rotated crops"""
    from univer_ocr_amd.my_model.crop import CropAndRotateParagraphs
    from univer_ocr_amd.my_model.model import Modes, make_context_maker, make_model_system
    from univer_ocr_amd.nn.optimizers import Momentum
    CP, _ = rt
    paragraph, arrays, _, _, angles = stage_page(g)
    layers = {'monochrome': arrays[0], 'paragraph': paragraph, 'line': arrays[1]}
    system, models, names = make_model_system((1, 16, 48, 1), Momentum(lr=0.01, momentum=0), mode=Modes.TRAIN_LINE, find_rotation=True)
    assert names == ['ParagraphCrop', 'Line'] and type(system.components[0].stage) is CropAndRotateParagraphs
    context = make_context_maker(Modes.TRAIN_LINE)(lambda layer_tags: {tag: layers[tag] for tag in layer_tags})
    system.train(context)
    assert system.components[0].stage.angles == angles
    for key, c in (('cropped_monochrome', 1), ('cropped_line', 2)):
        assert len(context[key]) == STAGE_PARAGRAPHS
        for p in range(STAGE_PARAGRAPHS):
            compare_sampled(CP.asnumpy(context[key][p]), g[f'stage/{p}/c{c}'], 1, bound('float32'), f'{key}[{p}]')
    assert len(context['line_pred']) == STAGE_PARAGRAPHS and len(context['losses']['Line']['output_losses']) == STAGE_PARAGRAPHS
    for p, pred in enumerate(context['line_pred']):
        assert pred.shape == g[f'stage/{p}/c2'].shape and np.isfinite(CP.asnumpy(pred)).all()
