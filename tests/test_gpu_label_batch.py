"""Batched connected components on the GPU (csrc/label_batch.hip): a LIST of images of different sizes, each one channel
of an interleaved tensor, in one call -- against the NumPy flood fill that tests/test_label_host.py pins to the
reference's fixture and tests/test_label_batch_host.py to scipy on strided channel views, and against
uocr_label_components on the channel copied out.  Sizes come from the call's own tile and group size
(last_label_batch).  Everything is exact: labels, counts and tables are integers, crops are compared bit for bit.  Inputs
are multiples of 1/64, so every float64 sum is exact in any order and the device's threshold is the host's bit for bit;
every value also keeps 1/128 clear of its entry's threshold, except in a 1 x 1 entry, whose mean IS its value (nothing
is above it: the entry is background under 'mean' and 'mean_max').  The two model systems run against the reference's
nets with SYSTEM_TOL of tests/test_gpu_label.py."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden, rel_linf
from test_gpu_bounds import GUARD, SENTINEL, Guarded
from test_gpu_label import SYSTEM_TOL, label_raw, serpentine, spiral, staircase, u_shapes
from test_label_host import RULES, flood_fill, threshold_of
from test_line_crop_host import LINES_OF_THE_PAGE, STAGE_NAMES, f64, stage_lines

pytestmark = pytest.mark.gpu

DTYPES = ('float32', 'float64', 'float16')
MODES = {'mean': 0, 'mean_max': 1, 'value': 2}
VALUE_T = 69 / 128               # 1/128 from every multiple of 1/64
FILL = -7


@pytest.fixture(scope='module')
def g():
    return load_golden('line_crop')


@pytest.fixture
def rt():
    from univer_ocr_amd.nn import CP
    CP.use_gpu(0)
    CP.set_dtype('float32')
    return CP, CP.runtime()


def pointers(values):
    return (C.c_void_p * len(values))(*values)


def ints(values):
    return (C.c_int * len(values))(*[int(v) for v in values])


def raw_call(runtime, dtype, x, h, w, c, channel, mode, value, labels, table, max_components, count, n=None):
    """uocr_label_batch on device pointers; `labels` is a list of pointers (None entries allowed) or None"""
    from univer_ocr_amd.hip import lib as hiplib
    runtime.call('uocr_label_batch', hiplib.dtype_code(np.dtype(dtype)), len(h) if n is None else n,
                 None if x is None else pointers(x), ints(h), ints(w), ints(c), ints(channel), mode, float(value),
                 None if labels is None else pointers(labels), table, max_components, count)


def batch_raw(rt, entries, rule='value', value=VALUE_T, max_components=64, dtype='float32', want_labels=True, dev=None):
    """entries: [(host array (1, H, W, C), channel)] -> labels [(H, W)] (or None), table (n, max, 8), count (n,); every
    output is filled with FILL first.  dev: the device arrays of an earlier call, to save the copies."""
    CP, runtime = rt
    dev = [CP.copy(x, dtype) for x, _ in entries] if dev is None else dev
    shapes = [x.shape for x, _ in entries]
    labels = [CP.full(s[1:3], FILL, np.int32) for s in shapes] if want_labels else None
    table = CP.full((len(entries), max_components, 8), FILL, np.int64)
    count = CP.full((len(entries),), FILL, np.int32)
    raw_call(runtime, dtype, [a.ptr for a in dev], [s[1] for s in shapes], [s[2] for s in shapes], [s[3] for s in shapes],
             [ch for _, ch in entries], MODES[rule], value, [a.ptr for a in labels] if want_labels else None, table.ptr,
             max_components, count.ptr)
    return [CP.asnumpy(a) for a in labels] if want_labels else None, CP.asnumpy(table), CP.asnumpy(count)


def check_entry(i, labels, table, count, expected, what=''):
    exp_labels, exp_table = expected
    assert count[i] == len(exp_table), f'{what} entry {i}: count {count[i]} != {len(exp_table)}'
    if labels is not None:
        assert np.array_equal(labels[i], exp_labels), f'{what} entry {i}: labels differ'
    rows = min(len(exp_table), table.shape[1])
    assert np.array_equal(table[i, :rows], exp_table[:rows]), f'{what} entry {i}: table differs'
    assert not table[i, rows:].any(), f'{what} entry {i}: rows past the count are not zero'


def mask_tensor(*masks):
    """(1, H, W, C) float64 with the boolean masks as channels"""
    return np.stack([np.asarray(m, np.float64) for m in masks], axis=-1)[None]


@pytest.fixture
def sizes(rt):
    """(TH, TW, E, (H, W) = (2 TH + 3, 2 TW + 5): two full tiles and a ragged one each way)"""
    batch_raw(rt, [(np.ones((1, 4, 4, 1)), 0)])
    th, tw, entries, launches = rt[1].last_label_batch()
    assert th > 0 and tw > 0 and entries >= 32 and launches > 0
    return th, tw, entries, (2 * th + 3, 2 * tw + 5)


# ---- mixed entries in one call ---------------------------------------------------------------------------------------------
def margin(x, rule):
    return float(np.min(np.abs(x - threshold_of(x, rule, VALUE_T))))


def clear_channel(rng, h, w, scale):
    """multiples of scale / 64 in a low and a high cluster whose mean and (mean + max) / 2 keep 1 / 128 clear of every value"""
    if h * w == 1:
        return np.full((1, 1), scale * int(rng.integers(1, 65)) / 64)
    while True:
        high = rng.random((h, w)) < rng.uniform(0.3, 0.6)
        x = scale * np.where(high, rng.integers(56, 65, (h, w)), rng.integers(0, 17, (h, w))) / 64
        if all(margin(x, rule) >= 1 / 128 for rule in RULES):
            return x


_MIXED = {}


def mixed_entries(th, tw):
    """every channel of tensors of 1, 2 and 3 channels at the five sizes; channel j holds multiples of 2^j / 64, so no
    channel shares its statistics with its neighbours.  Made once, with the flood fills per rule."""
    if (th, tw) not in _MIXED:
        rng = np.random.default_rng(31)
        entries = []
        for h, w in ((1, 1), (1, tw + 1), (th + 1, 1), (th, tw), (2 * th + 3, 2 * tw + 5)):
            for c in (1, 2, 3):
                x = np.stack([clear_channel(rng, h, w, 2 ** j) for j in range(c)], axis=-1)[None]
                entries += [(x, channel) for channel in range(c)]
        expected = {}
        for rule in RULES:
            for x, channel in entries:
                plane = x[0, :, :, channel]
                if plane.size > 1:
                    assert margin(plane, rule) >= 1 / 128
                else:
                    assert rule == 'value' or threshold_of(plane, rule) == plane[0, 0]
            expected[rule] = [flood_fill(x[0, :, :, ch] > threshold_of(x[0, :, :, ch], rule, VALUE_T)) for x, ch in entries]
        _MIXED[th, tw] = entries, expected
    return _MIXED[th, tw]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('rule', RULES)
def test_mixed_entries_in_one_call(rule, dtype, sizes, rt):
    th, tw, _, _ = sizes
    entries, expected = mixed_entries(th, tw)
    for x, _ in entries:
        assert np.array_equal(x.astype(dtype).astype(np.float64), x), 'the values are exact in every dtype'
    labels, table, count = batch_raw(rt, entries, rule, dtype=dtype, max_components=1024)
    assert rt[1].last_label_batch()[3] == (6 if rule == 'value' else 7), 'one chain for the call'
    for i, exp in enumerate(expected[rule]):
        check_entry(i, labels, table, count, exp, f'{rule}/{dtype}')
    assert len({len(t) for _, t in expected[rule]}) > 3, 'the entries hold different numbers of components'


# ---- the hard shapes ----------------------------------------------------------------------------------------------------------
def corners(h, w):
    m = np.zeros((h, w), bool)
    m[0, 0] = m[0, -1] = m[-1, 0] = m[-1, -1] = True
    return m


def test_hard_shapes_as_channels_of_one_call(sizes, rt):
    """every shape is channel 0 of one tensor and channel 1 of another, whose other channel is a different shape"""
    h, w = sizes[3]
    shapes = [f(h, w) for f in (serpentine, spiral, u_shapes, staircase, corners)]
    tensors = [mask_tensor(shapes[i], shapes[(i + 1) % 5]) for i in range(5)]
    entries = [(x, channel) for x in tensors for channel in (0, 1)]
    labels, table, count = batch_raw(rt, entries, 'value', 0.5)
    assert count.tolist() == [1, 1, 1, 4, 4, h, h, 4, 4, 1]
    for i, (x, channel) in enumerate(entries):
        mask = x[0, :, :, channel] > 0.5
        check_entry(i, labels, table, count, flood_fill(mask), 'shapes')
        one_labels, one_table, one_count = label_raw(rt, mask[None].astype(np.float32), 'value', 0.5, max_components=64)
        assert count[i] == one_count[0] and np.array_equal(labels[i], one_labels[0]) and np.array_equal(table[i], one_table[0])


# ---- per-entry statistics --------------------------------------------------------------------------------------------------------
def dots(values, h=8, w=8):
    """isolated pixels of the given values on a zero plane"""
    x = np.zeros((h, w))
    for i, v in enumerate(values):
        x[2 * (i // 3) + 1, 2 * (i % 3) + 1] = v
    return x


def test_thresholds_are_per_entry_and_per_channel(rt):
    a, b = dots([1.0, 1.0, 0.75, 0.75]), dots([0.25, 0.25, 0.0625, 0.0625])
    both = np.concatenate([a.reshape(-1), b.reshape(-1)])
    interleaved = np.stack([b, np.ones_like(b)], axis=-1)
    own = [flood_fill(x > threshold_of(x, 'mean_max')) for x in (a, b)]
    assert [len(t) for _, t in own] == [4, 2]
    for x in (a, b):
        assert margin(x, 'mean_max') >= 1 / 128
    # one threshold for the call, or one over all channels of the tensor, would lose b's components
    assert len(flood_fill(b > threshold_of(both, 'mean_max'))[1]) == 0
    assert len(flood_fill(b > threshold_of(interleaved, 'mean_max'))[1]) == 0
    assert min(np.min(np.abs(b - threshold_of(v, 'mean_max'))) for v in (both, interleaved)) >= 1 / 128
    entries = [(a[None, :, :, None], 0), (b[None, :, :, None], 0), (interleaved[None], 0), (interleaved[None], 1)]
    for dtype in DTYPES:
        labels, table, count = batch_raw(rt, entries, 'mean_max', dtype=dtype)
        assert count.tolist() == [4, 2, 2, 0], dtype
        for i, exp in enumerate([own[0], own[1], own[1], flood_fill(np.zeros_like(b))]):
            check_entry(i, labels, table, count, exp, dtype)


# ---- all-background and all-foreground entries between ordinary ones ---------------------------------------------------------
def test_empty_and_full_entries_between_ordinary_ones(sizes, rt):
    h, w = sizes[3]
    rng = np.random.default_rng(41)
    ordinary = [rng.random((h - i, w - 2 * i)) < 0.5 for i in range(3)]
    masks = [ordinary[0], np.zeros((h, w), bool), ordinary[1], np.ones((h, w), bool), ordinary[2]]
    entries = [(mask_tensor(m), 0) for m in masks]
    labels, table, count = batch_raw(rt, entries, 'value', 0.5, max_components=512)
    for i, m in enumerate(masks):
        check_entry(i, labels, table, count, flood_fill(m), 'between')
    assert count[1] == 0 and not labels[1].any() and not table[1].any()
    assert count[3] == 1 and (labels[3] == 1).all()
    assert table[3, 0].tolist() == [0, h * w, 0, h, 0, w, w * h * (h - 1) // 2, h * w * (w - 1) // 2]
    # under 'mean' a constant entry has nothing above its threshold
    labels, table, count = batch_raw(rt, entries, 'mean', max_components=512)
    assert count[1] == 0 and count[3] == 0 and not labels[3].any()
    for i in (0, 2, 4):
        check_entry(i, labels, table, count, flood_fill(masks[i]), 'between/mean')


# ---- more entries than one group ---------------------------------------------------------------------------------------------
def test_more_entries_than_one_group_takes(sizes, rt):
    CP, runtime = rt
    _, _, per_group, (h, w) = sizes
    rng = np.random.default_rng(43)
    masks = [rng.random((h, w) if i % 2 else (1, 1)) < 0.55 for i in range(per_group + 3)]
    entries = [(mask_tensor(m, ~m), 0) for m in masks]
    labels, table, count = batch_raw(rt, entries, 'mean', max_components=512)
    launches_more = runtime.last_label_batch()[3]
    for i, m in enumerate(masks):
        x = entries[i][0][0, :, :, 0]
        check_entry(i, labels, table, count, flood_fill(x > threshold_of(x, 'mean')), f'{per_group + 3} entries')
    one = [(mask_tensor(masks[1]), 0)]
    dev = [CP.copy(one[0][0], np.float32)]
    batch_raw(rt, one, 'mean', dev=dev, want_labels=False)
    launches_one = runtime.last_label_batch()[3]
    _, table, count = batch_raw(rt, one * per_group, 'mean', max_components=512, dev=dev * per_group, want_labels=False)
    launches_group = runtime.last_label_batch()[3]
    assert launches_one == launches_group == 7, 'the chain of a group does not grow with its entries'
    assert launches_group < launches_more <= 2 * launches_group
    exp = flood_fill(masks[1])
    for i in range(per_group):
        check_entry(i, None, table, count, exp, 'one entry, a group of times')


# ---- the table's capacity ----------------------------------------------------------------------------------------------------
def test_checkerboard_overflows_the_table_and_the_wrapper_asks_again(sizes, rt, monkeypatch):
    from univer_ocr_amd.hip import HipError
    from univer_ocr_amd.nn import ops
    CP, runtime = rt
    th = sizes[0]
    yy, xx = np.mgrid[:2 * th, :16]
    mask = (yy + xx) % 2 == 0
    exp_labels, exp_table = flood_fill(mask)
    assert len(exp_table) == 16 * th
    x = mask_tensor(mask)
    labels, table, count = batch_raw(rt, [(x, 0)], 'value', 0.5, max_components=8)
    assert count[0] == 16 * th, 'the count is the true number of components'
    assert np.array_equal(table[0], exp_table[:8]), 'the table holds the first max_components rows'
    assert np.array_equal(labels[0], exp_labels), 'the labels stay complete'
    calls = []
    original = runtime.call
    monkeypatch.setattr(runtime, 'call', lambda name, *args: (calls.append(name), original(name, *args))[1])
    small = mask_tensor(np.eye(5, dtype=bool))
    first, second = ops.label_batch([(CP.copy(x, np.float32), 0), (CP.copy(small, np.float32), 0)], 0.5, max_components=4096,
                                    cap=8, labels=True)
    assert calls.count('uocr_label_batch') == 2, 'one second call for the entry that holds more than cap'
    assert first.count == 16 * th and np.array_equal(first.table, exp_table) and np.array_equal(CP.asnumpy(first.labels), exp_labels)
    assert second.count == 5 and np.array_equal(second.table, flood_fill(np.eye(5, dtype=bool))[1])
    assert np.array_equal(first.boxes, exp_table[:, 2:6]) and np.array_equal(first.area, exp_table[:, 1])
    assert np.array_equal(first.center_of_mass, exp_table[:, 6:8] / exp_table[:, 1:2])
    with pytest.raises(HipError, match=f'{16 * th} components, more than max_components = 100'):
        ops.label_batch([(CP.copy(x, np.float32), 0)], 0.5, max_components=100, cap=8)


# ---- repeatability ------------------------------------------------------------------------------------------------------------
def test_second_call_after_a_larger_one_and_repeatability(sizes, rt):
    """stale workspace of larger entries must not leak into smaller ones; two calls give the same bytes"""
    h, w = sizes[3]
    rng = np.random.default_rng(47)
    big = [(mask_tensor(rng.random((3 * h, 2 * w)) < 0.6, rng.random((3 * h, 2 * w)) < 0.4), ch) for ch in (0, 1)]
    first = batch_raw(rt, big, 'mean', max_components=2048)
    small = [rng.random((h - 4, w - 9)) < 0.5, np.zeros((h - 4, w - 9), bool), rng.random((3, 5)) < 0.5]
    for want_labels in (True, False):
        labels, table, count = batch_raw(rt, [(mask_tensor(m), 0) for m in small], 'value', 0.5, max_components=512,
                                         want_labels=want_labels)
        for i, m in enumerate(small):
            check_entry(i, labels, table, count, flood_fill(m), 'small after big')
    again = batch_raw(rt, big, 'mean', max_components=2048)
    for a, b in zip(first[0], again[0]):
        assert np.array_equal(a, b)
    assert first[1].tobytes() == again[1].tobytes() and first[2].tobytes() == again[2].tobytes()
    for i, (x, ch) in enumerate(big):
        check_entry(i, first[0], first[1], first[2], flood_fill(x[0, :, :, ch] > threshold_of(x[0, :, :, ch], 'mean')), 'big')


def test_capture_and_replay(sizes, rt):
    """the call is asynchronous and capturable: a replayed graph labels what the buffers hold then"""
    import torch
    CP, runtime = rt
    h, w = sizes[3]
    rng = np.random.default_rng(49)
    versions = [[rng.random((h, w, 2)) < 0.55, rng.random((5, 7, 2)) < 0.5] for _ in range(2)]
    dev = [CP.copy(x[None].astype(np.float32), np.float32) for x in versions[0]]
    shapes = [(h, w), (5, 7)]
    labels = [CP.zeros(s, np.int32) for s in shapes]
    table, count = CP.zeros((2, 512, 8), np.int64), CP.zeros((2,), np.int32)
    with runtime.capture(torch.cuda.MemPool()) as graph:
        raw_call(runtime, 'float32', [a.ptr for a in dev], [h, 5], [w, 7], [2, 2], [1, 0], MODES['mean'], 0.0,
                 [a.ptr for a in labels], table.ptr, 512, count.ptr)
    for version in versions[::-1]:
        for a, x in zip(dev, version):
            a.set(x[None].astype(np.float32))
        graph.replay()
        host = [CP.asnumpy(a) for a in labels], CP.asnumpy(table), CP.asnumpy(count)
        for i, (x, ch) in enumerate(zip(version, (1, 0))):
            plane = x[:, :, ch].astype(np.float64)
            check_entry(i, *host, flood_fill(plane > threshold_of(plane, 'mean')), 'replay')
        eager = batch_raw(rt, [(x[None].astype(np.float64), ch) for x, ch in zip(version, (1, 0))], 'mean', max_components=512)
        assert all(np.array_equal(a, b) for a, b in zip(host[0], eager[0]))
        assert np.array_equal(host[1], eager[1]) and np.array_equal(host[2], eager[2])


# ---- bounds --------------------------------------------------------------------------------------------------------------------
def guarded_input(CP, x):
    buf = Guarded(CP, x.size)
    buf.buf.set(np.concatenate([np.full(GUARD, SENTINEL), x.reshape(-1), np.full(GUARD, SENTINEL)]).astype(np.float32))
    return buf


def test_everything_stays_inside_its_buffers(sizes, rt):
    """inputs and outputs sit between sentinel borders (tests/test_gpu_bounds.py); with NULL labels only table and
    count change"""
    CP, runtime = rt
    th, tw, _, (h, w) = sizes
    rng = np.random.default_rng(51)
    shapes = [(h, w, 2), (1, 1, 1), (th, tw, 3), (1, tw + 1, 2)]
    channels = [1, 0, 2, 0]
    masks = [rng.random(s) < 0.45 for s in shapes]
    max_components = 37
    expected = [flood_fill(m[:, :, ch] > threshold_of(m[:, :, ch], 'mean')) for m, ch in zip(masks, channels)]
    assert len(expected[0][1]) > max_components
    x = [guarded_input(CP, m.astype(np.float32)) for m in masks]
    for want_labels in (True, False):
        labels = [Guarded(CP, s[0] * s[1]) for s in shapes]
        table, count = Guarded(CP, 4 * max_components * 8 * 2), Guarded(CP, 4)
        raw_call(runtime, 'float32', [a.ptr for a in x], [s[0] for s in shapes], [s[1] for s in shapes], [s[2] for s in shapes],
                 channels, MODES['mean'], 0.0, [a.ptr for a in labels] if want_labels else None, table.ptr, max_components,
                 count.ptr)
        got_table = table.check('table').view(np.int64).reshape(4, max_components, 8)
        got_count = count.check('count').view(np.int32)
        got_labels = [a.check(f'labels {i}', expect_written=want_labels).view(np.int32).reshape(s[:2])
                      for i, (a, s) in enumerate(zip(labels, shapes))]
        if not want_labels:
            assert all((a == np.float32(SENTINEL).view(np.int32)).all() for a in got_labels), 'no labels were asked for'
        for a in x:
            a.check('x', expect_written=False)
        for i, exp in enumerate(expected):
            check_entry(i, got_labels if want_labels else None, got_table, got_count, exp, 'guarded')
    # some labels given, some not
    labels = [Guarded(CP, s[0] * s[1]) for s in shapes]
    table, count = Guarded(CP, 4 * max_components * 8 * 2), Guarded(CP, 4)
    raw_call(runtime, 'float32', [a.ptr for a in x], [s[0] for s in shapes], [s[1] for s in shapes], [s[2] for s in shapes],
             channels, MODES['mean'], 0.0, [labels[0].ptr, None, labels[2].ptr, None], table.ptr, max_components, count.ptr)
    for i in (0, 2):
        assert np.array_equal(labels[i].check(f'labels {i}').view(np.int32).reshape(shapes[i][:2]), expected[i][0])
    for i in (1, 3):
        labels[i].check(f'labels {i}', expect_written=False)
    got_table = table.check('table').view(np.int64).reshape(4, max_components, 8)
    for i, exp in enumerate(expected):
        check_entry(i, None, got_table, count.check('count').view(np.int32), exp, 'some labels')


def test_argument_errors_write_nothing(rt):
    from univer_ocr_amd.hip import HipError
    CP, runtime = rt
    h, w, c = 12, 20, 2
    x = [CP.copy(np.random.default_rng(53).random((1, h, w, c)), np.float32) for _ in range(2)]
    labels = [CP.full((h, w), FILL, np.int32) for _ in range(2)]
    table, count = CP.full((2, 4, 8), FILL, np.int64), CP.full((2,), FILL, np.int32)
    good = dict(x=[a.ptr for a in x], h=[h, h], w=[w, w], c=[c, c], channel=[0, 1], mode=0, labels=[a.ptr for a in labels],
                table=table.ptr, max_components=4, count=count.ptr, n=2)
    bad = [dict(x=None), dict(table=None), dict(count=None), dict(x=[x[0].ptr, None]), dict(x=[x[0].ptr, x[1].ptr + 2]),
           dict(labels=[labels[0].ptr, labels[1].ptr + 2]), dict(table=table.ptr + 4), dict(count=count.ptr + 2),
           dict(h=[h, 0]), dict(w=[-1, w]), dict(c=[c, 0]), dict(channel=[0, -1]), dict(channel=[c, 1]), dict(mode=3),
           dict(mode=-1), dict(max_components=-1), dict(n=-1)]
    for change in bad:
        a = dict(good, **change)
        with pytest.raises(HipError, match=r'\(-1\)'):
            raw_call(runtime, 'float32', a['x'], a['h'], a['w'], a['c'], a['channel'], a['mode'], 0.0, a['labels'], a['table'],
                     a['max_components'], a['count'], n=a['n'])
        for what, out in (('labels', labels[0]), ('labels', labels[1]), ('table', table), ('count', count)):
            assert (CP.asnumpy(out) == FILL).all(), f'{change}: {what} was touched'
    with pytest.raises(HipError, match=r'\(-2\)'):
        runtime.call('uocr_label_batch', 77, 2, pointers(good['x']), ints(good['h']), ints(good['w']), ints(good['c']),
                     ints(good['channel']), 0, 0.0, pointers(good['labels']), table.ptr, 4, count.ptr)
    # no entries: UOCR_OK, nothing launched, nothing looked at
    raw_call(runtime, 'float32', None, [], [], [], [], 0, 0.0, None, None, 4, None, n=0)
    assert (CP.asnumpy(table) == FILL).all() and (CP.asnumpy(count) == FILL).all()
    a = good
    raw_call(runtime, 'float32', a['x'], a['h'], a['w'], a['c'], a['channel'], a['mode'], 0.0, a['labels'], a['table'],
             a['max_components'], a['count'])
    assert (CP.asnumpy(count) > 0).all() and not (CP.asnumpy(labels[1]) == FILL).any()


# ---- CropLines(labelling='page') ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_crop_lines_by_page_equals_the_reference_on_the_stage_cases(dtype, g, rt):
    """all four paragraphs as ONE page: rotation, line order, shapes and arrays of both companions; one chain"""
    from univer_ocr_amd.my_model.crop import CropLines
    CP, runtime = rt
    one = np.zeros((1, 40, 70, 1))
    one[0, 3:30, 5:60] = 1.0
    batch_raw(rt, [(one, 0)], 'mean_max')
    one_group = runtime.last_label_batch()[3]
    masks = [CP.copy(f64(g[f'stage/{name}/mask']), dtype) for name in STAGE_NAMES]
    arrays = [[CP.copy(f64(g[f'stage/{name}/img{c}']), dtype) for name in STAGE_NAMES] for c in (1, 9)]
    crop_lines = CropLines(labelling='page')
    found = crop_lines.find_lines(masks)
    assert runtime.last_label_batch()[3] == one_group == 7, 'eight masks, the launches of one group'
    for name, (rotation, boxes) in zip(STAGE_NAMES, found):
        assert (rotation or 0) == int(g[f'stage/{name}/rotation']), name
        assert np.array_equal(np.array(boxes), g[f'stage/{name}/boxes']), name
    result = crop_lines(masks, arrays)
    assert runtime.last_line_crop()[3] == 1 and runtime.last_label_batch()[3] == one_group
    assert len(result) == 2 and all(len(per_array) == len(STAGE_NAMES) for per_array in result)
    for c, per_array in zip((1, 9), result):
        for name, lines in zip(STAGE_NAMES, per_array):
            expected = stage_lines(g, name, c)
            assert len(lines) == len(expected), name
            for l, (line, exp) in enumerate(zip(lines, expected)):
                got = CP.asnumpy(line)
                assert got.dtype == np.dtype(dtype) and got.shape == exp.shape, f'{name} c={c} line {l}'
                assert np.array_equal(got, exp.astype(dtype)), f'{name} c={c} line {l}'


def test_crop_lines_by_page_yields_no_lines_where_the_reference_raises(g, rt):
    """no top component, no bottom component, a flat mask: the paragraph stays empty, its neighbour keeps its lines"""
    from univer_ocr_amd.my_model.crop import CropLines
    CP, _ = rt
    mask = f64(g['stage/turned/mask'])
    no_top, no_bottom, flat = mask.copy(), mask.copy(), np.full(mask.shape, 0.5)
    no_top[..., 0], no_bottom[..., 1] = 1 / 64, 0.25
    image = f64(g['stage/turned/img9'])
    crop_lines = CropLines(labelling='page')
    result = crop_lines([CP.copy(m) for m in (no_top, mask, no_bottom, flat)], [[CP.copy(image) for _ in range(4)]])
    assert [len(lines) for lines in result[0]] == [0, 2, 0, 0]
    for line, exp in zip(result[0][1], stage_lines(g, 'turned', 9)):
        assert np.array_equal(CP.asnumpy(line), exp.astype(np.float32))
    assert crop_lines([], [[], []]) == [[], []]


# ---- the model systems -----------------------------------------------------------------------------------------------------------
def recorded_calls(runtime, monkeypatch):
    calls = []
    original = runtime.call
    monkeypatch.setattr(runtime, 'call', lambda name, *args: (calls.append(name), original(name, *args))[1])
    return calls


@pytest.mark.parametrize('opt_tag,dtype', [('sgd', 'float32'), ('sgd', 'float64'), ('adam', 'float64')])
def test_train_char_system_by_page_equals_the_reference(opt_tag, dtype, g, rt, monkeypatch):
    """[ParagraphCrop, LineCrop, CharLabel, Char] with line_labelling='page' on the page of fixture (c): the cropped lines
    and the labels equal the reference's exactly; losses, char_pred[p][l] and the weights after the three steps equal the
    reference Char net's to the tolerances of DESIGN 3"""
    from test_gpu_models import check_sampled, set_analytic_weights
    from univer_ocr_amd.my_model.model import make_train_char_context_maker, make_train_char_system
    from univer_ocr_amd.nn.optimizers import Adam, Momentum
    CP, runtime = rt
    CP.set_dtype(dtype)
    try:
        opt = Momentum(lr=0.01, momentum=0) if opt_tag == 'sgd' else Adam(lr=0.0015)
        system, models, names = make_train_char_system(g['system/mono0_0'].shape, opt, line_labelling='page')
        assert system.components[names.index('LineCrop')].stage.labelling == 'page'
        char = models['Char']
        set_analytic_weights(char)
        layers = {tag: f64(g[f'system/page/{tag}']) for tag in ('monochrome', 'paragraph', 'line', 'char')}
        context = make_train_char_context_maker()(lambda layer_tags: {tag: layers[tag] for tag in layer_tags})
        calls = recorded_calls(runtime, monkeypatch)
        system.train(context)
        monkeypatch.undo()
        assert calls.count('uocr_label_batch') == 1 and calls.count('uocr_label_components') == 1, 'the page; the line masks'
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


def test_predict_system_by_page_reads_the_same_text(rt, monkeypatch):
    """page in, text out on the route of tests/test_gpu_pred_to_text.py (tests/golden/pred_to_text.npz holds the lines
    of its page, not the page: the page is that test's synthetic one, the paragraph and line masks planted behind the
    untrained nets): 'page' and 'paragraph' cut the same lines and read the same text"""
    from test_gpu_models import set_analytic_weights
    from test_gpu_pred_to_text import PREDICT_NAMES, planted_lines, planted_paragraphs
    from univer_ocr_amd.my_model.model import make_divisible_by, make_predict_system
    from univer_ocr_amd.my_model.predict import predict_text
    from univer_ocr_amd.my_model.synthetic import make_page_batch
    from univer_ocr_amd.nn.model_system import RawFunctionComponent
    CP, runtime = rt
    page = make_page_batch(1, 64, 96, seed=7)['image']
    framed = make_divisible_by(page, 16, 16).shape
    results = {}
    for labelling in ('paragraph', 'page'):
        system, models, names = make_predict_system(framed, line_labelling=labelling)
        assert names == PREDICT_NAMES and system.components[names.index('LineCrop')].stage.labelling == labelling
        for model in models.values():
            set_analytic_weights(model)

        def plant_paragraphs(context):
            context['paragraph_pred'] = CP.copy(planted_paragraphs(framed))

        def plant_lines(context):
            context['line_pred'] = [CP.copy(planted_lines(crop.shape)) for crop in context['cropped_monochrome']]
        system.components.insert(names.index('ParagraphCrop'), RawFunctionComponent(plant_paragraphs))
        system.components.insert(names.index('LineCrop') + 1, RawFunctionComponent(plant_lines))
        calls = recorded_calls(runtime, monkeypatch)
        context = {}
        text = predict_text(page, system, context=context)
        monkeypatch.undo()
        assert calls.count('uocr_label_batch') == (1 if labelling == 'page' else 0)
        assert calls.count('uocr_label_components') == (1 if labelling == 'page' else 5), 'the page, then two per paragraph'
        results[labelling] = text, [[CP.asnumpy(line) for line in p] for p in context['cropped_2_monochrome']]
    (text_a, crops_a), (text_b, crops_b) = results['paragraph'], results['page']
    assert [len(p) for p in text_a] == [2, 2] and text_a == text_b
    for p, (lines_a, lines_b) in enumerate(zip(crops_a, crops_b)):
        assert len(lines_a) == len(lines_b)
        for l, (a, b) in enumerate(zip(lines_a, lines_b)):
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), f'line [{p}][{l}]'
