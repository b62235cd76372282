"""Char labels on the GPU (csrc/char_label.hip) against the reference's LabelChar._func1 results in
tests/golden/char_label.npz and, at sizes derived from the kernels' own tile, chunk and launch sizes, against the NumPy
restatement of the rules that tests/test_char_label_host.py pins to that fixture.  Labels and ids are exact in every
dtype (`array_equal`, no tolerance): every input is a multiple of 1/64 -- the same number in binary16, float32 and float64
-- and keeps more than 1e-3 away from its line's threshold.  The [CharLabel, Char] model system runs against the
reference's Char net with the tolerances of tests/test_gpu_label.py."""
import contextlib
import ctypes as C

import numpy as np
import pytest

from conftest import load_golden, rel_linf
from test_char_label_host import BITS, N_CHARS, char_label_rules
from test_gpu_bounds import GUARD, SENTINEL
from test_gpu_label import SYSTEM_TOL

pytestmark = pytest.mark.gpu

DTYPES = ('float32', 'float64', 'float16')
LINES_OF_THE_PAGE = ((0, 0), (0, 1), (1, 0))


@pytest.fixture(scope='module')
def g():
    return load_golden('char_label')


@pytest.fixture
def rt():
    from univer_ocr_amd.nn import CP
    CP.use_gpu(0)
    CP.set_dtype('float32')
    return CP, CP.runtime()


def raw_call(runtime, dtype, x, h, w, c, bits, n_chars, labels, ids, n_lines=None):
    """uocr_char_label on lists of device addresses (None = a null entry; x / h / w / labels / ids = None: a null array)"""
    from univer_ocr_amd.hip import lib as hiplib
    n = len(h) if n_lines is None else n_lines
    pointers = lambda values: None if values is None else (C.c_void_p * len(values))(*values)
    ints = lambda values: None if values is None else (C.c_int * len(values))(*values)
    runtime.call('uocr_char_label', hiplib.dtype_code(dtype), n, pointers(x), ints(h), ints(w), c, bits, n_chars,
                 pointers(labels), pointers(ids))


def label_lines(rt, lines, bits=BITS, n_chars=N_CHARS, dtype='float32'):
    """ONE uocr_char_label call on host arrays (1, H, W, C); the outputs start as NaN / -7 -> (labels, ids) on the host"""
    CP, runtime = rt
    dev = [CP.copy(x, dtype) for x in lines]
    labels = [CP.copy(np.full((x.shape[2], n_chars), np.nan), dtype) for x in lines]
    ids = [CP.full((x.shape[2],), -7, np.int32) for x in lines]
    raw_call(runtime, dtype, [a.ptr for a in dev], [x.shape[1] for x in lines], [x.shape[2] for x in lines],
             lines[0].shape[3], bits, n_chars, [a.ptr for a in labels], [a.ptr for a in ids])
    return [CP.asnumpy(a) for a in labels], [CP.asnumpy(a) for a in ids]


def check_lines(rt, lines, bits=BITS, n_chars=N_CHARS, dtype='float32', expected=None, what=''):
    labels, ids = label_lines(rt, lines, bits, n_chars, dtype)
    expected = expected or [char_label_rules(x, bits, n_chars) for x in lines]
    for i, (x, (exp_labels, exp_ids)) in enumerate(zip(lines, expected)):
        where = f'{what} line {i} {x.shape} {dtype}'
        assert labels[i].dtype == np.dtype(dtype) and not np.isnan(labels[i]).any(), f'{where}: labels not fully written'
        assert np.array_equal(ids[i], exp_ids), f'{where}: ids differ in columns {np.flatnonzero(ids[i] != exp_ids)[:8]}'
        assert np.array_equal(labels[i], exp_labels.astype(dtype)), f'{where}: labels differ'
    return labels, ids


def random_line(rng, h, w, c=BITS + 1, bits=BITS, n_chars=N_CHARS, replaced=0.35):
    """(1, H, W, C) of multiples of 1/64: a class per column, `replaced` of the pixels another code (classes and codes
    that are no class alike), so the votes are contested and, for small H, often tied; set bits lie in [56, 64] / 64,
    clear ones in [0, 8] / 64, the channels past the bits hold either; every element keeps 1e-3 clear of the threshold"""
    codes = np.repeat(rng.integers(0, n_chars, (1, w)), h, axis=0)
    codes = np.where(rng.random((h, w)) < replaced, rng.integers(0, 1 << bits, (h, w)), codes)
    set_bits = (codes[:, :, None] >> np.arange(c)) & 1
    set_bits[:, :, bits:] = rng.integers(0, 2, (h, w, c - bits))
    x = np.where(set_bits == 1, rng.integers(56, 65, set_bits.shape), rng.integers(0, 9, set_bits.shape))[None] / 64.0
    assert np.min(np.abs(x - 0.5 * (x.mean() + x.max()))) > 1e-3
    return x


def threshold_of(x):
    return 0.5 * (x.mean() + x.max())


def sensitive_line(rng, h, w, top=1.0, top_at=None, ramp=False):
    """(1, H, W, 9) of multiples of 1/64 whose labels depend on the line's exact statistics.  Every pixel is WEAK (its set
    bits hold a, the largest multiple of 1/64 at least 2e-3 below the threshold t) or STRONG (b, the smallest one at least
    2e-3 above t).  In about half of the columns 65 % of the rows are weak pixels of the column's class k and the others
    strong pixels of another class j, in the other columns 35 %.  A weak pixel reads as k below a and as class 0 above; a
    strong one as j below b and as class 0 above.  So the first kind of column elects k when t comes out below a, and 0
    otherwise; the second kind j when t comes out below b, and 0 otherwise: an error of about 1/64 in t, either way,
    changes the labels (downwards only in a line of one column, which has columns of the first kind only).  t itself hangs on ONE element, `top` (> b) at flat index `top_at` (default: the last
    letter_spacing element), the line's only maximum: without it t falls by (top - b) / 2.  ramp: the clear elements
    grow from [0, 4] / 64 in the first row to [16, 20] / 64 in the last, so the statistics chunks of a long line have
    very different sums.  Returned with t; every element keeps more than 1e-3 clear of t."""
    c = BITS + 1
    k, other = rng.integers(1, N_CHARS, (2, 1, w))
    mostly_weak = rng.random(w) < 0.5
    mostly_weak[:2] = [True, False][:w]                            # both kinds of column wherever there are two columns
    weak = np.argsort(rng.random((h, w)), axis=0) < np.where(mostly_weak, -(-13 * h // 20), 7 * h // 20)
    codes = np.where(weak, k, np.where(other == k, other % (N_CHARS - 1) + 1, other))
    set_bits = ((codes[:, :, None] >> np.arange(c)) & 1).astype(bool)
    clear = rng.integers(0, 5, (h, w, c)) + (np.round(16 * np.arange(h) / max(1, h - 1)).astype(int)[:, None, None] if ramp else 0)
    top_at = h * w * c - 1 if top_at is None else top_at
    a, b = 30, 34
    for _ in range(100):
        x = np.where(set_bits, np.where(weak[:, :, None], a, b), clear).reshape(-1) / 64.0
        x[top_at] = top
        t = threshold_of(x)
        fit = int(np.floor((t - 2e-3) * 64)), int(np.ceil((t + 2e-3) * 64))
        if fit == (a, b):
            break
        a, b = fit
    else:
        raise AssertionError('no fixed point for the two levels')
    assert clear.max() < a and b / 64 < top and x.max() == top and np.sum(x == top) == 1
    assert np.min(np.abs(x - t)) > 1e-3
    return x.reshape(1, h, w, c), t


def assert_depends_on_statistics(x, t, what=''):
    """the expected ids change when the one maximum goes, and when t is off by 0.02 either way (a line of one column:
    when it is 0.02 too low)"""
    ids = char_label_rules(x)[1]
    without = x.copy()
    without.reshape(-1)[np.argmax(x)] = 0.0
    assert not np.array_equal(char_label_rules(without)[1], ids), f'{what}: the maximum decides nothing'
    for wrong in (t - 0.02, t + 0.02)[:1 if x.shape[2] == 1 else 2]:
        assert not np.array_equal(char_label_rules(x, threshold=wrong)[1], ids), f'{what}: t = {wrong:.3f} gives the same labels'
    return ids


@pytest.fixture
def sizes(rt):
    """(columns per vote block, elements per statistics chunk, lines per launch) of the library"""
    label_lines(rt, [np.zeros((1, 2, 2, BITS + 1))])
    cols, chunk, per_launch, launches = rt[1].last_char_label()
    assert cols > 1 and chunk > 0 and per_launch > 0 and launches == 2
    return cols, chunk, per_launch


# ---- fixture (a): the reference's labels -------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_labels_and_ids_equal_the_reference(dtype, g, rt):
    names = [str(s) for s in g['line_names']]
    lines = [g[f'{name}/x'] for name in names]
    check_lines(rt, lines, dtype=dtype, expected=[(g[f'{name}/labels'], g[f'{name}/ids']) for name in names], what='golden')
    assert rt[1].last_char_label()[3] == 2, 'all lines of the fixture fit one launch pair'


def test_python_wrapper_allocates_and_returns_device_arrays(g, rt):
    from univer_ocr_amd.my_model.crop import LabelChars
    from univer_ocr_amd.nn import ops
    CP, _ = rt
    names = [str(s) for s in g['line_names']]
    for dtype in DTYPES:
        dev = [CP.copy(g[f'{name}/x'], dtype) for name in names]
        labels, ids = ops.char_label(dev, BITS, N_CHARS, want_ids=True)
        for name, lab, idv in zip(names, labels, ids):
            assert lab.dtype == np.dtype(dtype) and idv.dtype == np.int32
            assert np.array_equal(CP.asnumpy(lab), g[f'{name}/labels'].astype(dtype)), name
            assert np.array_equal(CP.asnumpy(idv), g[f'{name}/ids']), name
        nested = LabelChars()([dev[:2], [], dev[2:5]])
        assert [len(p) for p in nested] == [2, 0, 3]
        for name, lab in zip(names, nested[0] + nested[2]):
            assert np.array_equal(CP.asnumpy(lab), g[f'{name}/labels'].astype(dtype)), name


# ---- sizes derived from the library's own ----------------------------------------------------------------------------------
_EXPECTED = {}


def grid_of_sizes(cols):
    """every W in {1, cols - 1, cols, cols + 1, 2 cols + 3} at every H in {1, 2, 31, 32, 33, 256}, each line with labels
    that hang on its own statistics and a threshold unlike its neighbours'; expected values once"""
    if cols not in _EXPECTED:
        rng = np.random.default_rng(20)
        shapes = [(h, w) for h in (1, 2, 31, 32, 33, 256) for w in (1, cols - 1, cols, cols + 1, 2 * cols + 3)]
        made = [sensitive_line(rng, h, w, top=(1.0, 0.9, 0.8, 0.7, 0.6)[(i + i // 5) % 5], ramp=h > 8) for i, (h, w) in enumerate(shapes)]
        for i, (x, t) in enumerate(made):
            assert_depends_on_statistics(x, t, f'grid line {i}')
            assert i == 0 or abs(t - made[i - 1][1]) > 0.02, 'neighbouring lines share a threshold'
        lines = [x for x, _ in made]
        _EXPECTED[cols] = lines, [char_label_rules(x) for x in lines]
    return _EXPECTED[cols]


@pytest.mark.parametrize('dtype', DTYPES)
def test_widths_and_heights_around_the_tile(dtype, sizes, rt):
    """30 lines of different H and W mixed in ONE call: ragged last tiles, one-column lines, the tallest line allowed"""
    lines, expected = grid_of_sizes(sizes[0])
    check_lines(rt, lines, dtype=dtype, expected=expected, what='grid')
    assert rt[1].last_char_label()[3] == 2 * -(-len(lines) // sizes[2])


@pytest.mark.parametrize('c,bits,n_chars', [(8, 8, 162), (9, 8, 162), (12, 8, 162), (4, 3, 5), (9, 8, 256), (16, 1, 2),
                                            (5, 5, 1)])
def test_channel_bit_and_class_counts(c, bits, n_chars, sizes, rt):
    """channels past the bits count in the threshold only; n_chars = 2^bits leaves no code unknown; one class: every
    other code is unknown"""
    rng = np.random.default_rng(21 + c)
    lines = [random_line(rng, h, w, c, bits, n_chars) for h, w in ((32, sizes[0] + 5), (3, 7), (32, 1))]
    for dtype in DTYPES:
        _, ids = check_lines(rt, lines, bits, n_chars, dtype, what=f'c={c} bits={bits} n_chars={n_chars}')
        if n_chars == 1 << bits:
            assert all((v >= 0).all() for v in ids)


def labels_need_every_chunk(x, chunk):
    """no single chunk's statistics, nor those of the whole chunks without the partial last one, give x's labels"""
    ids, flat = char_label_rules(x)[1], x.reshape(-1)
    parts = [flat[k:k + chunk] for k in range(0, flat.size, chunk)] + [flat[:flat.size // chunk * chunk]]
    return all(not np.array_equal(char_label_rules(x, threshold=threshold_of(part))[1], ids) for part in parts)


def test_a_line_longer_than_two_statistics_chunks(sizes, rt):
    """three partials per line with very different sums, the line's one maximum in the last, partial chunk -- or in the
    first, with a fifth of the sum in the last: the labels follow only if the vote blocks add up ALL partials of THEIR line"""
    cols, chunk, _ = sizes
    c = BITS + 1
    w, wide = 2 * chunk // (32 * c) + 3, 45 * chunk // (512 * c)
    assert 2 * chunk < 32 * w * c < 32 * wide * c < 3 * chunk
    rng = np.random.default_rng(22)
    last, t_last = sensitive_line(rng, 32, w, ramp=True)
    for _ in range(50):                                           # (t has to sit close enough above its lower level)
        first, t_first = sensitive_line(rng, 32, wide, 0.8, top_at=c - 1, ramp=True)
        if labels_need_every_chunk(first, chunk):
            break
    small, t_small = sensitive_line(rng, 5, 3, top=0.6)
    for x, t in ((last, t_last), (first, t_first), (small, t_small)):
        assert_depends_on_statistics(x, t, 'long')
    assert labels_need_every_chunk(last, chunk) and labels_need_every_chunk(first, chunk)
    assert min(abs(t_last - t_first), abs(t_first - t_small), abs(t_last - t_small)) > 0.03
    for dtype in DTYPES:
        check_lines(rt, [last, small, first], dtype=dtype, what='long')


def many_small_lines(count, per_launch, seed):
    """4 x 3 lines, each drawn until neither it nor the line before it, nor the line per_launch places before it (same
    place in the previous launch pair), keeps its labels under the other's threshold"""
    rng = np.random.default_rng(seed)
    lines, ts, ids = [], [], []

    def confusable(x, t, mine, j):
        return (np.array_equal(char_label_rules(x, threshold=ts[j])[1], mine) or
                np.array_equal(char_label_rules(lines[j], threshold=t)[1], ids[j]))
    while len(lines) < count:
        i = len(lines)
        x, t = sensitive_line(rng, 4, 3, top=(1.0, 0.9, 0.8, 0.7, 0.6)[i % 5])
        mine = assert_depends_on_statistics(x, t, f'line {i}')
        if not any(confusable(x, t, mine, j) for j in (i - 1, i - per_launch) if j >= 0):
            lines.append(x), ts.append(t), ids.append(mine)
    return lines, ts


def test_more_lines_than_one_launch_takes(sizes, rt):
    """the second launch pair starts its partials and its tiles over: every line must come out by ITS statistics"""
    _, _, per_launch = sizes
    lines, _ = many_small_lines(per_launch + 1, per_launch, 23)
    expected = [char_label_rules(x) for x in lines]
    check_lines(rt, lines, expected=expected, what='many')
    assert rt[1].last_char_label()[3] == 4, 'two launch pairs'
    check_lines(rt, lines[:per_launch], expected=expected[:per_launch], what='exactly one chunk')
    assert rt[1].last_char_label()[3] == 2


def test_second_call_after_a_larger_one_and_repeatability(sizes, rt):
    """stale partials of a larger call must not leak into a smaller one (under any of the larger call's thresholds the
    small line would get other labels); the same call twice gives the same bytes"""
    cols, chunk, _ = sizes
    rng = np.random.default_rng(24)
    (big_a, t_a), (big_b, t_b) = sensitive_line(rng, 32, 3 * chunk // (32 * 9) + 1, ramp=True), sensitive_line(rng, 32, 2 * cols + 1, 0.9)
    small, t_small = sensitive_line(rng, 7, cols - 3, top=0.65)
    small_ids = assert_depends_on_statistics(small, t_small, 'small')
    for t in (t_a, t_b):
        assert not np.array_equal(char_label_rules(small, threshold=t)[1], small_ids)
    assert_depends_on_statistics(big_a, t_a, 'big'), assert_depends_on_statistics(big_b, t_b, 'big')
    first = check_lines(rt, [big_a, big_b], what='big')
    check_lines(rt, [small], what='small after big')
    again = label_lines(rt, [big_a, big_b])
    for a, b in zip(first[0] + first[1], again[0] + again[1]):
        assert a.tobytes() == b.tobytes()


def test_capture_and_replay(sizes, rt):
    """the call is asynchronous and capturable: a replayed graph labels what the input buffers hold then"""
    import torch
    CP, runtime = rt
    cols = sizes[0]
    rng = np.random.default_rng(25)
    shapes = [(32, 2 * cols + 3), (5, cols - 1)]
    versions = [[sensitive_line(rng, h, w, top)[0] for h, w in shapes] for top in (1.0, 0.7)]   # (thresholds 0.1 apart)
    dev = [CP.copy(x, np.float32) for x in versions[0]]
    labels = [CP.zeros((w, N_CHARS), np.float32) for _, w in shapes]
    ids = [CP.zeros((w,), np.int32) for _, w in shapes]
    with runtime.capture(torch.cuda.MemPool()) as graph:
        raw_call(runtime, 'float32', [a.ptr for a in dev], [h for h, _ in shapes], [w for _, w in shapes], BITS + 1, BITS,
                 N_CHARS, [a.ptr for a in labels], [a.ptr for a in ids])
    for lines in versions[::-1] + versions:
        for a, x in zip(dev, lines):
            a.set(x)
        graph.replay()
        for i, x in enumerate(lines):
            exp_labels, exp_ids = char_label_rules(x)
            assert np.array_equal(CP.asnumpy(ids[i]), exp_ids) and np.array_equal(CP.asnumpy(labels[i]), exp_labels)


# ---- bounds --------------------------------------------------------------------------------------------------------------------
class Packed:
    """float32-sized slots laid out one after the other in ONE sentinel-filled device buffer, `gap` elements (odd: the
    slots lose their 16-byte alignment) between them and GUARD elements at both ends"""

    def __init__(self, CP, counts, gap=3):
        self.CP, self.offsets, at = CP, [], GUARD
        for count in counts:
            self.offsets.append((at, int(count)))
            at += int(count) + gap
        self.host = np.full(at - gap + GUARD, SENTINEL, np.float32)
        self.buf = None

    def upload(self, payloads=()):
        for (at, count), payload in zip(self.offsets, payloads):
            self.host[at:at + count] = np.asarray(payload, np.float32).reshape(-1)
        self.buf = self.CP.copy(self.host, np.float32)
        return [self.buf.ptr + 4 * at for at, _ in self.offsets]

    def check(self, what, expect_written=True):
        """the slots' contents; everything between and around them must still hold the sentinel"""
        got = self.CP.asnumpy(self.buf)
        outside = np.ones(got.size, bool)
        for at, count in self.offsets:
            outside[at:at + count] = False
        assert np.all(got[outside] == SENTINEL), f'{what}: wrote outside its buffers at {np.flatnonzero(outside & (got != SENTINEL))[:8]}'
        slots = [got[at:at + count] for at, count in self.offsets]
        if expect_written:
            assert not any(np.any(s == SENTINEL) for s in slots), f'{what}: elements not written'
        return slots


def test_everything_stays_inside_its_buffers(sizes, rt):
    """inputs, labels and ids of every line sit between sentinel borders, off 16-byte alignment (the scalar heads and
    tails of the 16-byte loads and stores), at ragged sizes.  The one maximum of every line, on which its labels hang,
    is its FIRST or its LAST element: inside a scalar head or tail of the statistics kernel wherever the line has one"""
    CP, runtime = rt
    cols, chunk, _ = sizes
    c = BITS + 1
    rng = np.random.default_rng(26)
    shapes = [(32, 2 * cols + 3), (1, 1), (33, cols - 1), (32, chunk // (32 * c) + 2), (2, cols + 1), (5, 3), (31, cols)]
    made = [sensitive_line(rng, h, w, top=(1.0, 0.85, 0.7)[i % 3], top_at=0 if i % 2 else None, ramp=h > 8)
            for i, (h, w) in enumerate(shapes)]
    lines = [x for x, _ in made]
    for i, (line, t) in enumerate(made):
        assert_depends_on_statistics(line, t, f'line {i}')
    x, labels, ids = (Packed(CP, [v.size for v in lines]), Packed(CP, [w * N_CHARS for _, w in shapes]),
                      Packed(CP, [w for _, w in shapes], gap=1))
    # at least one line starts off a 16-byte border with its maximum in front, one ends off a border with it at the end
    starts, ends = [4 * at % 16 for at, _ in x.offsets], [4 * (at + n) % 16 for at, n in x.offsets]
    assert any(starts[i] and i % 2 for i in range(len(lines))) and any(ends[i] and not i % 2 for i in range(len(lines)))
    raw_call(runtime, 'float32', x.upload(lines), [h for h, _ in shapes], [w for _, w in shapes], c, BITS, N_CHARS,
             labels.upload(), ids.upload())
    got_labels, got_ids = labels.check('labels'), ids.check('ids')
    x.check('x', expect_written=False)
    for i, line in enumerate(lines):
        exp_labels, exp_ids = char_label_rules(line)
        assert np.array_equal(got_ids[i].view(np.int32), exp_ids), f'line {i}: ids'
        assert np.array_equal(got_labels[i].reshape(-1, N_CHARS), exp_labels.astype(np.float32)), f'line {i}: labels'


@contextlib.contextmanager
def workspace_of(CP, nbytes):
    """the runtime's calls go to a context of its own whose workspace is exactly `nbytes` long"""
    import torch
    rt = CP.runtime()
    handle = C.c_void_p()
    assert rt.lib.uocr_ctx_create(rt.device_index, nbytes, C.byref(handle)) == 0
    from univer_ocr_amd.nn.gpu import Lane
    try:
        with rt.on(Lane(torch.cuda.current_stream(), handle)):
            rt.call('uocr_ctx_set_stream', C.c_void_p(torch.cuda.current_stream().cuda_stream))
            yield
            rt.call('uocr_stream_sync')
    finally:
        rt.lib.uocr_ctx_destroy(handle)


def test_workspace_is_sized_by_the_statistics_chunks(sizes, rt):
    """16 bytes per statistics chunk of the largest launch pair: a workspace of exactly that size does, 16 bytes less
    are refused with UOCR_ERR_WORKSPACE and nothing is written.  This pins the size computation and that a refused call
    writes nothing.  It does NOT detect a write past the workspace: the ABI hands out no pointer to it, so what lies behind
    it cannot be filled with a sentinel as the callers' buffers are, and a write past an exactly sized device allocation
    goes unobserved."""
    from univer_ocr_amd.hip import HipError
    CP, runtime = rt
    _, chunk, _ = sizes
    rng = np.random.default_rng(27)
    lines = [random_line(rng, 32, 2 * chunk // (32 * 9) + 2), random_line(rng, 3, 5), random_line(rng, 32, chunk // (32 * 9) + 1)]
    need = 16 * sum(-(-x.size // chunk) for x in lines)
    assert need == 16 * 6
    with workspace_of(CP, need):
        check_lines(rt, lines, what='exact workspace')
    with workspace_of(CP, need - 16):
        dev = [CP.copy(x, np.float32) for x in lines]
        labels = [CP.copy(np.full((x.shape[2], N_CHARS), np.nan), np.float32) for x in lines]
        with pytest.raises(HipError, match=r'\(-4\)'):
            raw_call(runtime, 'float32', [a.ptr for a in dev], [x.shape[1] for x in lines], [x.shape[2] for x in lines], 9,
                     BITS, N_CHARS, [a.ptr for a in labels], None)
        assert all(np.isnan(CP.asnumpy(a)).all() for a in labels), 'a refused call wrote labels'
        check_lines(rt, lines[1:], what='a smaller call fits')


# ---- arguments -----------------------------------------------------------------------------------------------------------------
def test_argument_errors_write_nothing(rt):
    from univer_ocr_amd.hip import HipError
    CP, runtime = rt
    h, w, c = 4, 6, 9
    x = [CP.zeros((1, h, w, c), np.float32) for _ in range(2)]
    tall = CP.zeros((1, 257, w, c), np.float32)
    labels = [CP.copy(np.full((w, 256), np.nan), np.float32) for _ in range(2)]
    ids = [CP.full((w,), -7, np.int32) for _ in range(2)]
    good = dict(dtype='float32', x=[a.ptr for a in x], h=[h, h], w=[w, w], c=c, bits=BITS, n_chars=N_CHARS,
                labels=[a.ptr for a in labels], ids=[a.ptr for a in ids], n_lines=2)
    bad = [(dict(x=None), -1), (dict(h=None), -1), (dict(w=None), -1), (dict(labels=None), -1), (dict(n_lines=-1), -1),
           (dict(x=[x[0].ptr, None]), -1), (dict(labels=[None, labels[1].ptr]), -1), (dict(ids=[ids[0].ptr, None]), -1),
           (dict(h=[h, 0]), -1), (dict(w=[w, -2]), -1), (dict(bits=9), -1), (dict(bits=0), -1), (dict(c=7), -1),
           (dict(c=17, bits=8), -1), (dict(n_chars=257), -1), (dict(n_chars=0), -1), (dict(bits=3, n_chars=9), -1),
           (dict(x=[x[0].ptr, tall.ptr], h=[h, 257]), -5), (dict(x=[x[0].ptr, x[1].ptr + 2]), -1),
           (dict(labels=[labels[0].ptr + 2, labels[1].ptr]), -1), (dict(ids=[ids[0].ptr, ids[1].ptr + 2]), -1)]
    for change, code in bad:
        with pytest.raises(HipError, match=rf'\({code}\)'):
            raw_call(runtime, **dict(good, **change))
        for a in labels:
            assert np.isnan(CP.asnumpy(a)).all(), f'{change}: labels were touched'
        for a in ids:
            assert (CP.asnumpy(a) == -7).all(), f'{change}: ids were touched'
    with pytest.raises(HipError, match=r'\(-2\)'):
        runtime.call('uocr_char_label', 7, 2, (C.c_void_p * 2)(*good['x']), (C.c_int * 2)(h, h), (C.c_int * 2)(w, w), c, BITS,
                     N_CHARS, (C.c_void_p * 2)(*good['labels']), None)
    before = runtime.last_char_label()
    raw_call(runtime, **dict(good, n_lines=0))                   # nothing to do: OK, no launch
    assert np.isnan(CP.asnumpy(labels[0])).all() and runtime.last_char_label() == before
    raw_call(runtime, 'float32', None, None, None, c, BITS, N_CHARS, None, None, n_lines=0)   # ... whatever else is passed
    assert runtime.last_char_label() == before
    raw_call(runtime, **dict(good, ids=None))                    # ids are optional; an all-zero line is class 0 everywhere
    for a in labels:
        flat = CP.asnumpy(a).reshape(-1)
        assert np.array_equal(flat[:w * N_CHARS].reshape(w, N_CHARS), np.eye(N_CHARS, dtype=np.float32)[[0] * w])
        assert np.isnan(flat[w * N_CHARS:]).all()
    assert (CP.asnumpy(ids[0]) == -7).all()


# ---- the [CharLabel, Char] model system ---------------------------------------------------------------------------------
def page_of(g, CP, what):
    return [[CP.copy(g[f'{what}0_0']), CP.copy(g[f'{what}0_1'])], [CP.copy(g[f'{what}1_0'])]]


@pytest.mark.parametrize('opt_tag,dtype', [('sgd', 'float32'), ('sgd', 'float64'), ('adam', 'float64')])
def test_char_label_system_equals_the_reference(opt_tag, dtype, g, rt):
    """[CharLabel, Char] on the page of fixture (b): char_labels equal the reference's exactly; losses, char_pred[p][l] and
    the weights after the three steps (one per line) equal the reference Char net's to the tolerances of DESIGN 3.
    (Adam in float64 only: float32 Adam weights cannot be held to a normalised bound after more than one step.)"""
    from test_gpu_models import check_sampled, set_analytic_weights
    from univer_ocr_amd.my_model.model import CharSelector, make_char, make_char_label_component
    from univer_ocr_amd.nn.model_system import ModelComponent, ModelSystem
    from univer_ocr_amd.nn.optimizers import Adam, Momentum
    CP, _ = rt
    CP.set_dtype(dtype)
    try:
        opt = Momentum(lr=0.01, momentum=0) if opt_tag == 'sgd' else Adam(lr=0.0015)
        char = make_char(g['mono0_0'].shape, opt)
        set_analytic_weights(char)
        system = ModelSystem([make_char_label_component(), ModelComponent(
            'Char', char, CharSelector('cropped_2_monochrome', 'char_labels', 'char_pred'), delist_result=True)])
        context = {'cropped_2_char': page_of(g, CP, 'char'), 'cropped_2_monochrome': page_of(g, CP, 'mono')}
        system.train(context)
        assert [len(p) for p in context['char_labels']] == [2, 1]
        for p, l in LINES_OF_THE_PAGE:
            got = CP.asnumpy(context['char_labels'][p][l])
            assert got.dtype == np.dtype(dtype) and np.array_equal(got, g[f'labels{p}_{l}']), f'char_labels[{p}][{l}]'
        tol, weight_tol = SYSTEM_TOL[dtype]
        entry = context['losses']['Char']
        assert len(entry['output_losses']) == 3 and [len(p) for p in context['char_pred']] == [2, 1]
        errs = {'losses': rel_linf(np.array([float(v) for v in entry['output_losses']]), g[f'{opt_tag}/train/Char/output_losses']),
                'reg': rel_linf(np.array(float(entry['regularization_loss'])), g[f'{opt_tag}/train/Char/regularization_loss'])}
        for p, l in LINES_OF_THE_PAGE:
            pred, key = CP.asnumpy(context['char_pred'][p][l]), f'{opt_tag}/train/char_pred{p}_{l}'
            errs[f'pred{p}_{l}'] = (rel_linf(pred, g[key]) if key in g.files
                                    else rel_linf(pred.reshape(-1)[::5], g[key + '@stride5']))
        print(f'{opt_tag}/{dtype}: ' + ', '.join(f'{k} {v:.2e}' for k, v in errs.items()))
        for what, err in errs.items():
            assert err <= tol, f'{what}: rel_linf={err:.3e} > {tol:.1e}'
        werrs = {pn: check_sampled(pn, p.value, g, f'{opt_tag}/final', weight_tol) for pn, p in char.params().items()}
        print(f'{opt_tag}/{dtype}: weights {max(werrs.values()):.2e} ({max(werrs, key=werrs.get)})')
    finally:
        CP.set_dtype('float32')
