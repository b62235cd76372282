"""The label overlap on the GPU (csrc/label_overlap.hip) against the rules of tests/mask_score_rules.py, which
tests/test_mask_score_host.py pins.  The table, its rows and columns and the summary EQUAL the rules (`==`: the kernels
count).  All sizes come from uocr_label_overlap_limits.  Then ops.label_overlap and ops.mask_score on generated pages, the
mask evaluate system, evaluate_masks and the command line."""
import ctypes as C
import json

import numpy as np
import pytest

import mask_score_rules as M

pytestmark = pytest.mark.gpu

UNSET = -7                                                         # what every output holds before a call
SLACK = 6                                                          # elements of every output past what the call owns
TOP = 2 ** 31 - 1


@pytest.fixture
def rt():
    from univer_ocr_amd.nn import CP
    CP.use_gpu(0)
    CP.set_dtype('float32')
    return CP, CP.runtime()


@pytest.fixture(scope='module')
def limits():
    """(pixels per block, cells of the largest table counted in LDS, entries per launch, largest cap) of the library"""
    from univer_ocr_amd.hip import lib as hiplib
    outs = [C.c_int(0) for _ in range(4)]
    assert hiplib.get_lib().uocr_label_overlap_limits(*[C.byref(out) for out in outs]) == 0
    pixels, lds_cells, per_launch, max_cap = [out.value for out in outs]
    assert pixels % 4 == 0 and pixels >= 512 and lds_cells >= 16 and per_launch > 0 and max_cap > 0
    return pixels, lds_cells, per_launch, max_cap


# ---- planes --------------------------------------------------------------------------------------------------------------------
def runs(rng, n, labels, longest):
    """n labels in runs of 1 .. longest pixels (short ones as likely as long ones), drawn from `labels`"""
    out = np.empty(n, np.int32)
    at = 0
    while at < n:
        length = int(rng.integers(1, int(rng.choice([2, 6, 40, longest])) + 1))
        out[at:at + length] = rng.choice(labels)
        at += length
    return out


def pair_of(rng, h, w, cap_a, cap_b, longest=700):
    """a pair of (h, w) planes in runs: labels 0 .. cap + 1 (the background three times as likely) and now and then the
    largest int and a negative one"""
    pool = lambda cap: [0, 0] + list(range(cap + 2)) + [TOP, -1, -TOP - 1, cap + 1000]
    return (runs(rng, h * w, pool(cap_a), longest).reshape(h, w), runs(rng, h * w, pool(cap_b), longest).reshape(h, w))


def raw_call(runtime, a, b, h, w, cap_a, cap_b, overlap, rows, cols, summary, n_entries=None):
    """uocr_label_overlap on lists of device addresses (None = a null entry; a list that is None: a null array)"""
    n = len(h) if n_entries is None else n_entries
    pointers = lambda values: None if values is None else (C.c_void_p * len(values))(*values)
    ints = lambda values: None if values is None else (C.c_int * len(values))(*[int(v) for v in values])
    void = lambda address: None if address is None else C.c_void_p(address)
    runtime.call('uocr_label_overlap', n, pointers(a), pointers(b), ints(h), ints(w), cap_a, cap_b, void(overlap), void(rows),
                 void(cols), void(summary))


class Outputs:
    """the four outputs for n entries, each with SLACK elements behind it, everything UNSET"""

    def __init__(self, CP, n, cap_a, cap_b):
        self.CP, self.n, self.shapes = CP, n, ((n, cap_a + 2, cap_b + 2), (n, cap_a + 2, 4), (n, cap_b + 2, 4), (n, 8))
        self.arrays = [CP.copy(np.full(int(np.prod(shape)) + SLACK, UNSET, dtype), dtype)
                       for shape, dtype in zip(self.shapes, (np.int32, np.int32, np.int32, np.int64))]

    def pointers(self):
        return [a.ptr for a in self.arrays]

    def host(self):
        flat = [self.CP.asnumpy(a) for a in self.arrays]
        assert all((v[-SLACK:] == UNSET).all() for v in flat), 'written behind an output'
        return [v[:-SLACK].reshape(shape) for v, shape in zip(flat, self.shapes)]

    def untouched(self):
        return all((self.CP.asnumpy(a) == UNSET).all() for a in self.arrays)


def upload(CP, plane, offset=0):
    """the plane on the device, `offset` ints behind the start of its buffer, two guard ints behind it: (buffer, address)"""
    buffer = CP.copy(np.concatenate([np.full(offset, 3, np.int32), plane.reshape(-1), np.full(2, 3, np.int32)]), np.int32)
    return buffer, buffer.ptr + 4 * offset


def check(got, pairs, cap_a, cap_b, what=''):
    overlap, rows, cols, summary = got
    for i, (a, b) in enumerate(pairs):
        want = M.everything(a, b, cap_a, cap_b)
        where = f'{what} entry {i} {a.shape} caps {cap_a}, {cap_b}'
        for name, mine, rule in zip(('overlap', 'rows', 'cols', 'summary'), (overlap[i], rows[i], cols[i], summary[i]), want):
            assert np.array_equal(mine, rule), f'{where}: {name} differs\n{mine}\nthe rules say\n{rule}'


def run_pairs(rt, pairs, cap_a, cap_b, offsets=(0, 0), what=''):
    """ONE uocr_label_overlap call on host pairs of planes: all four outputs EQUAL the rules.  Returns them."""
    CP, runtime = rt
    a = [upload(CP, pa, offsets[0]) for pa, _ in pairs]
    b = [upload(CP, pb, offsets[1]) for _, pb in pairs]
    out = Outputs(CP, len(pairs), cap_a, cap_b)
    raw_call(runtime, [p for _, p in a], [p for _, p in b], [pa.shape[0] for pa, _ in pairs], [pa.shape[1] for pa, _ in pairs],
             cap_a, cap_b, *out.pointers())
    got = out.host()
    check(got, pairs, cap_a, cap_b, what)
    return got


# ---- sizes, alignment ------------------------------------------------------------------------------------------------------------
def test_sizes_around_the_blocks(limits, rt):
    pixels = limits[0]
    rng = np.random.default_rng(80)
    shapes = [(1, pixels - 1), (1, pixels), (1, pixels + 1), (1, 3 * pixels + 5), (1, 1), (1, 257), (257, 1), (3, 5), (67, 129)]
    for caps in ((5, 3), (0, 0)):
        run_pairs(rt, [pair_of(rng, h, w, *caps) for h, w in shapes], *caps, what='sizes')


def test_planes_off_the_vector_alignment(limits, rt):
    """both planes 0 .. 3 ints behind a 16-byte border, never the same distance: head and tail of the 16-byte loads, and a
    second plane that is read across the borders the first one is split at"""
    pixels = limits[0]
    rng = np.random.default_rng(81)
    pairs = [pair_of(rng, 1, n, 4, 6, longest=90) for n in (1, 2, 3, 4, 5, 7, 8, 9, 300, pixels // 4 + 3, pixels + 9)]
    for oa in range(4):
        for ob in range(4):
            if oa != ob:
                run_pairs(rt, pairs, 4, 6, offsets=(oa, ob), what=f'offsets {oa}, {ob}')


def test_the_two_ends_of_the_folding(limits, rt):
    """an all-background pair: one carried run per wave, flushed at its end; two checkerboards a pixel apart: no run is
    longer than a pixel; and one pair of another kind held through whole tiles, then changed"""
    pixels = limits[0]
    background = np.zeros((1, 3 * pixels + 5), np.int32)
    y, x = np.mgrid[0:40, 0:65]
    board = (1 + ((x + y) & 1)).astype(np.int32)
    held = np.full((1, 2 * pixels), 2, np.int32)
    held_b = held.copy()
    held_b[0, pixels // 2:] = 1                                         # the carried pair changes at a tile border
    held_b[0, pixels + 1024 + 77:] = 3                                  # and inside a tile
    got = run_pairs(rt, [(background, background), (board, 3 - board), (held, held_b)], 2, 3, what='folding')
    assert got[0][0, 0, 0] == background.size and got[0][1].sum() == board.size and got[0][1, 1, 2] == board.size // 2


def test_run_borders_at_lane_tile_wave_and_block_ends(limits, rt):
    """the label changes exactly at, one before and one behind every kind of border the kernel has: a lane's four pixels,
    a tile of 256, a wave's share and a block's -- in one plane at the borders, in the other one pixel later"""
    pixels = limits[0]
    n = 2 * pixels + 300
    borders = np.array(sorted({k for step in (4, 256, pixels // 4, pixels) for k in range(step, n, step)
                               if step >= 256 or k < 64 or k > n - 64}))
    rng = np.random.default_rng(82)
    # the label of a pixel: how many borders lie at or before it, modulo 5; `shift` moves every change that many pixels on
    planes = [(np.searchsorted(borders, np.arange(n) - shift, side='right') % 5).astype(np.int32).reshape(1, n)
              for shift in (0, 1, -1)]
    assert planes[0][0, 3] != planes[0][0, 4] and planes[0][0, pixels - 1] != planes[0][0, pixels]
    run_pairs(rt, [(planes[0], planes[1]), (planes[2], planes[0]), (planes[1], planes[1]), (planes[0], rng.permuted(planes[0], axis=1))],
              4, 4, what='borders')


# ---- caps ------------------------------------------------------------------------------------------------------------------------
def table_sides(cells, max_cap):
    """(rows, columns) of a table of exactly `cells` cells, the squarest there is, or None"""
    sides = [(r, cells // r) for r in range(2, max_cap + 3) if cells % r == 0 and 2 <= cells // r <= max_cap + 2]
    return min(sides, key=lambda side: abs(side[0] - side[1])) if sides else None


def test_caps_and_both_table_paths(limits, rt):
    """caps 0 and 0; unequal caps; a table of exactly lds_cells cells (counted in LDS) and one of lds_cells + 1 (added to
    directly); the largest caps; labels at cap, cap + 1 and far above in every one (pair_of)"""
    pixels, lds_cells, _, max_cap = limits
    fits, spills = table_sides(lds_cells, max_cap), table_sides(lds_cells + 1, max_cap)
    assert fits and spills, f'no caps give tables of {lds_cells} and {lds_cells + 1} cells'
    rng = np.random.default_rng(83)
    for rows, columns in ((2, 2), (3, 9), (9, 3), (2, max_cap + 2), fits, fits[::-1], spills, (max_cap + 2, max_cap + 2)):
        cap_a, cap_b = rows - 2, columns - 2
        pairs = [pair_of(rng, 1, pixels + 77, cap_a, cap_b, longest=30), pair_of(rng, 9, 31, cap_a, cap_b, longest=3)]
        a = rng.integers(0, cap_a + 2, (50, 70)).astype(np.int32)       # every cell of the table, no run at all
        pairs.append((a, rng.integers(0, cap_b + 2, (50, 70)).astype(np.int32)))
        edge = np.array([[cap_a, cap_a + 1, TOP, -1, 0, cap_a, 1]], np.int32)
        pairs.append((edge, np.array([[cap_b, cap_b, cap_b + 1, cap_b + 2, cap_b, 0, TOP]], np.int32)))
        run_pairs(rt, pairs, cap_a, cap_b, what=f'table {rows} x {columns}')


def test_more_entries_than_one_launch_takes(limits, rt):
    pixels, _, per_launch, _ = limits
    rng = np.random.default_rng(84)
    shapes = [(1 + k % 5, 3 + (7 * k) % 41) for k in range(per_launch - 1)] + [(1, pixels + 3), (1, 1)]
    assert len(shapes) == per_launch + 1
    run_pairs(rt, [pair_of(rng, h, w, 6, 6, longest=20) for h, w in shapes], 6, 6, what='two groups')


# ---- arguments -------------------------------------------------------------------------------------------------------------------
def test_argument_errors_write_nothing(limits, rt):
    from univer_ocr_amd.hip import HipError
    CP, runtime = rt
    max_cap = limits[3]
    rng = np.random.default_rng(85)
    pairs = [pair_of(rng, 5, 9, 3, 2), pair_of(rng, 1, 40, 3, 2)]
    a, b = [CP.copy(pa, np.int32) for pa, _ in pairs], [CP.copy(pb, np.int32) for _, pb in pairs]
    out = Outputs(CP, 2, 3, 2)
    overlap, rows, cols, summary = out.pointers()
    good = dict(a=[x.ptr for x in a], b=[x.ptr for x in b], h=[5, 1], w=[9, 40], cap_a=3, cap_b=2, overlap=overlap, rows=rows,
                cols=cols, summary=summary, n_entries=2)
    bad = [(dict(a=None), -1), (dict(b=None), -1), (dict(h=None), -1), (dict(w=None), -1), (dict(overlap=None), -1),
           (dict(rows=None), -1), (dict(cols=None), -1), (dict(summary=None), -1), (dict(n_entries=-1), -1),
           (dict(a=[a[0].ptr, None]), -1), (dict(b=[None, b[1].ptr]), -1), (dict(a=[a[0].ptr + 2, a[1].ptr]), -1),
           (dict(b=[b[0].ptr, b[1].ptr + 1]), -1), (dict(h=[5, 0]), -1), (dict(h=[-1, 1]), -1), (dict(w=[9, 0]), -1),
           (dict(w=[-9, 40]), -1), (dict(cap_a=-1), -1), (dict(cap_b=-1), -1), (dict(overlap=overlap + 2), -1),
           (dict(rows=rows + 1), -1), (dict(cols=cols + 2), -1), (dict(summary=summary + 4), -1),
           (dict(cap_a=max_cap + 1), -5), (dict(cap_b=max_cap + 1), -5), (dict(h=[5, 2 ** 16], w=[9, 2 ** 15]), -5)]
    for change, code in bad:
        with pytest.raises(HipError, match=rf'\({code}\)'):
            raw_call(runtime, **dict(good, **change))
        assert out.untouched(), f'{change}: the outputs were touched'
    raw_call(runtime, **dict(good, n_entries=0))                   # nothing to do: OK, no launch
    raw_call(runtime, None, None, None, None, -5, -5, None, None, None, None, n_entries=0)   # ... whatever else is passed
    assert out.untouched()
    raw_call(runtime, **good)
    check(out.host(), pairs, 3, 2, 'after the errors')


# ---- repeatability, capture ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('caps', [(5, 4), (70, 70)], ids=['lds', 'global'])
def test_two_calls_into_the_same_buffers_and_a_replayed_graph(caps, limits, rt):
    """the memset is part of the call: a second call counts from zero, and so does every replay of a captured one"""
    import torch
    CP, runtime = rt
    pixels, lds_cells = limits[:2]
    assert ((caps[0] + 2) * (caps[1] + 2) <= lds_cells) == (caps == (5, 4))
    rng = np.random.default_rng(86)
    shapes = [(1, pixels + 11), (20, 33)]
    versions = [[pair_of(rng, h, w, *caps) for h, w in shapes] for _ in range(2)]
    a = [CP.copy(pa, np.int32) for pa, _ in versions[0]]
    b = [CP.copy(pb, np.int32) for _, pb in versions[0]]
    out = Outputs(CP, 2, *caps)
    call = lambda: raw_call(runtime, [x.ptr for x in a], [x.ptr for x in b], [h for h, _ in shapes], [w for _, w in shapes],
                            *caps, *out.pointers())
    call()
    first = [v.copy() for v in out.host()]
    check(first, versions[0], *caps, 'first call')
    call()
    again = out.host()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(first, again)), 'the second call differs from the first'
    with runtime.capture(torch.cuda.MemPool()) as graph:
        call()
    for pairs in versions[::-1] + versions[:1] * 2:
        for x, y, (pa, pb) in zip(a, b, pairs):
            x.set(pa), y.set(pb)
        graph.replay()
        check(out.host(), pairs, *caps, 'replay')


# ---- the wrappers ----------------------------------------------------------------------------------------------------------------
def test_label_overlap_wrapper(limits, rt):
    from univer_ocr_amd.nn import ops
    CP, _ = rt
    rng = np.random.default_rng(87)
    pairs = [pair_of(rng, h, w, 7, 5) for h, w in ((4, 9), (1, 1), (30, 300))]
    device = [(CP.copy(a, np.int32), CP.copy(b, np.int32)) for a, b in pairs]
    summary, rows, cols = ops.label_overlap(device, 7, 5)
    assert (summary.dtype, rows.dtype, cols.dtype) == (np.int64, np.int32, np.int32)
    again = ops.label_overlap(device, 7, 5, want_table=True)
    assert all(np.array_equal(x, y) for x, y in zip((summary, rows, cols), again[:3]))
    check((again[3], rows, cols, summary), pairs, 7, 5, 'ops.label_overlap')
    empty = ops.label_overlap([], 7, 5, want_table=True)
    assert [v.shape for v in empty] == [(0, 8), (0, 9, 4), (0, 7, 4), (0, 9, 7)]
    for wrong in ([(device[0][0], device[1][0])], [(device[0][0], CP.copy(np.zeros((4, 9)), np.float32))], [(pairs[0][0], device[0][1])]):
        with pytest.raises(ValueError, match='label_overlap'):
            ops.label_overlap(wrong, 7, 5)
    with pytest.raises(ValueError, match='label_overlap'):
        ops.label_overlap(device, -1, 5)


@pytest.mark.parametrize('dtype', ['float32', 'float64', 'float16'])
@pytest.mark.parametrize('size', [(64, 128), (256, 512)], ids=['64x128', '256x512'])
def test_mask_score_on_generated_pages(size, dtype, rt):
    """the truth against itself: everything found and nothing else; against itself three columns to the right: what the
    rules say of the planes label_batch returns"""
    from univer_ocr_amd.my_model.pages import GeneratedPages, PagesWithText
    from univer_ocr_amd.nn import ops
    CP, _ = rt
    source = GeneratedPages(1, *size, seed={(64, 128): 12, (256, 512): 31}[size], length=1, dtype=dtype)
    pages = PagesWithText(source, 1)
    layers = pages.get(0, ['monochrome', 'paragraph', 'line'])
    n_paragraphs = int(source.tables(None, first_page=pages.page_of(0), n_pages=1)['counts'].numpy()[0, 0])
    assert n_paragraphs >= 1
    for tag, threshold, cap in (('monochrome', 0.5, 0), ('paragraph', 'mean', 64), ('line', 'mean_max', 64)):
        truth = CP.copy(layers[tag]) if not hasattr(layers[tag], 'ptr') else layers[tag]
        assert str(truth.dtype) == dtype
        channels = range(truth.shape[3])
        same = ops.mask_score([((truth, c), (truth, c)) for c in channels], threshold, cap=cap)
        for score in same:
            assert score.fp == score.fn == 0 and score.tp > 0 and score.tp + score.tn == size[0] * size[1]
            assert score.matched == score.expected == score.predicted and score.overflow == (score.tp if cap == 0 else 0)
            assert (score.precision, score.recall, score.f1, score.iou) == (1.0, 1.0, 1.0, 1.0)
            assert score.mean_matched_iou == (None if cap == 0 else 1.0) and len(score.rows) == score.expected
        if tag == 'paragraph':
            assert same[0].expected == n_paragraphs
        shifted = CP.copy(np.roll(CP.asnumpy(truth), 3, axis=2), dtype)
        moved = ops.mask_score([((shifted, c), (truth, c)) for c in channels], threshold, cap=cap)
        planes = ops.label_batch([(x, c) for x in (truth, shifted) for c in channels], threshold, labels=True)
        for c in channels:
            a, b = CP.asnumpy(planes[c].labels), CP.asnumpy(planes[len(channels) + c].labels)
            _, rows, _, summary = M.everything(a, b, cap, cap)
            assert moved[c] == ops.mask_score_of(summary, rows), f'{tag} channel {c}'
            assert moved[c].fp == moved[c].fn > 0
        # another rule for the truth: two labelling calls
        other = ops.mask_score([((shifted, 0), (truth, 0))], threshold, true_threshold=0.25, cap=cap)[0]
        a = CP.asnumpy(ops.label_batch([(truth, 0)], 0.25, labels=True)[0].labels)
        _, rows, _, summary = M.everything(a, CP.asnumpy(planes[len(channels)].labels), cap, cap)
        assert other == ops.mask_score_of(summary, rows), f'{tag}: the truth at another threshold'


def test_mask_evaluate_system(rt):
    from univer_ocr_amd.my_model.model import make_mask_evaluate_context_maker, make_mask_evaluate_system
    from univer_ocr_amd.my_model.pages import GeneratedPages, PagesWithText
    from univer_ocr_amd.nn import ops
    np.random.seed(0)
    pages = PagesWithText(GeneratedPages(1, 64, 128, seed=12, length=1), 1)
    system, models, names = make_mask_evaluate_system((1, 64, 128, 1))
    assert names == ['Monochrome', 'Paragraph', 'Line', 'MaskScore'] and list(models) == names[:3]
    assert len(system.components) == 4
    context = make_mask_evaluate_context_maker()(pages.get, (0,))
    assert sorted(context) == ['line_X', 'line_y', 'monochrome_X', 'monochrome_y', 'paragraph_X', 'paragraph_y']
    system.predict(context)
    scores = context['mask_scores']
    assert {net: len(channels) for net, channels in scores.items()} == {'monochrome': 1, 'paragraph': 1, 'line': 2}
    for net, threshold, cap in (('monochrome', 0.5, 0), ('paragraph', 'mean', 64), ('line', 'mean_max', 64)):
        pred, truth = context[f'{net}_pred'], context[f'{net}_y']
        assert pred.shape == truth.shape
        by_hand = ops.mask_score([((pred, c), (truth, c)) for c in range(pred.shape[3])], threshold, cap=cap)
        assert scores[net] == by_hand, net
        for score in by_hand:
            assert score.tp + score.fp + score.fn + score.tn == 64 * 128
            assert score.expected >= 1 or cap == 0


def test_evaluate_masks_and_the_command_line(rt, capsys):
    from univer_ocr_amd.my_model import evaluate
    from univer_ocr_amd.my_model.pages import GeneratedPages, PagesWithText
    np.random.seed(0)
    pages = PagesWithText(GeneratedPages(1, 64, 128, seed=1234, length=2), 2)
    contexts = []
    reports = evaluate.evaluate_masks(pages, 2, contexts=contexts)
    assert len(contexts) == 2 and {net: len(channels) for net, channels in reports.items()} == {'monochrome': 1, 'paragraph': 1, 'line': 2}
    for net, channels in reports.items():
        for c, report in enumerate(channels):
            per_page = [context['mask_scores'][net][c] for context in contexts]
            assert list(report[1:9]) == [sum(score[k] for score in per_page) for k in range(8)]
            assert report.tp + report.fp + report.fn + report.tn == 2 * 64 * 128
    capsys.readouterr()
    np.random.seed(0)
    evaluate.main(['--masks', '--pages', '2', '--height', '64', '--width', '128'])
    printed = capsys.readouterr().out.strip().split('\n')
    assert len(printed) == 1, printed
    line = json.loads(printed[0])
    assert sorted(line) == ['line', 'monochrome', 'paragraph'] and [len(line[net]) for net in sorted(line)] == [2, 1, 1]
    for net, channels in line.items():
        for c, report in enumerate(channels):
            assert list(report) == list(evaluate.MaskReport._fields)
            assert report == json.loads(json.dumps(reports[net][c]._asdict())), 'the same weights, the same report'
    evaluate.main(['--pages', '1', '--height', '96', '--width', '384', '--seed', '77'])
    assert list(json.loads(capsys.readouterr().out)) == list(evaluate.TextReport._fields)
