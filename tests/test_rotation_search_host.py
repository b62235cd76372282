"""Host side of the device rotation search: the table of the search tree (nn/ops.py: search_table), the replay of a leaf
(angle_of_leaf), the geometry the device evaluates (search_geometry) against scipy's (rotation_geometry), and
`search_rules`, the NumPy restatement of the whole device search that the GPU tests use as expected value -- trusted
because it reproduces the reference's own 13-round traces and angles of tests/golden/rotation.npz here.  Then the stage's
call pattern with the device operations replaced, the model systems' assembly and the ABI names.  Nothing here needs a
GPU.

Tolerances.  Table rows, angles, heights, leaves and shapes: equality.  Offsets of search_geometry against
rotation_geometry: 1e-12 -- NumPy's matrix product may fuse one multiply-add where the device rounds product and sum
apart; with |c|, |s| <= 1 and half shapes below 600 one such rounding is at most 2^-53 * 600 * 2 = 1.4e-13 per offset."""

import numpy as np
import pytest

from conftest import load_golden
from test_rotation_host import STAGE_PARAGRAPHS, FakeOps, extent_rules, stage_page

NEW_SYMBOLS = ('uocr_rotation_search', 'uocr_rotation_search_workspace', 'uocr_ctx_last_rotation_search')
ROUNDS, NODES = 13, 8191
OFFSET_TOL = 1e-12
SHAPES = [(1, 1), (1, 7), (7, 1), (2, 3), (16, 16), (37, 211), (100, 300), (255, 511)]


@pytest.fixture(scope='module')
def g():
    return load_golden('rotation')


# ---- the restatement of the device search --------------------------------------------------------------------------------
def probe_height_rules(mask, c, s):
    """the height of the order-0 rotation of a boolean (h, w) mask with the geometry of search_geometry: coordinates
    (offset + oy * m0) + ox * m1 in float64, inside means 0 <= c <= n - 1 (inclusive), the pixel read is floor(c + 0.5)"""
    from univer_ocr_amd.nn.ops import search_geometry
    ih, iw = mask.shape
    M, offset, (oh, ow) = search_geometry(ih, iw, c, s)
    oy, ox = np.mgrid[:oh, :ow].astype(np.float64)
    cy = (offset[0] + oy * M[0]) + ox * M[1]
    cx = (offset[1] + oy * M[2]) + ox * M[3]
    inside = (cy >= 0) & (cy <= ih - 1) & (cx >= 0) & (cx <= iw - 1)
    sy, sx = np.floor(cy + 0.5).astype(int).clip(0, ih - 1), np.floor(cx + 0.5).astype(int).clip(0, iw - 1)
    rows = np.nonzero((inside & mask[sy, sx]).any(axis=1))[0]
    return int(rows.max() - rows.min() + 1) if len(rows) else 0


def search_rules(labels, k, box, eps=1.0):
    """the device search for component k of the (H, W) labels, box (y0, x0, h, w): (leaf, heights int (rounds, 2)) --
    the walk through the table from node 0, to child 2j + 1 where height_a < height_b, else to 2j + 2"""
    from univer_ocr_amd.nn.ops import search_table
    rounds, table = search_table(eps)
    y, x, h, w = box
    mask = labels[y:y + h, x:x + w] == k
    node, heights = 0, []
    for _ in range(rounds):
        ca, sa, cb, sb = table[node].tolist()
        heights.append((probe_height_rules(mask, ca, sa), probe_height_rules(mask, cb, sb)))
        node = 2 * node + (1 if heights[-1][0] < heights[-1][1] else 2)
    return node, np.array(heights, np.int64)


def trace_rules(labels, k, box, eps=1.0):
    """(angle, trace (rounds, 4) = a, b, height_a, height_b): what ops.rotation_search returns for one component"""
    from univer_ocr_amd.nn.ops import search_path
    leaf, heights = search_rules(labels, k, box, eps)
    probes, angle = search_path(leaf, eps)
    return angle, np.column_stack([np.array(probes, np.float64), heights.astype(np.float64)])


def tree_angles(eps=1.0):
    """[(a, b)] of every node of the search tree in heap order, by search_steps' own expressions"""
    nodes, level = [], [(0.0, 180.0)]
    while level[0][1] - level[0][0] > eps:
        probes = [(low + (high - low) / 3, high - (high - low) / 3) for low, high in level]
        nodes += probes
        level = [child for (low, high), (a, b) in zip(level, probes) for child in ((low, b), (a, high))]
    return nodes


# ---- search_table and angle_of_leaf --------------------------------------------------------------------------------------
def test_table_has_the_tree_of_search_steps():
    from univer_ocr_amd.my_model.crop import search_steps
    from univer_ocr_amd.nn.ops import angle_of_leaf, rotation_geometry, search_path, search_table
    rounds, table = search_table(1.0)
    assert rounds == ROUNDS and table.shape == (NODES, 4) and table.dtype == np.float64
    assert search_table(1.0)[1] is table, 'built once'
    r = np.random.default_rng(430)
    sequences = [[0] * ROUNDS, [1] * ROUNDS] + r.integers(0, 2, (200, ROUNDS)).tolist()
    ended = set()
    for decisions in sequences:
        steps = search_steps(1.0)
        a, b = next(steps)
        node, met = 0, []
        for i, low_moves in enumerate(decisions):
            met.append((a, b))
            Ma, Mb = rotation_geometry(3, 5, a)[0], rotation_geometry(3, 5, b)[0]
            assert table[node].tolist() == [Ma[0, 0], Ma[0, 1], Mb[0, 0], Mb[0, 1]], f'node {node}'
            node = 2 * node + (2 if low_moves else 1)
            try:
                a, b = steps.send((2, 1) if low_moves else (1, 2))
            except StopIteration as done:
                assert i == ROUNDS - 1
                angle = done.value
        assert NODES <= node <= 2 * NODES
        assert search_path(node, 1.0) == (met, angle) and angle_of_leaf(node, 1.0) == angle
        ended.add(angle)
    assert angle_of_leaf(NODES, 1.0) is None and angle_of_leaf(2 * NODES, 1.0) is None, 'the ends near 0 and near 180'
    assert None in ended and len(ended) > 150
    for leaf in (0, NODES - 1, 2 * NODES + 1, -1):
        with pytest.raises(ValueError, match='search_path'):
            angle_of_leaf(leaf, 1.0)


def test_every_table_row_equals_rotation_geometry():
    from univer_ocr_amd.nn.ops import rotation_geometry, search_table
    _, table = search_table(1.0)
    nodes = tree_angles()
    assert len(nodes) == NODES
    for node, (a, b) in enumerate(nodes):
        Ma, Mb = rotation_geometry(2, 3, a)[0], rotation_geometry(2, 3, b)[0]
        assert table[node].tolist() == [Ma[0, 0], Ma[0, 1], Mb[0, 0], Mb[0, 1]], f'node {node}: {a}, {b}'


def test_table_refuses_trees_the_device_cannot_walk():
    from univer_ocr_amd.nn.ops import search_table
    assert search_table(2.0)[0] == 12 and search_table(2.0)[1].shape == (4095, 4)
    with pytest.raises(ValueError, match='more than 16 rounds'):
        search_table(0.1)                                              # 180 * (2 / 3)^R < 0.1 first at R = 19
    with pytest.raises(ValueError, match='no round'):
        search_table(180.0)


# ---- search_geometry ---------------------------------------------------------------------------------------------------
def test_search_geometry_against_rotation_geometry():
    """every angle of the table on the issue's box shapes and six random ones: equal shapes, offsets within 1e-12.  A
    shape mismatch on another BLAS would be a tie of the documented kind and is to be listed here
    by (shape, angle), not tolerated by a wider rule: none is listed."""
    from univer_ocr_amd.nn.ops import rotation_geometry, search_geometry
    r = np.random.default_rng(431)
    shapes = SHAPES + [tuple(int(v) for v in r.integers(1, 600, 2)) for _ in range(6)]
    angles = sorted({angle for probes in tree_angles() for angle in probes})
    assert len(angles) >= NODES
    worst, mismatches = 0.0, []
    for angle in angles:
        c, s = np.cos(np.deg2rad(angle)), np.sin(np.deg2rad(angle))
        for ih, iw in shapes:
            M, offset, shape = rotation_geometry(ih, iw, angle)
            m, off, out_shape = search_geometry(ih, iw, c, s)
            assert m == tuple(M.reshape(-1).tolist())
            if out_shape != shape:
                mismatches.append(((ih, iw), angle, out_shape, shape))
            else:
                worst = max(worst, abs(off[0] - offset[0]), abs(off[1] - offset[1]))
    print(f'search_geometry against rotation_geometry: {len(angles) * len(shapes)} pairs, {len(mismatches)} shape '
          f'mismatches, offsets differ by at most {worst:.2e}')
    assert not mismatches, mismatches[:5]
    assert worst <= OFFSET_TOL


# ---- the restatement against the fixture -----------------------------------------------------------------------------------
def test_rules_reproduce_the_traces_and_angles_of_the_reference(g):
    _, _, labels, boxes, angles = stage_page(g)
    for p in range(STAGE_PARAGRAPHS):
        angle, trace = trace_rules(labels, p + 1, boxes[p])
        assert trace.shape == (ROUNDS, 4) and np.array_equal(trace, g[f'stage/{p}/trace']), f'paragraph {p}'
        assert angle == angles[p], f'paragraph {p}'
    assert [a is None for a in angles] == [True, False, False, False]


def test_a_probe_without_a_set_pixel_moves_low(g):
    """0 < 0 is false: low = a in every round, the search ends near 180 and the angle is None"""
    labels = np.zeros((9, 12), np.int32)
    labels[2:5, 3:8] = 1
    leaf, heights = search_rules(labels, 2, (2, 3, 3, 5))
    assert leaf == 2 * NODES and not heights.any()


# ---- the stage with the device operations replaced ---------------------------------------------------------------------
class FakeSearchOps(FakeOps):
    """FakeOps with the device search: the rules on the host labels"""

    def search_table(self, eps=1.0):
        from univer_ocr_amd.nn.ops import search_table
        return search_table(eps)

    def rotation_search(self, components, image_index, ks, eps=1.0):
        ks = list(ks)
        self.calls.append(('search', len(ks)))
        found = []
        for k in ks:
            ys, xs = np.nonzero(components.labels == k)
            box = (int(ys.min()), int(xs.min()), int(ys.max() - ys.min() + 1), int(xs.max() - xs.min() + 1))
            found.append(trace_rules(components.labels, k, box, eps))
        return [angle for angle, _ in found], [trace for _, trace in found]


def test_stage_makes_one_search_one_extent_and_one_crop_call(g, monkeypatch):
    from univer_ocr_amd.my_model import crop
    paragraph, arrays, labels, boxes, angles = stage_page(g)
    fake = FakeSearchOps()
    monkeypatch.setattr(crop, 'ops', fake)
    stage = crop.CropAndRotateParagraphs(search='device')
    assert stage.search == 'device'
    result = stage(paragraph, arrays, divisible_by=(16, 16))
    rotated = sum(a is not None for a in angles)
    assert fake.calls == [('label', 'mean'), ('search', STAGE_PARAGRAPHS), ('extent', rotated), ('crop', 2 * rotated),
                          ('masked', 1), ('masked', 1)]
    assert stage.angles == angles
    for a, per_array in zip(arrays, result):
        for p, item in enumerate(per_array):
            if angles[p] is None:
                assert item == ('upright', id(a), p + 1, (16, 16))
            else:
                y, x, h, w = boxes[p]
                assert item == ('turned', id(a), p + 1, angles[p], extent_rules(labels[y:y + h, x:x + w] == p + 1, angles[p]), (16, 16))
    # the same page through the host search: the same result, 14 extent calls
    fake.calls.clear()
    host = crop.CropAndRotateParagraphs()
    assert host.search == 'host' and host(paragraph, arrays, divisible_by=(16, 16)) == result and host.angles == angles
    assert [kind for kind, _ in fake.calls].count('extent') == 14 and ('search', STAGE_PARAGRAPHS) not in fake.calls
    # an empty page and find_rotation=False make no search call
    fake.calls.clear()
    assert stage(np.zeros((1, 8, 9, 1)), [np.zeros((1, 8, 9, 1))]) == [[]]
    crop.CropAndRotateParagraphs(find_rotation=False, search='device')(paragraph, arrays)
    assert not [call for call in fake.calls if call[0] in ('search', 'extent', 'crop')]


def test_stage_keeps_to_the_host_where_the_device_cannot_walk_the_tree():
    from univer_ocr_amd.my_model.crop import CropAndRotateParagraphs
    assert CropAndRotateParagraphs(eps=0.1, search='device').search == 'host'
    assert CropAndRotateParagraphs(eps=2.0, search='device').search == 'device'
    with pytest.raises(ValueError, match="'host' or 'device'"):
        CropAndRotateParagraphs(search='gpu')


def test_rotation_search_of_nothing_makes_no_call():
    from univer_ocr_amd.nn import ops
    assert ops.rotation_search(None, 0, []) == ([], [])


# ---- the model systems ---------------------------------------------------------------------------------------------------
def test_rotation_search_option_reaches_the_stage():
    from univer_ocr_amd.my_model import predict
    from univer_ocr_amd.my_model.model import (Modes, make_model_system, make_paragraph_crop_component, make_predict_system,
                                               make_train_char_system)
    makers = (lambda **kw: make_model_system((1, 32, 48, 1), mode=Modes.TRAIN_LINE, find_rotation=True, **kw),
              lambda **kw: make_train_char_system((1, 32, 16, 1), find_rotation=True, **kw),
              lambda **kw: make_predict_system((1, 32, 48, 1), **kw))
    for make in makers:
        for kw, expected in (({}, 'host'), ({'rotation_search': 'host'}, 'host'), ({'rotation_search': 'device'}, 'device')):
            system, _, names = make(**kw)
            assert system.components[names.index('ParagraphCrop')].stage.search == expected
    assert make_paragraph_crop_component(True, rotation_search='device').stage.search == 'device'
    assert not hasattr(make_paragraph_crop_component(False, rotation_search='device').stage, 'search'), 'the upright crop has no search'
    system = predict.load_model_system((1, 32, 48, 1), rotation_search='device')
    assert system.components[2].stage.search == 'device'
    assert predict.load_model_system((1, 32, 48, 1)).components[2].stage.search == 'host'
    with pytest.raises(ValueError, match="'host' or 'device'"):
        make_predict_system((1, 32, 48, 1), rotation_search='both')


# ---- the ABI -------------------------------------------------------------------------------------------------------------
def test_library_exports_the_new_entry_points():
    import ctypes as C
    from univer_ocr_amd.hip import lib as hiplib
    lib = hiplib.get_lib()
    assert lib.uocr_abi_version() == 4
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), f'{name} is not exported by {hiplib.lib_path()}'
    size = C.c_size_t(7)
    assert lib.uocr_rotation_search_workspace(0, C.byref(size)) == 0 and size.value == 0
    sizes = []
    for paragraphs in (1, 14, 29):
        assert lib.uocr_rotation_search_workspace(paragraphs, C.byref(size)) == 0
        sizes.append(size.value)
    assert sizes[0] >= 12 and sizes[1] == 14 * sizes[0] and sizes[2] == 29 * sizes[0], 'a node and two ranges per paragraph'
    assert lib.uocr_rotation_search_workspace(-1, C.byref(size)) == -1 and lib.uocr_rotation_search_workspace(3, None) == -1
    assert lib.uocr_rotation_search(None, None, 1, 1, 1, 0, 0, None, None, ROUNDS, None, None, None) == -1
    assert lib.uocr_ctx_last_rotation_search(None, None, None, None) == -1
