"""Host side of the text score: the rules of tests/text_score_rules.py -- the oracle of
tests/test_gpu_text_score.py, there being no scoring code in the reference to take a golden file from -- pinned against
a second implementation of the distance, against hand-made rows, and against the one property they are for: the one-hot
labels of every line of a generated page, made by the host restatements of the stages, READ as what was typed.  Then
the two entry points of the library, as far as they go without a GPU."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import page_rules as R
import text_score_rules as T
from conftest import ROOT
from test_char_label_host import char_label_rules
from test_label_host import flood_fill
from test_line_crop_host import line_crop_rules

NEW_SYMBOLS = {'uocr_text_score': 11, 'uocr_text_score_limits': 4}       # name -> arguments, the context included
N_CHARS = 162


# ---- distance ------------------------------------------------------------------------------------------------------------
def recursive_distance(a, b, canon):
    """the definition, memoised: d(i, j) between the first i ids of a and the first j of b"""
    @functools.lru_cache(maxsize=None)
    def d(i, j):
        if i == 0 or j == 0:
            return i + j
        return min(d(i - 1, j) + 1, d(i, j - 1) + 1, d(i - 1, j - 1) + (canon[a[i - 1]] != canon[b[j - 1]]))
    return d(len(a), len(b))


def test_distance_equals_the_recursive_definition():
    rng = np.random.default_rng(70)
    tables = [T.identity(5), np.array([0, 1, 1, 3, 3], np.int32)]
    differing = 0
    for case in range(3000):
        a = rng.integers(1, 5, rng.integers(0, 9)).tolist()
        b = rng.integers(1, 5, rng.integers(0, 9)).tolist()
        got = [T.distance(a, b, canon) for canon in tables]
        assert got == [recursive_distance(a, b, canon) for canon in tables], (a, b)
        assert got[1] <= got[0] and T.distance(b, a, tables[0]) == got[0]
        differing += got[1] < got[0]
    assert differing > 300, 'the table matters'


def test_distance_on_fixed_cases():
    ids = lambda word: [ord(c) - ord('a') + 1 for c in word]
    same = T.identity(27)
    assert T.distance(ids('kitten'), ids('sitting'), same) == 3
    assert T.distance(ids('flaw'), ids('lawn'), same) == 2
    for n in (0, 1, 7):
        assert T.distance([], ids('abcdefg')[:n], same) == n and T.distance(ids('abcdefg')[:n], [], same) == n
        assert T.distance(ids('abcdefg')[:n], ids('abcdefg')[:n], same) == 0
    one = np.zeros(27, np.int32)                                       # every id is every other: only the lengths count
    for n, m in ((0, 0), (3, 3), (2, 7), (9, 1)):
        assert T.distance(list(range(1, n + 1)), list(range(5, m + 5)), one) == abs(n - m)


# ---- reading -------------------------------------------------------------------------------------------------------------
def rows(*specs, n_chars=8, dtype=np.float64):
    """a matrix from one spec per row: an int is a one-hot row, anything else the row itself"""
    M = np.zeros((len(specs), n_chars), dtype)
    for r, spec in enumerate(specs):
        if isinstance(spec, int):
            M[r, spec] = 1.0
        else:
            M[r] = spec
    return M


def test_reading_on_hand_made_rows():
    a, b = 3, 5
    tie = [0, 0.5, 0, 0.5, 0, 0.5, 0, 0]
    nan = [0, 0, 0, 9, np.nan, 0, 0, 0]
    zero = [0.0] * 8
    negative_zero = [-1, -2, -0.0, -3, -1, -1, -1, -1]
    negative = [-5, -4, -3, -0.25, -2, -0.25, -7, -9]
    assert T.row_ids(rows(tie, nan, zero, negative_zero, negative, a, 0)) == [1, -1, -1, -1, 3, 3, 0]
    assert T.reading(rows(a, a, 0, a)) == [a, a] and T.reading(rows(a, a, a)) == [a]
    assert T.reading(rows(a, nan, a)) == [a, a] and T.reading(rows(a, zero, a)) == [a, a]
    assert T.reading(rows(a, negative_zero, a)) == [a, a], 'a row without a maximum ends a run'
    assert T.reading(rows(a, negative, a)) == [a], 'a negative maximum reads its id: the run goes on'
    assert T.reading(rows(0, 0, a, b, b, a, 0)) == [a, b, a] and T.reading(rows(0, zero, nan)) == []
    assert T.reading(rows(tie, 1, 3)) == [1, 3], 'ties take the first column'
    assert T.reading(rows(a, a, b, dtype=np.float16)) == [a, b]
    (d, n_expected, n_read), read, expected = T.score(rows(a, 0, b, b), rows(a, a, 0, b, 0, a), T.identity(8))
    assert (d, n_expected, n_read, read, expected) == (1, 3, 2, [a, b], [a, b, a])


def test_the_two_tables():
    from univer_ocr_amd.my_model.crop import CHARS, SIMILAR_PAIRS, canonical_ids
    assert len(CHARS) == N_CHARS and len(SIMILAR_PAIRS) == 18
    assert np.array_equal(canonical_ids(similar=False), T.identity(N_CHARS))
    canon = canonical_ids()
    assert np.array_equal(canon, T.look_alikes_equal(SIMILAR_PAIRS, N_CHARS)) and canon.dtype == np.int32
    for cyrillic, latin in SIMILAR_PAIRS:
        assert canon[cyrillic] == canon[latin] == cyrillic
    assert (canon != np.arange(N_CHARS)).sum() == 18
    assert T.distance([78, 3], [2, 3], canon) == 0 and T.distance([78, 3], [2, 3], T.identity(N_CHARS)) == 1


# ---- the labels of a generated page read as typed ------------------------------------------------------------------------
def labels_of_page(layers):
    """{(x0, y0) of the paragraph's box: [one-hot labels (W, N_CHARS) per line]} from the layers paragraph, line and char
    of one page, each (1, H, W, C) float64, through the host restatements of ParagraphCrop, LineCrop and CharLabel (the
    walk of tests/test_pages_host.py: read_page, which keeps the ids; this one keeps the labels)"""
    from univer_ocr_amd.my_model.crop import arrange_lines, line_boxes
    from univer_ocr_amd.my_model.model import make_divisible_by
    mask = layers['paragraph']
    labels, table = flood_fill(mask[0, :, :, 0] > np.mean(mask))
    found = {}
    for k, (_, _, y0, y1, x0, x1, _, _) in enumerate(table.tolist()):
        inside = (labels == k + 1)[None, :, :, None]
        line, char = (make_divisible_by((layers[tag] * inside)[:, y0:y1, x0:x1], 16, 16) for tag in ('line', 'char'))
        tables = []
        for channel in (0, 1):
            layer = line[0, :, :, channel]
            _, t = flood_fill(layer > 0.5 * (np.mean(layer) + np.max(layer)))
            tables.append((t[:, 6:8] / t[:, 1:2], t[:, 2:6]))
        arranged = arrange_lines(tables[0][0], tables[1][0])
        assert arranged is not None and arranged[2] is None, 'upright lines'
        boxes = line_boxes(tables[0][1], tables[1][1], arranged[0], arranged[1])
        found[(x0, y0)] = [char_label_rules(line_crop_rules(char, *box, None))[0] for box in boxes]
    return found


def test_the_labels_of_generated_pages_read_as_typed():
    atlas = R.load_atlas()
    lines = 0
    for number, (height, width) in ((0, (256, 512)), (1, (256, 512)), (2, (256, 512)), (40, (96, 384)), (41, (96, 384))):
        page = R.layout_page(atlas, 31, number, height, width)
        rendered = R.render_page(atlas, page, height, width, R.make_lut(np.float64))
        found = labels_of_page({tag: rendered[tag][None] for tag in ('paragraph', 'line', 'char')})
        typed = {(int(row[0]), int(row[1])): ids for row, ids in zip(page['paragraphs'], R.typed_ids(page))}
        assert sorted(found) == sorted(typed)
        for key, ids in typed.items():
            assert len(found[key]) == len(ids)
            for label, line_ids in zip(found[key], ids):
                assert label.shape[1] == N_CHARS and T.reading(label) == list(line_ids), f'page {number}, paragraph at {key}'
                assert T.score(label, label, T.identity(N_CHARS))[0] == (0, len(line_ids), len(line_ids))
                lines += 1
    assert lines >= 12


# ---- bindings --------------------------------------------------------------------------------------------------------------
def test_library_exports_the_new_entry_points():
    from univer_ocr_amd.hip import lib as hiplib
    assert set(NEW_SYMBOLS) <= set(hiplib.ABI_SYMBOLS)
    for name, arguments in NEW_SYMBOLS.items():
        assert len(hiplib._PROTOS[name]) == arguments, name
    header = open(os.path.join(ROOT, 'include', 'univer_hip.h')).read()
    assert all(f'int {name}(' in header for name in NEW_SYMBOLS)
    assert not [name for name in hiplib.ABI_SYMBOLS if name.startswith('uocr_ctx_last_') and 'text_score' in name]
    if not os.path.exists(hiplib.lib_path()):
        pytest.skip('libuniver_hip.so is not built')
    lib = hiplib.get_lib()
    assert lib.uocr_abi_version() == 4
    for name in NEW_SYMBOLS:
        getattr(lib, name)
    # a null context is an argument error before anything else is looked at
    assert lib.uocr_text_score(None, 0, 1, None, None, None, N_CHARS, None, None, None, None) == -1
    assert lib.uocr_text_score(None, 0, 0, None, None, None, N_CHARS, None, None, None, None) == -1
    # the limits need no context; a null pointer is refused before anything is written
    outs = [C.c_int(-1) for _ in range(4)]
    assert lib.uocr_text_score_limits(*[C.byref(out) for out in outs]) == 0
    rows_per_block, lines_per_launch, columns_per_panel, max_width = [out.value for out in outs]
    assert rows_per_block > 0 and lines_per_launch > 0 and max_width >= columns_per_panel > 0 and columns_per_panel % 64 == 0
    for null in range(4):
        outs = [C.c_int(-1) for _ in range(4)]
        args = [None if k == null else C.byref(out) for k, out in enumerate(outs)]
        assert lib.uocr_text_score_limits(*args) == -1, f'null pointer {null} was accepted'
        assert all(out.value == -1 for out in outs), f'wrote before refusing null pointer {null}'
