"""Host side of the page generator: the committed glyph atlas, the counter-based random numbers of
tests/page_rules.py against an implementation on Python integers, what the layout promises, and the one property the whole
feature is for: the label layers of a generated page, passed through the host restatements of the stages that read them
(the flood fill of test_label_host, my_model/crop.py: arrange_lines / line_boxes, the zoom rule of test_line_crop_host and
char_label_rules), say what was typed -- for every line of 36 generated pages of 256 x 512, of the small pages that hold
text and of one page per face that holds every character.  Nothing here needs a GPU."""
import importlib.util
import os

import numpy as np
import pytest

import page_rules as R
from conftest import ROOT
from test_char_label_host import char_label_rules
from test_label_host import flood_fill
from test_line_crop_host import line_crop_rules

NEW_SYMBOLS = ('uocr_page_layout', 'uocr_page_render', 'uocr_ctx_last_page_gen')
FONT_DIR = '/usr/share/fonts/truetype/dejavu'


@pytest.fixture(scope='module')
def atlas():
    return R.load_atlas()


@pytest.fixture(scope='module')
def pages(atlas):
    """200 pages of 256 x 512 past page number 2^32 and 200 pages of 64 x 128, laid out once"""
    return {(256, 512): [R.layout_page(atlas, 11, (1 << 32) + 5 + i, 256, 512) for i in range(200)],
            (64, 128): [R.layout_page(atlas, 12, i, 64, 128) for i in range(200)]}


# ---- the atlas file ------------------------------------------------------------------------------------------------------
def test_atlas_file_is_consistent(atlas):
    assert os.path.getsize(R.ATLAS_PATH) <= 1_000_000
    assert os.path.exists(os.path.join(os.path.dirname(R.ATLAS_PATH), 'glyphs.LICENSE.txt'))
    from univer_ocr_amd.my_model.pages import ATLAS_PATH
    assert os.path.dirname(ATLAS_PATH).endswith('my_model'), 'the package reads its own directory'
    if os.path.exists(ATLAS_PATH):                                   # installed by build.sh: the committed bytes, the licence beside them
        assert open(ATLAS_PATH, 'rb').read() == open(R.ATLAS_PATH, 'rb').read()
        assert os.path.exists(os.path.join(os.path.dirname(ATLAS_PATH), 'glyphs.LICENSE.txt'))
    metrics, adv, offset, cells = (atlas[k] for k in ('metrics', 'adv', 'offset', 'cells'))
    assert metrics.shape == (16, 7) and adv.shape == offset.shape == (16, R.N_IDS) and len(atlas['faces']) == 16
    assert cells.dtype == np.uint8 and metrics.dtype == adv.dtype == offset.dtype == np.int32
    assert sorted(set(metrics[:, R.SIZE].tolist())) == [12, 16, 24, 32]
    assert np.all(adv[:, 0] == 0) and np.all(adv[:, 1:] >= 4), 'one cell per id 1..161, none for the tab'
    assert np.all(metrics[:, R.X_HEIGHT] < metrics[:, R.ASCENT]) and np.all(metrics[:, R.X_HEIGHT] > 0)
    assert np.array_equal(metrics[:, R.HEIGHT], metrics[:, R.ASCENT] + metrics[:, R.DESCENT])
    assert np.array_equal(metrics[:, R.SPACING], metrics[:, R.SIZE] // 2)
    assert np.array_equal(metrics[:, R.PITCH], metrics[:, R.HEIGHT] + metrics[:, R.SPACING])
    sizes = (adv * metrics[:, R.HEIGHT:R.HEIGHT + 1]).reshape(-1)
    assert np.array_equal(offset.reshape(-1), np.concatenate([[0], np.cumsum(sizes)[:-1]])), 'cells follow each other'
    assert offset[-1, -1] + sizes[-1] == len(cells)
    # a 32-row crop of the tallest face keeps a sample of every 2 columns: the zoom factor is at least 0.5
    assert 32 / metrics[:, R.HEIGHT].max() >= 0.5
    # ink: every character but the space has some, and it reaches full coverage somewhere in every face
    for face in range(16):
        for char_id in range(2, R.N_IDS):
            cell = cells[offset[face, char_id]:offset[face, char_id] + sizes[face * R.N_IDS + char_id]]
            assert cell.max() > 64, (face, char_id)


def test_atlas_cells_equal_a_fresh_rasterisation(atlas):
    pytest.importorskip('PIL')
    if not os.path.exists(os.path.join(FONT_DIR, 'DejaVuSans.ttf')):
        pytest.skip('the DejaVu fonts are not installed')
    from PIL import ImageFont
    spec = importlib.util.spec_from_file_location('make_glyph_atlas', os.path.join(ROOT, 'tools', 'make_glyph_atlas.py'))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    from univer_ocr_amd.my_model.crop import CHARS
    for face in (0, 7, 10, 13):
        family, size = tool.FAMILIES[face // 4][1], tool.SIZES[face % 4]
        font = ImageFont.truetype(os.path.join(FONT_DIR, family), size)
        assert list(tool.face_metrics(font)) == atlas['metrics'][face].tolist()
        height = int(atlas['metrics'][face, R.HEIGHT])
        for char_id in (1, 2, 36, 70, 78, 87, 113, 130, 161):          # space, Cyrillic, digit, Latin (j: a negative bearing), ~
            cell = tool.glyph_cell(font, CHARS[char_id], height)
            start = atlas['offset'][face, char_id]
            assert cell.shape[1] == atlas['adv'][face, char_id]
            assert np.array_equal(cell.reshape(-1), atlas['cells'][start:start + cell.size]), (face, char_id)


# ---- random numbers --------------------------------------------------------------------------------------------------------
def python_draw(seed, page, attempt, slot, lo, hi):
    """section 2 on Python integers, written apart from page_rules.draws"""
    mask = (1 << 64) - 1
    index = ((page * 32 + attempt) * 1024 + slot) & mask
    z = (seed + (index + 1) * 0x9E3779B97F4A7C15) & mask
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & mask
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & mask
    z ^= z >> 31
    return lo + (((z >> 32) * (hi - lo + 1)) >> 32)


def test_draws_equal_python_integers():
    # splitmix64 itself: the first output of the generator seeded with 0 (the published test vector)
    assert python_draw(0, 0, 0, 0, 0, 0) == 0
    mask = (1 << 64) - 1
    z = (0 + 0x9E3779B97F4A7C15) & mask
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & mask
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & mask
    assert z ^ (z >> 31) == 0xE220A8397B1DCDAF
    slots = np.array([0, 1, 2, 3, 32, 64, 363, 512, 639, 1023])
    for seed, page in ((0, 0), (1234, 7), (2 ** 64 - 1, 2 ** 33 + 3), (0xDEADBEEF, 2 ** 63 + 11)):
        for attempt in (0, 31):
            for lo, hi in ((0, 15), (3, 30), (30, 100), (2, 161), (20, 20), (0, 2 ** 24)):
                got = R.draws(seed, page, attempt, slots, lo, hi).tolist()
                assert got == [python_draw(seed, page, attempt, int(s), lo, hi) for s in slots], (seed, page, attempt, lo, hi)


def test_draws_stay_in_range():
    slots = np.arange(1024)
    for lo, hi in ((5, 5), (0, 0), (2, 161), (0, 2 ** 24), (20, 2 ** 24 - 26)):      # lo == hi; the widest: a 2^24 wide page
        got = np.concatenate([R.draws(99, page, attempt, slots, lo, hi) for page in (0, 2 ** 40) for attempt in range(32)])
        assert got.min() >= lo and got.max() <= hi
        if hi - lo >= 160:
            assert got.min() < lo + (hi - lo) // 50 and got.max() > hi - (hi - lo) // 50, 'the whole range is reached'
    assert R.draw(1, 2, 3, 4, 0, 100) != R.draw(1, 2, 3, 5, 0, 100) or R.draw(1, 2, 3, 4, 0, 10 ** 6) != R.draw(1, 2, 3, 5, 0, 10 ** 6)


# ---- layout ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('size', [(256, 512), (64, 128)])
def test_layout_invariants(size, atlas, pages):
    height, width = size
    n_paragraphs = 0
    for page in pages[size]:
        paragraphs, lines, glyphs = page['paragraphs'], page['lines'], page['glyphs']
        assert len(paragraphs) <= R.MAX_PARAGRAPHS and len(lines) <= R.MAX_LINES and len(glyphs) <= R.MAX_GLYPHS
        n_paragraphs += len(paragraphs)
        next_line = next_glyph = 0
        for p, (x0, y0, w, h, face, n_lines, first_line, attempt) in enumerate(paragraphs.tolist()):
            assert x0 >= R.LEFT + R.MARGIN and x0 + w + R.MARGIN + R.LEFT <= width and y0 >= R.MARGIN and y0 + h + R.MARGIN <= height
            assert first_line == next_line and 1 <= n_lines <= R.MAX_WORDS and 0 <= face < 16 and 0 <= attempt < R.ATTEMPTS
            assert p == 0 or attempt > paragraphs[p - 1, 7]
            for bx, by, bw, bh, *_ in paragraphs[:p].tolist():
                gap_x, gap_y = max(bx - (x0 + w), x0 - (bx + bw)), max(by - (y0 + h), y0 - (by + bh))
                assert max(gap_x, gap_y) >= R.MARGIN, 'boxes are at least 3 pixels apart'
            metrics, adv = atlas['metrics'][face], atlas['adv'][face]
            assert h == n_lines * metrics[R.PITCH] - metrics[R.SPACING]
            widths = []
            for k, (left, y_ascent, line_w, g0, n) in enumerate(lines[first_line:first_line + n_lines].tolist()):
                assert (left, y_ascent) == (x0, y0 + k * metrics[R.PITCH]) and y_ascent + metrics[R.HEIGHT] <= y0 + h
                assert g0 == next_glyph and 1 <= n <= 100 and line_w <= w
                ids, pens = glyphs[g0:g0 + n, 1], glyphs[g0:g0 + n, 0]
                assert ids.min() >= 1 and ids.max() < R.N_IDS and ids[0] != 1 and ids[-1] != 1
                assert not np.any((ids[1:] == 1) & (ids[:-1] == 1)), 'one space between words'
                assert np.array_equal(pens, left + np.concatenate([[0], np.cumsum(adv[ids])[:-1]])) and line_w == adv[ids].sum()
                widths.append(line_w)
                next_glyph += n
            assert max(widths) == w
            next_line += n_lines
        assert (next_line, next_glyph) == (len(lines), len(glyphs))
    if size == (256, 512):
        assert n_paragraphs >= 400, 'a usual page holds some paragraphs'
    else:
        assert 0 < n_paragraphs < 100 and any(len(page['paragraphs']) == 0 for page in pages[size]), 'most attempts are dropped'


def test_wrapping_is_greedy(atlas):
    for attempt in range(32):
        face, text = R.attempt_text(5, 77, attempt, 16)
        wrap = R.draw(5, 77, attempt, 2, 30, 100)
        assert all(len(ids) <= wrap for ids in text)
        for this, after in zip(text, text[1:]):
            first_word = after[:after.index(1)] if 1 in after else after
            assert len(this) + 1 + len(first_word) > wrap, 'the next word did not fit'
        words = [w for ids in text for w in ''.join(chr(i) for i in ids).split(chr(1))]
        assert len(words) == R.draw(5, 77, attempt, 1, 3, 30) and all(1 <= len(w) <= 10 for w in words)


# ---- the labels say what was typed ---------------------------------------------------------------------------------------
def read_page(layers):
    """{(x0, y0) of the paragraph's box: [ids per line]} read from the layers paragraph, line and char of one page, each
    (1, H, W, C) float64, through the host restatements of ParagraphCrop, LineCrop and CharLabel"""
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
        found[(x0, y0)] = []
        for box in boxes:
            ids = char_label_rules(line_crop_rules(char, *box, None))[1].tolist()
            runs, run = [], []
            for i in ids + [0]:
                if i == 0:
                    runs += [run] if run else []
                    run = []
                elif not run or run[-1] != i:
                    run.append(i)
            found[(x0, y0)].append([i for run in runs for i in run])
    return found


def check_page_reads_as_typed(atlas, page, height, width):
    rendered = R.render_page(atlas, page, height, width, R.make_lut(np.float64))
    found = read_page({tag: rendered[tag][None] for tag in ('paragraph', 'line', 'char')})
    typed = {(int(row[0]), int(row[1])): ids for row, ids in zip(page['paragraphs'], R.typed_ids(page))}
    assert sorted(found) == sorted(typed), 'every paragraph is found, and nothing else'
    lines = 0
    for key, ids in typed.items():
        assert found[key] == ids, f'paragraph at {key}'
        lines += len(ids)
    return lines


@pytest.mark.parametrize('part', range(6))
def test_generated_pages_read_as_typed(part, atlas, pages):
    """36 pages of 256 x 512, six per case (the restated CharLabel is a Python loop per column), every line of each"""
    chosen = pages[(256, 512)][6 * part:6 * part + 6]
    lines = sum(check_page_reads_as_typed(atlas, page, 256, 512) for page in chosen)
    assert lines >= 6 * 4 and sum(len(page['paragraphs']) >= 3 for page in chosen) >= 3, 'pages with stacked paragraphs'


def test_small_generated_pages_read_as_typed(atlas, pages):
    """every page of 64 x 128 among the 200 that holds text at all"""
    small = [page for page in pages[(64, 128)] if len(page['paragraphs'])]
    assert sum(check_page_reads_as_typed(atlas, page, 64, 128) for page in small) >= len(small) >= 5


@pytest.mark.parametrize('face', range(16))
def test_every_character_of_every_face_reads_as_typed(face, atlas):
    """one paragraph per face that holds every id, a doubled character and the narrowest cell next to itself"""
    narrow = int(np.argmin(atlas['adv'][face][1:])) + 1
    ids = list(range(2, R.N_IDS)) + [narrow, narrow, 2, 2]
    text = [ids[i:i + 33] for i in range(0, len(ids), 33)]
    t_width, t_height = R.text_size(atlas, face, text)
    page = R.hand_page(atlas, [(R.LEFT + R.MARGIN, R.MARGIN, face, text)])
    assert check_page_reads_as_typed(atlas, page, t_height + 2 * R.MARGIN, t_width + 2 * (R.LEFT + R.MARGIN)) == len(text)


def test_render_gives_the_first_box_the_pixel_and_exact_values(atlas):
    lut = R.make_lut(np.float32)
    page = R.hand_page(atlas, [(2, 1, 0, [[80, 81]]), (6, 4, 4, [[90]])])       # overlapping boxes: the first one owns the overlap
    out = R.render_page(atlas, page, 40, 48, lut)
    assert out['image'][0, 0, 0] == np.float32(1.0) and out['monochrome'][0, 0, 0] == 0.0
    assert out['monochrome'].max() > 0.9 and out['image'].min() < 0.1, 'ink'
    assert np.array_equal(out['image'], lut[255 - np.round(out['monochrome'].astype(np.float64) * 255).astype(int)])
    for name, c in R.LAYERS[2:]:
        assert out[name].shape == (40, 48, c) and set(np.unique(out[name]).tolist()) <= {0.0, 1.0}
    alone = R.render_page(atlas, R.hand_page(atlas, [(2, 1, 0, [[80, 81]])]), 40, 48, lut)
    x0, y0, w, h = page['paragraphs'][0, :4]
    for name, _ in R.LAYERS:
        assert np.array_equal(out[name][y0:y0 + h, x0:x0 + w], alone[name][y0:y0 + h, x0:x0 + w]), name


# ---- bindings ----------------------------------------------------------------------------------------------------------------
def test_library_exports_the_new_entry_points():
    from univer_ocr_amd.hip import lib as hiplib
    assert set(NEW_SYMBOLS) <= set(hiplib.ABI_SYMBOLS)
    if not os.path.exists(hiplib.lib_path()):
        pytest.skip('libuniver_hip.so is not built')
    lib = hiplib.get_lib()
    assert lib.uocr_abi_version() == 4
    for name in NEW_SYMBOLS:
        getattr(lib, name)
    header = open(os.path.join(ROOT, 'include', 'univer_hip.h')).read()
    assert all(f'int {name}(' in header for name in NEW_SYMBOLS)
    # a null context is an argument error before anything else is looked at
    assert lib.uocr_ctx_last_page_gen(None, None, None, None, None) == -1
    assert lib.uocr_page_layout(None, 0, 0, 1, 8, 8, 1, None, None, None, None, None, None) == -1
    assert lib.uocr_page_render(None, 0, 1, 8, 8, *[None] * 4, 1, *[None] * 4, 0, *[None] * 6) == -1


def test_the_capacities_are_the_worst_cases():
    from univer_ocr_amd.nn import ops
    assert dict((name, rows) for name, rows, _ in ops.PAGE_TABLES) == {
        'paragraphs': R.MAX_PARAGRAPHS, 'lines': R.MAX_LINES, 'glyphs': R.MAX_GLYPHS}
    assert R.MAX_GLYPHS == 32 * (30 * 11) and tuple(ops.PAGE_LAYERS) == R.LAYERS


def test_train_model_knows_its_data_sources(monkeypatch):
    from univer_ocr_amd.my_model import train
    with pytest.raises(ValueError, match='generated'):
        train.train_model(data='drawn')
    monkeypatch.setenv('UOCR_TRAIN_DATA', 'sketched')
    with pytest.raises(ValueError, match='sketched'):
        train.train_model()
