"""The page generator's rules restated in plain Python / NumPy: the counter-based random numbers, the
layout of a page and its label layers.  The GPU tests take their expected values from here; tests/test_pages_host.py pins
the random numbers to an implementation on Python integers and checks what the layout promises.  A helper, not a test."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATLAS_PATH = os.path.join(ROOT, 'tests', 'golden', 'glyphs.npz')       # the committed bytes; build.sh installs them into the package

ATTEMPTS, MAX_WORDS, MAX_WORD, TRIES, MARGIN, LEFT = 32, 30, 10, 64, 3, 20
N_IDS = 162
MAX_PARAGRAPHS, MAX_LINES, MAX_GLYPHS = ATTEMPTS, ATTEMPTS * MAX_WORDS, ATTEMPTS * MAX_WORDS * (MAX_WORD + 1)
SIZE, ASCENT, DESCENT, HEIGHT, X_HEIGHT, SPACING, PITCH = range(7)        # columns of atlas['metrics']
GOLDEN, MIX_1, MIX_2 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)
LAYERS = (('image', 1), ('monochrome', 1), ('paragraph', 1), ('line', 2), ('char', 9))


def load_atlas():
    with np.load(ATLAS_PATH, allow_pickle=False) as f:
        return {key: f[key] for key in f.files}


def make_lut(dtype):
    """lut[cov] = cov / 255 in float64, then cast: what the host hands to the device"""
    return (np.arange(256) / 255).astype(dtype)


# ---- 2. random numbers ---------------------------------------------------------------------------------------------------
def draws(seed, page, attempt, slots, lo, hi):
    """the draws in [lo, hi] (scalars or arrays like slots) at `slots` of attempt `attempt` of page `page`, as int64"""
    with np.errstate(over='ignore'):
        key = np.uint64(((int(page) * 32 + int(attempt)) * 1024) % 2 ** 64)
        z = np.uint64(int(seed) % 2 ** 64) + (key + np.asarray(slots).astype(np.uint64) + np.uint64(1)) * GOLDEN
        z = (z ^ (z >> np.uint64(30))) * MIX_1
        z = (z ^ (z >> np.uint64(27))) * MIX_2
        z = z ^ (z >> np.uint64(31))
        span = (np.asarray(hi, np.int64) - np.asarray(lo, np.int64) + 1).astype(np.uint64)
        return np.asarray(lo, np.int64) + (((z >> np.uint64(32)) * span) >> np.uint64(32)).astype(np.int64)


def draw(seed, page, attempt, slot, lo, hi):
    return int(draws(seed, page, attempt, np.array([slot]), lo, hi)[0])


# ---- 3. layout -------------------------------------------------------------------------------------------------------------
def attempt_text(seed, page, attempt, n_faces):
    """(face, [[id, ...] per line]) of an attempt: greedy wrapping, one space (id 1) between the words of a line"""
    face = draw(seed, page, attempt, 0, 0, n_faces - 1)
    n_words = draw(seed, page, attempt, 1, 3, MAX_WORDS)
    wrap = draw(seed, page, attempt, 2, 30, 100)
    lengths = draws(seed, page, attempt, 3 + np.arange(n_words), 1, MAX_WORD)
    lines = []
    for j, length in enumerate(lengths.tolist()):
        word = draws(seed, page, attempt, 64 + MAX_WORD * j + np.arange(length), 2, N_IDS - 1).tolist()
        if lines and len(lines[-1]) + 1 + length <= wrap:
            lines[-1] += [1] + word
        else:
            lines.append(word)
    return face, lines


def place(atlas, x0, y0, face, text, first_line, first_glyph, attempt=0):
    """the table rows of the paragraph `text` ([[id, ...] per line]) in `face` at (x0, y0): (paragraph row, line rows,
    glyph rows)"""
    adv, pitch = atlas['adv'][face], int(atlas['metrics'][face, PITCH])
    lines, glyphs = [], []
    for k, ids in enumerate(text):
        pens = x0 + np.concatenate([[0], np.cumsum(adv[ids])])
        lines.append((x0, y0 + k * pitch, int(pens[-1] - x0), first_glyph + len(glyphs), len(ids)))
        glyphs += list(zip(pens[:-1].tolist(), ids))
    t_width, t_height = text_size(atlas, face, text)
    return (x0, y0, t_width, t_height, face, len(text), first_line, attempt), lines, glyphs


def text_size(atlas, face, text):
    metrics = atlas['metrics'][face]
    return (max(int(atlas['adv'][face][ids].sum()) for ids in text), len(text) * int(metrics[PITCH]) - int(metrics[SPACING]))


def as_page(paragraphs, lines, glyphs):
    return {'paragraphs': np.array(paragraphs, np.int32).reshape(-1, 8), 'lines': np.array(lines, np.int32).reshape(-1, 5),
            'glyphs': np.array(glyphs, np.int32).reshape(-1, 2)}


def hand_page(atlas, entries):
    """the tables of a hand-built page: entries = [(x0, y0, face, [[id, ...] per line]), ...]"""
    paragraphs, lines, glyphs = [], [], []
    for x0, y0, face, text in entries:
        row, new_lines, new_glyphs = place(atlas, x0, y0, face, text, len(lines), len(glyphs))
        paragraphs.append(row)
        lines += new_lines
        glyphs += new_glyphs
    return as_page(paragraphs, lines, glyphs)


def layout_page(atlas, seed, page, height, width):
    """the tables of page `page`: {'paragraphs': (n, 8), 'lines': (m, 5), 'glyphs': (g, 2)} int32"""
    paragraphs, lines, glyphs = [], [], []
    for attempt in range(ATTEMPTS):
        face, text = attempt_text(seed, page, attempt, len(atlas['metrics']))
        t_width, t_height = text_size(atlas, face, text)
        pw, ph = t_width + 2 * MARGIN, t_height + 2 * MARGIN
        x_hi, y_hi = width - pw - LEFT, height - ph
        if x_hi < LEFT or y_hi < 0:
            continue
        xs = draws(seed, page, attempt, 512 + 2 * np.arange(TRIES), LEFT, x_hi).tolist()
        ys = draws(seed, page, attempt, 513 + 2 * np.arange(TRIES), 0, y_hi).tolist()
        for x, y in zip(xs, ys):
            if not any(x < bx + bw and bx < x + pw and y < by + bh and by < y + ph for bx, by, bw, bh, *_ in paragraphs):
                row, new_lines, new_glyphs = place(atlas, x + MARGIN, y + MARGIN, face, text, len(lines), len(glyphs), attempt)
                paragraphs.append(row)
                lines += new_lines
                glyphs += new_glyphs
                break
    return as_page(paragraphs, lines, glyphs)


def counts_of(page):
    return np.array([len(page['paragraphs']), len(page['lines']), len(page['glyphs']), 0], np.int32)


def pack_tables(pages):
    """the tables of several pages as the device holds them, rows past the counts zero: paragraphs (n, 32, 8), lines
    (n, 960, 5), glyphs (n, 10560, 2), counts (n, 4)"""
    n = len(pages)
    out = {'paragraphs': np.zeros((n, MAX_PARAGRAPHS, 8), np.int32), 'lines': np.zeros((n, MAX_LINES, 5), np.int32),
           'glyphs': np.zeros((n, MAX_GLYPHS, 2), np.int32), 'counts': np.zeros((n, 4), np.int32)}
    for i, page in enumerate(pages):
        for key in ('paragraphs', 'lines', 'glyphs'):
            out[key][i, :len(page[key])] = page[key]
        out['counts'][i] = counts_of(page)
    return out


def texts(page, chars):
    """text[paragraph][line] of a page's tables"""
    return [[''.join(chars[i] for i in page['glyphs'][g0:g0 + n, 1]) for _, _, _, g0, n in page['lines'][first:first + count]]
            for *_, count, first, _ in page['paragraphs']]


def typed_ids(page):
    """ids[paragraph][line] of a page's tables"""
    return [[page['glyphs'][g0:g0 + n, 1].tolist() for _, _, _, g0, n in page['lines'][first:first + count]]
            for *_, count, first, _ in page['paragraphs']]


# ---- 4. layers ---------------------------------------------------------------------------------------------------------------
def render_page(atlas, page, height, width, lut):
    """the five layers of a page, {'image': (H, W, 1), 'monochrome', 'paragraph', 'line': (H, W, 2), 'char': (H, W, 9)} in
    lut.dtype.  Paragraphs are painted last to first, each over its whole box: the first box that holds a pixel owns it.
    Precondition: every line and every cell of a paragraph lies inside the paragraph's box, and line k lies at
    y0 + k * pitch -- what layout_page and hand_page make.  Bands and cells are painted unclipped, so tables outside that
    promise would differ from the kernel, which gives a pixel to its box first and reads the line from its row in the box."""
    cov = np.zeros((height, width), np.uint8)
    flags = {name: np.zeros((height, width, c), bool) for name, c in LAYERS[2:]}
    for x0, y0, w, h, face, n_lines, first_line, _ in page['paragraphs'][::-1].tolist():
        box = (slice(y0, y0 + h), slice(x0, x0 + w))
        cov[box] = 0
        for layer in flags.values():
            layer[box] = False
        flags['paragraph'][box] = True
        _, ascent, _, cell_h, x_height, _, pitch = atlas['metrics'][face].tolist()
        adv, offset = atlas['adv'][face], atlas['offset'][face]
        for left, y_ascent, line_w, g0, n in page['lines'][first_line:first_line + n_lines].tolist():
            rows = lambda a, b: (slice(y_ascent + a, min(y_ascent + b, y0 + h)), slice(left, left + line_w))
            flags['line'][rows(0, ascent) + (0,)] = True
            flags['line'][rows(ascent - x_height, cell_h) + (1,)] = True
            glyphs = page['glyphs'][g0:g0 + n].tolist()
            for g, (pen, char_id) in enumerate(glyphs):
                cell_w = int(adv[char_id])
                w10 = max(1, cell_w // 10)
                cell = atlas['cells'][offset[char_id]:offset[char_id] + cell_h * cell_w].reshape(cell_h, cell_w)
                band = slice(y_ascent, y_ascent + cell_h)
                cov[band, pen:pen + cell_w] = cell
                for k in range(8):
                    if char_id >> k & 1:
                        flags['char'][band, pen + w10:pen + cell_w - w10, k] = True
                if g < n - 1:
                    flags['char'][band, pen + cell_w - w10:pen + cell_w, 8] = True
                if g > 0:
                    flags['char'][band, pen:pen + min(cell_w, max(1, int(adv[glyphs[g - 1][1]]) // 10)), 8] = True
    out = {'image': lut[255 - cov.astype(np.int64)][:, :, None], 'monochrome': lut[cov][:, :, None]}
    out.update({name: layer.astype(lut.dtype) for name, layer in flags.items()})
    return out


def render_pages(atlas, pages, height, width, lut):
    """{layer: (n, H, W, C)} of several pages"""
    rendered = [render_page(atlas, page, height, width, lut) for page in pages]
    return {name: np.stack([r[name] for r in rendered]) for name, _ in LAYERS}
