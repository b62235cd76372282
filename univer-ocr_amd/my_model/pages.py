"""Training pages generated where they are used: the reference's generate_data
(image_generator/generate.py: LayeredImage.add_paragraph) draws random text in random fonts and writes every label layer
from the same geometry; here the layout and the layers are two kernel calls (nn/ops.py: page_layout, page_render) over a
glyph atlas (glyphs.npz in this directory, made by tools/make_glyph_atlas.py from the DejaVu fonts, glyphs.LICENSE.txt
beside it; build.sh installs both from tests/golden/, where the repository keeps its binary data), integer arithmetic only.
Neither Pillow nor the fonts are needed at run time.  A page is a pure function of (seed, page number): nothing is cached
and nothing repeats.
"""
import os

import numpy as np

from ..nn import ops
from ..nn.gpu import CP
from .crop import CHARS

ATLAS_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'glyphs.npz')
LAYER_TAGS = tuple(name for name, _ in ops.PAGE_LAYERS)


class GlyphAtlas:
    """The atlas file, loaded once per process (`host`) and uploaded once per device (`device()`): faces (F,) names,
    metrics (F, 7) = size, ascent, descent, height, x_height, spacing, pitch, adv and offset (F, 162), cells (n,) uint8."""

    _shared = None

    def __init__(self, path=ATLAS_PATH):
        if not os.path.exists(path):
            raise FileNotFoundError(f'{path} not found: ./build.sh (or __graft_entry__.build()) installs it')
        with np.load(path, allow_pickle=False) as f:
            self.host = {key: f[key] for key in f.files}
        if self.host['adv'].shape[1] != len(CHARS):
            raise ValueError(f'{path}: {self.host["adv"].shape[1]} character ids, the table has {len(CHARS)}')
        self._device, self._luts = {}, {}

    @classmethod
    def shared(cls):
        if cls._shared is None:
            cls._shared = cls()
        return cls._shared

    def device(self):
        """{'metrics', 'adv', 'offset', 'cells'} as DeviceArrays on the current device"""
        key = str(CP.storage_device())
        if key not in self._device:
            self._device[key] = {name: CP.copy(self.host[name], np.uint8 if name == 'cells' else np.int32)
                                 for name in ('metrics', 'adv', 'offset', 'cells')}
        return self._device[key]

    def lut(self, dtype):
        """cov / 255 for cov = 0..255, computed in float64 and cast to dtype, on the current device"""
        key = (str(CP.storage_device()), np.dtype(dtype))
        if key not in self._luts:
            self._luts[key] = CP.copy(np.arange(256) / 255, dtype)
        return self._luts[key]


class GeneratedPages:
    """Dataset-like source with the reference's `get(index, layer_tags=...)` call shape (my_model/datasets.py:88-161):
    batch `index` holds pages index * batch .. index * batch + batch - 1 of the stream `seed`, so it can be made again
    from (seed, index), and no two indices share a page.  `get` returns DeviceArrays: image, monochrome, paragraph
    (B, H, W, 1), line (B, H, W, 2), char (B, H, W, 9) in `dtype` (default: the compute dtype).  `length` is what
    len() says -- an epoch for the Trainer; any index >= 0 is served."""

    def __init__(self, batch, height=256, width=512, seed=1234, length=4, dtype=None, atlas=None):
        self.batch, self.height, self.width = int(batch), int(height), int(width)
        self.seed, self.length, self.dtype = int(seed), int(length), dtype
        self.atlas = GlyphAtlas.shared() if atlas is None else atlas

    def __len__(self):
        return self.length

    def tables(self, index, first_page=None, n_pages=None):
        """the tables of batch `index`, or of the n_pages pages from page number first_page on"""
        first_page, n_pages = (int(index) * self.batch, self.batch) if first_page is None else (int(first_page), int(n_pages))
        return ops.page_layout(self.atlas.device(), self.seed, first_page, n_pages, self.height, self.width)

    def get(self, index, layer_tags=None, first_page=None, n_pages=None):
        """the layers of batch `index`, or of the n_pages pages from page number first_page on: a page's bytes depend on
        (seed, page number) alone, not on the batch it is made in"""
        dtype = CP.dtype if self.dtype is None else np.dtype(self.dtype)
        tables = self.tables(index, first_page, n_pages)
        layers = ops.page_render(self.atlas.device(), tables, self.height, self.width, self.atlas.lut(dtype))
        return layers if layer_tags is None else {tag: layers[tag] for tag in layer_tags}

    def texts(self, index, first_page=None, n_pages=None):
        """text[page][paragraph][line] of batch `index` (or of the pages from first_page on), read from its tables: the
        shape predict_text returns per page"""
        tables = {name: a.numpy() for name, a in self.tables(index, first_page, n_pages).items()}
        result = []
        for paragraphs, lines, glyphs, counts in zip(*(tables[k] for k in ('paragraphs', 'lines', 'glyphs', 'counts'))):
            result.append([[''.join(CHARS[i] for i in glyphs[g0:g0 + n, 1]) for _, _, _, g0, n in lines[first:first + count]]
                           for *_, count, first, _ in paragraphs[:counts[0]]])
        return result


class PagesWithText:
    """The pages of a GeneratedPages source that hold at least one line, one at a time: get(index) is the index-th such
    page of the stream alone, (1, H, W, C) per layer -- what the page-by-page systems (TRAIN_LINE,
    make_train_char_system) take; their epoch loop expects a loss from every page, and a page may be empty.  Reads the
    counts of the batches it walks over (16 bytes per page), once; a page it serves is laid out and rendered alone."""

    SEARCH_BATCHES = 64            # batches without a single line before the page size is called too small

    def __init__(self, source, length):
        self.source, self.length = source, int(length)
        self._found, self._next_batch = [], 0

    def __len__(self):
        return self.length

    def page_of(self, index):
        """the page number of the index-th page with text"""
        barren = 0
        while len(self._found) <= index:
            counts = self.source.tables(self._next_batch)['counts'].numpy()
            rows = [self._next_batch * self.source.batch + row for row in range(self.source.batch) if counts[row, 1] > 0]
            barren = 0 if rows else barren + 1
            if barren == self.SEARCH_BATCHES:
                raise ValueError(f'PagesWithText: no text fits pages of {self.source.height} x {self.source.width}')
            self._found += rows
            self._next_batch += 1
        return self._found[index]

    def get(self, index, layer_tags=None):
        return self.source.get(None, layer_tags, first_page=self.page_of(int(index)), n_pages=1)

    def texts(self, index):
        return self.source.texts(None, first_page=self.page_of(int(index)), n_pages=1)[0]
