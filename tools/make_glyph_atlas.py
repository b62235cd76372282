#!/usr/bin/env python
"""Rasterise the glyph atlas of the page generator.  The package reads
univer-ocr_amd/my_model/glyphs.npz; the committed bytes are tests/golden/glyphs.npz, where the repository keeps its binary
data, and ./build.sh installs them (with glyphs.LICENSE.txt) into the package.  This tool writes the committed file and
the installed one.

Needs Pillow and the DejaVu TrueType files (fonts-dejavu-core); neither is needed afterwards: the atlas is committed.
16 faces: DejaVu Sans, Sans Bold, Serif, Serif Bold at 12, 16, 24 and 32 pixels.  Per face the integers
    size, ascent, descent, height = ascent + descent, x_height = rows of the mask of 'x', spacing = size // 2,
    pitch = height + spacing
and per character id 1..161 of my_model/crop.py: CHARS one cell of `height` rows by `adv` columns of coverage 0..255,
    adv = max(4, ceil(advance), left bearing + bitmap width)
with the bitmap at its bearing, clamped to the cell: all ink of a glyph lies in its own cell.  Id 0 (the tab) has no
cell.  Arrays of the file:
    faces    (16,) str       names
    metrics  (16, 7) int32   the integers above, in that order
    adv      (16, 162) int32 columns of every cell (0 for id 0)
    offset   (16, 162) int32 start of every cell in `cells`; cells follow each other by face, then by id
    cells    (n,) uint8      coverage, row-major per cell

    python tools/make_glyph_atlas.py [--fonts /usr/share/fonts/truetype/dejavu] [--out PATH]
"""
import argparse
import math
import os
import shutil
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FAMILIES = (('DejaVuSans', 'DejaVuSans.ttf'), ('DejaVuSans-Bold', 'DejaVuSans-Bold.ttf'),
            ('DejaVuSerif', 'DejaVuSerif.ttf'), ('DejaVuSerif-Bold', 'DejaVuSerif-Bold.ttf'))
SIZES = (12, 16, 24, 32)
FONT_DIR = '/usr/share/fonts/truetype/dejavu'
MIN_ADV = 4


def face_metrics(font):
    """(size, ascent, descent, height, x_height, spacing, pitch) of a PIL font"""
    ascent, descent = font.getmetrics()
    height, spacing = ascent + descent, font.size // 2
    return (int(font.size), ascent, descent, height, font.getmask('x').size[1], spacing, height + spacing)


def glyph_cell(font, char, height):
    """the (height, adv) uint8 cell of one character: its mask at (left bearing, rows below the ascender line), moved
    into the cell where a bearing is negative or the ink passes the descender line"""
    mask, (left, top) = font.getmask2(char, mode='L')
    bw, bh = mask.size
    if not (bw and bh):                                  # the space: no ink
        bw = bh = 0
    bitmap = np.asarray(mask, np.uint8).reshape(bh, bw)[:height]
    bh = bitmap.shape[0]
    left, top = max(0, int(left)), min(max(0, int(top)), height - bh)
    adv = max(MIN_ADV, math.ceil(font.getlength(char)), left + bw)
    cell = np.zeros((height, adv), np.uint8)
    cell[top:top + bh, left:left + bw] = bitmap
    return cell


def build(font_dir=FONT_DIR):
    from PIL import ImageFont

    from univer_ocr_amd.my_model.crop import CHARS
    names, metrics, adv, offset, cells, start = [], [], [], [], [], 0
    for family, file_name in FAMILIES:
        for size in SIZES:
            font = ImageFont.truetype(os.path.join(font_dir, file_name), size)
            m = face_metrics(font)
            names.append(f'{family}-{size}')
            metrics.append(m)
            face_adv, face_offset = [0], [start]
            for char in CHARS[1:]:
                cell = glyph_cell(font, char, m[3])
                face_adv.append(cell.shape[1])
                face_offset.append(start)
                cells.append(cell.reshape(-1))
                start += cell.size
            adv.append(face_adv)
            offset.append(face_offset)
    return {'faces': np.array(names), 'metrics': np.array(metrics, np.int32), 'adv': np.array(adv, np.int32),
            'offset': np.array(offset, np.int32), 'cells': np.concatenate(cells)}


def main():
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    parser.add_argument('--fonts', default=FONT_DIR)
    parser.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'glyphs.npz'))
    args = parser.parse_args()
    atlas = build(args.fonts)
    np.savez_compressed(args.out, **atlas)
    if os.path.abspath(args.out) == os.path.join(ROOT, 'tests', 'golden', 'glyphs.npz'):
        shutil.copyfile(args.out, os.path.join(ROOT, 'univer-ocr_amd', 'my_model', 'glyphs.npz'))
    size = os.path.getsize(args.out)
    print(f'{args.out}: {len(atlas["faces"])} faces, {atlas["cells"].size} cell bytes, {size} bytes on disk')
    if size > 1_000_000:
        raise SystemExit('the atlas must stay within 1 MB')


if __name__ == '__main__':
    main()
