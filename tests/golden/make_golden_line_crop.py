#!/usr/bin/env python3
"""Generate tests/golden/line_crop.npz: inputs and expected outputs of the LineCrop stage and of the TRAIN_CHAR model
system [ParagraphCrop, LineCrop, CharLabel, Char], taken from the REFERENCE (needs the reference checkout and scipy; see
make_golden.py, whose import stand-ins this script reuses by importing it).

    python tests/golden/make_golden_line_crop.py

Route taken: the reference's functions are called directly -- `label_layer` (interpreter/interpreter.py:16-21),
`rearrange_lines` (:42-82), `CropRotateAndZoomLines._func1` / `_func2` (:494-523) and `LabelChar._func1` (:547-571);
constructing the pool classes would start their worker processes.  The one expression that has no function of its own,
the (mean + max) / 2 threshold inside CropRotateAndZoomLines._func (:437-438), is restated as `thresholded`.  Only inputs
and outputs are stored.

Contents
  (a) gather/  gather/img{c}_{k}: (1, H, W, c) images with c = 1 and c = 9, k = 0 a tall one and k = 1 a wide one;
               gather/cases: int32 rows (k, y0, x0, box_h, box_w); per case i, channel count c and rotation r in 0 / 90 / 180 / 270 (0: the reference's None)
               gather/{i}/c{c}/r{r} = _func2(image, box, rotation, 32, 8).  The boxes: 32 x 40 (zf = 1), 16 x 20 (zf = 2),
               64 x 10 (an output column on an exact half), 33 x 31, 5 x 8, 37 x 64 (scipy writes 0 into the last
               column), a height whose last ROW comes out 0 (searched below 130; stored only if there is one), 64 x 1
               (the zoom is empty: all of the 32 x 8 result is padding), 32 x 3 (padded to 8), 32 x 8 (not padded),
               32 x 257 (wide)
  (b) stage/   stage/names; per paragraph {n}: stage/{n}/mask (1, H, W, 2), /img1, /img9 the companions, /rotation (0 for
               None), /boxes int32 (lines, 4) = y0, x0, height, width in output order, /c{c}/{line} every result array.
               upright: three lines whose label order differs from the reading order; shared: a bottom that is the
               nearest of two tops; stray: a bottom that no top takes; turned: two plain lines.  Each is stored in the
               orientation named by its rotation; all four rotations occur.
  (c) system/  a page of 96 x 48 with two paragraphs, of two lines and of one line: system/page/{monochrome, paragraph,
               line, char}; the paragraphs' crops by the route of make_golden_crops.py, padded by the reference's
               make_divisible_by(16, 16), go through LineCrop and CharLabel: system/mono{p}_{l}, system/char{p}_{l},
               system/labels{p}_{l}; the reference's Char net (make_char, analytic weights) trained by ONE
               ModelSystem.train call through the reference's CharSelector (one step per line), once with
               Momentum(lr=0.01, momentum=0) and once with Adam(lr=0.0015): accumulated losses, char_pred[p][l] and the
               final weights under system/sgd/ and system/adam/, with the keys char_label.npz uses.

Every value of (a) and (b) is a multiple of 1/64 in [1/64, 1]: exact in binary16, and a zero in a result can only be
scipy's artefact or padding.  All images, masks, crops and labels are STORED as binary16 (the archive has to stay small),
which holds every one of them exactly; the reference computed them in float64.  The page layers of (c) are multiples of 1/64 in [0, 1].  Every mask value lies more than
1e-3 from its channel's threshold and every char value more than 1e-3 from its line's (asserted), so that a float32 or
binary16 mean cannot flip a pixel: the reference alone decides every pixel.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (installs the stand-ins, puts the reference on sys.path)
from make_golden_char_label import check_margin, encode  # noqa: E402
from make_golden_crops import reference_crops, sample_prediction, save_reproducible  # noqa: E402

from components.interpreter import interpreter as ref_interp  # noqa: E402
from components.my_model import model as ref_mm  # noqa: E402
from components.nn import optimizers as ref_opt  # noqa: E402
from components.nn.model_system import ModelComponent, ModelSystem  # noqa: E402
from components.primitives import BITS_COUNT, CHARS  # noqa: E402

MARGIN = 1e-3
ZOOMED_HEIGHT, MINIMAL_WIDTH = ref_mm.CHAR_INPUT_HEIGHT, ref_mm.CHAR_FIXED_WIDTH
N_CHARS = len(CHARS)
assert (ZOOMED_HEIGHT, MINIMAL_WIDTH, BITS_COUNT, N_CHARS) == (32, 8, 8, 162)
ROTATIONS = (None, 90, 180, 270)


def levels(r, shape):
    """multiples of 1/64 in [1/64, 1].  A 1-channel image draws every element on its own, from the 32 even levels; a wider one draws every PIXEL
    from 16 channel vectors, each a draw of distinct levels without replacement (the archive has to stay small: a pixel is
    then one repeated string to the compressor, while neighbouring pixels still differ and no two channels of a pixel
    are equal)"""
    if shape[-1] == 1:
        return r.integers(1, 33, shape) / 32.0
    book = np.array([r.permutation(64)[:shape[-1]] + 1 for _ in range(16)]) / 64.0
    return book[r.integers(0, len(book), shape[:-1])]


def half(a):
    """stored as binary16, which holds every value exactly"""
    assert np.array_equal(a.astype(np.float16).astype(np.float64), a)
    return a.astype(np.float16)


def thresholded(arr):
    return arr > 0.5 * (np.mean(arr) + np.max(arr))                # interpreter.py:437-438


def check_mask(name, mask):
    for ch in range(2):
        layer = mask[..., ch]
        t = 0.5 * (np.mean(layer) + np.max(layer))
        assert np.min(np.abs(layer - t)) > MARGIN, f'{name}: a value of channel {ch} lies within {MARGIN} of its threshold'


def reference_lines(mask, arrays):
    """CropRotateAndZoomLines._func (interpreter.py:436-492) for ONE paragraph without the pool:
    (rotation, boxes in output order, result[array_id][line_id])"""
    top, bottom = thresholded(mask[:, :, :, 0:1]), thresholded(mask[:, :, :, 1:2])
    tops, bottoms, rotation = ref_interp.rearrange_lines(ref_interp.label_layer(top), ref_interp.label_layer(bottom))
    boxes, result = [], [[] for _ in arrays]
    for top_mask, bottom_mask in zip(tops, bottoms):
        y, x = ref_interp.CropRotateAndZoomLines._func1(top_mask, bottom_mask)
        boxes.append((y.start, x.start, y.stop - y.start, x.stop - x.start))
        for i, image in enumerate(arrays):
            result[i].append(ref_interp.CropRotateAndZoomLines._func2(image, y, x, rotation, ZOOMED_HEIGHT, MINIMAL_WIDTH))
    return rotation, np.array(boxes, np.int32).reshape(-1, 4), result


# ---- (a) ------------------------------------------------------------------------------------------------------------
def last_index_is_artefact(n_in, n_out):
    return n_out > 1 and (n_out - 1) * ((n_in - 1) / (n_out - 1)) > n_in - 1


def hits_exact_half(n_in, n_out):
    return n_out > 1 and any((j * ((n_in - 1) / (n_out - 1))) % 1.0 == 0.5 for j in range(n_out))


def gen_gather(out):
    r = np.random.default_rng(31)
    boxes = [(32, 40), (16, 20), (64, 10), (33, 31), (5, 8), (37, 64)]
    last_row = [h for h in range(2, 130) if last_index_is_artefact(h, ZOOMED_HEIGHT)]
    print(f'heights below 130 whose last zoomed row is an artefact: {last_row}')
    if last_row:
        boxes.append((last_row[0], 23))
    boxes += [(64, 1), (32, 3), (32, 8), (32, 257)]
    # two images per channel count (the archive has to stay small): a wide one for the boxes wider than 64, a tall one
    wide = [bw > 64 for _, bw in boxes]
    sizes = [(max(bh for (bh, _), f in zip(boxes, wide) if f == flag) + 5, max(bw for (_, bw), f in zip(boxes, wide) if f == flag) + 7)
             for flag in (False, True)]
    images = {c: [levels(r, (1, h, w, c)) for h, w in sizes] for c in (1, 9)}
    cases, seen = [], set()
    for i, (bh, bw) in enumerate(boxes):
        height, width = sizes[wide[i]]
        y0, x0 = int(r.integers(1, height - bh)), int(r.integers(1, width - bw))
        cases.append((int(wide[i]), y0, x0, bh, bw))
        for rotation in ROTATIONS:
            rh, rw = (bh, bw) if rotation in (None, 180) else (bw, bh)
            zoom_w = int(round(rw * (ZOOMED_HEIGHT / rh)))
            for c, per_size in images.items():
                image = per_size[wide[i]]
                res = ref_interp.CropRotateAndZoomLines._func2(image, slice(y0, y0 + bh), slice(x0, x0 + bw), rotation,
                                                               ZOOMED_HEIGHT, MINIMAL_WIDTH)
                assert res.shape == (1, ZOOMED_HEIGHT, max(zoom_w, MINIMAL_WIDTH), c), (bh, bw, rotation, res.shape)
                out[f'gather/{i}/c{c}/r{rotation or 0}'] = half(res)
                zoomed = res[:, :, :zoom_w]
                if zoom_w and not zoomed[:, :, -1].any():
                    assert last_index_is_artefact(rw, zoom_w) and zoomed[:, :-1, :-1].all()
                    seen.add('artefact column')
                if zoom_w and not zoomed[:, -1].any():
                    assert last_index_is_artefact(rh, ZOOMED_HEIGHT) and zoomed[:, :-1, :-1].all()
                    seen.add('artefact row')
                assert not res[:, :, zoom_w:].any()
            seen |= {'exact half'} if hits_exact_half(rw, zoom_w) else set()
            seen |= {'empty'} if zoom_w == 0 else set()
            seen |= {'padded'} if 0 < zoom_w < MINIMAL_WIDTH else set()
        print(f'gather {i}: {bh} x {bw} at ({y0}, {x0})')
    assert seen >= {'artefact column', 'exact half', 'empty', 'padded'}, seen
    assert ('artefact row' in seen) == bool(last_row), seen
    for c, per_size in images.items():
        out[f'gather/img{c}_0'], out[f'gather/img{c}_1'] = half(per_size[0]), half(per_size[1])
    out['gather/cases'] = np.array(cases, np.int32)


# ---- (b) ------------------------------------------------------------------------------------------------------------
def paragraph(h, w, tops, bottoms, r):
    """(1, h, w, 2) mask: rectangles (y0, y1, x0, x1) of [48, 64] / 64 on a ground of [1, 4] / 64, tops in channel 0"""
    mask = r.integers(1, 5, (1, h, w, 2)) / 64.0
    for ch, rects in enumerate((tops, bottoms)):
        for y0, y1, x0, x1 in rects:
            mask[0, y0:y1, x0:x1, ch] = r.integers(48, 65, (y1 - y0, x1 - x0)) / 64.0
    return mask


def stage_paragraphs(r):
    """name -> (mask in upright layout, quarter turns np.rot90 applies to the whole paragraph before it is stored)"""
    return {
        # B's top and bottom each have a spur that starts above A's: scipy labels B's components first
        'upright': (paragraph(52, 50, [(3, 7, 20, 46), (20, 24, 5, 46), (3, 20, 5, 6), (36, 40, 8, 40)],
                              [(10, 14, 20, 46), (28, 32, 3, 46), (8, 28, 3, 4), (44, 48, 8, 44)], r), 0),
        # both of the first two tops are nearest to the first bottom
        'shared': (paragraph(48, 40, [(3, 7, 4, 30), (15, 19, 6, 34), (30, 34, 4, 36)], [(9, 13, 4, 34), (38, 42, 4, 30)], r), 1),
        'turned': (paragraph(40, 44, [(3, 6, 5, 40), (20, 23, 9, 36)], [(12, 15, 5, 38), (30, 33, 9, 40)], r), 2),
        # a third bottom at the foot of the paragraph that no top takes
        'stray': (paragraph(52, 36, [(3, 7, 4, 30), (22, 26, 4, 32)], [(10, 14, 4, 32), (30, 34, 6, 30), (46, 49, 10, 20)], r), 3),
    }


def gen_stage(out):
    r = np.random.default_rng(32)
    rotations, names = set(), []
    for name, (upright, turns) in stage_paragraphs(r).items():
        mask = np.ascontiguousarray(np.rot90(upright, turns, axes=(1, 2)))
        check_mask(name, mask)
        images = {c: levels(r, (*mask.shape[:3], c)) for c in (1, 9)}
        top, bottom = ref_interp.label_layer(thresholded(mask[..., 0:1])), ref_interp.label_layer(thresholded(mask[..., 1:2]))
        rotation, boxes, result = reference_lines(mask, [images[1], images[9]])
        rotations.add(rotation)
        names.append(name)
        out[f'stage/{name}/mask'], out[f'stage/{name}/img1'], out[f'stage/{name}/img9'] = half(mask), half(images[1]), half(images[9])
        out[f'stage/{name}/rotation'], out[f'stage/{name}/boxes'] = np.array(rotation or 0), boxes
        for c, per_line in zip((1, 9), result):
            for line, res in enumerate(per_line):
                out[f'stage/{name}/c{c}/{line}'] = half(res)
        print(f'stage {name}: {mask.shape[1]} x {mask.shape[2]}, {len(top)} tops, {len(bottom)} bottoms, rotation {rotation}, '
              f'{len(boxes)} lines {[tuple(b) for b in boxes.tolist()]}')
        centers = [ref_interp.ndimage.center_of_mass(m)[1:3] for m in top]
        if name == 'upright':
            assert rotation is None and len(boxes) == 3
            assert centers != sorted(centers), 'label order equals reading order'
        if name == 'shared':
            assert len(top) == 3 and len(bottom) == 2 and len(boxes) == 3
        if name == 'stray':
            assert len(top) == 2 and len(bottom) == 3 and len(boxes) == 2
    assert rotations == set(ROTATIONS), rotations
    out['stage/names'] = np.array(names)


# ---- (c) ------------------------------------------------------------------------------------------------------------
def system_page(r):
    h, w = 96, 48
    page = {'monochrome': r.integers(0, 65, (1, h, w, 1)) / 64.0, 'paragraph': np.zeros((1, h, w, 1)),
            'line': np.zeros((1, h, w, 2)), 'char': np.zeros((1, h, w, BITS_COUNT + 1))}
    codes = np.zeros((h, w), np.int64)
    # (paragraph rows, columns, [(top row, bottom row) of every line])
    for (y0, y1, x0, x1), lines in (((4, 52, 6, 38), [(7, 21), (30, 46)]), ((62, 88, 4, 38), [(66, 80)])):
        page['paragraph'][0, y0:y1, x0:x1, 0] = 1.0
        for top, bottom in lines:
            page['line'][0, top:top + 2, x0 + 2:x1 - 2, 0] = 1.0
            page['line'][0, bottom - 2:bottom, x0 + 2:x1 - 2, 1] = 1.0
            for x in range(x0 + 2, x1 - 2, 4):                      # a class per glyph of four columns
                codes[top:bottom, x:x + 4] = r.integers(1, N_CHARS)
    noise = r.random((h, w)) < 0.15
    codes = np.where(noise & (codes > 0), r.integers(0, 2 ** BITS_COUNT, (h, w)), codes)
    page['char'] = encode(codes, r, low=(0, 2), high=(61, 64))
    return page


def gen_system(out):
    r = np.random.default_rng(33)
    page = system_page(r)
    for tag, layer in page.items():
        out[f'system/page/{tag}'] = half(layer)
    assert np.min(np.abs(page['paragraph'] - np.mean(page['paragraph']))) > MARGIN
    crops = reference_crops(page['paragraph'], [page['monochrome'], page['line'], page['char']])
    padded = [[ref_mm.make_divisible_by(c, 16, 16) for c in per_array] for per_array in crops]   # model.py:552-574
    assert [c.shape[1:3] for c in padded[0]] == [(64, 48), (32, 48)], [c.shape for c in padded[0]]
    monos, chars, labels = [], [], []
    for p in range(2):
        check_mask(f'paragraph {p}', padded[1][p])
        rotation, boxes, (mono, char) = reference_lines(padded[1][p], [padded[0][p], padded[2][p]])   # model.py:595-612
        assert rotation is None and len(boxes) == (2, 1)[p], (rotation, boxes)
        monos.append(mono), chars.append(char), labels.append([])
        for l, x in enumerate(char):
            check_margin(f'char{p}_{l}', x)
            labels[p].append(ref_interp.LabelChar._func1(x))     # model.py:614-623
            assert labels[p][l].any(axis=1).sum() > x.shape[2] // 2, 'hardly a column has a class'
            out[f'system/mono{p}_{l}'], out[f'system/char{p}_{l}'], out[f'system/labels{p}_{l}'] = half(mono[l]), half(x), half(labels[p][l])
        print(f'system paragraph {p}: lines {[tuple(b) for b in boxes.tolist()]} -> {[m.shape[1:3] for m in mono]}')
    for tag, make_opt in (('sgd', lambda: ref_opt.Momentum(lr=0.01, momentum=0)), ('adam', lambda: ref_opt.Adam(lr=0.0015))):
        np.random.seed(11)
        char_net = ref_mm.make_char(monos[0][0].shape, make_opt())
        mg.set_analytic_weights(char_net)
        system = ModelSystem([ModelComponent(
            'Char', char_net, ref_mm.CharSelector('cropped_2_monochrome', 'char_labels', 'char_pred'), delist_result=True)])
        context = {'cropped_2_monochrome': [list(m) for m in monos], 'char_labels': [list(v) for v in labels]}
        system.train(context)                                      # three steps: one per line
        entry = context['losses']['Char']
        assert len(entry['output_losses']) == 3 and [len(v) for v in context['char_pred']] == [2, 1]
        out[f'system/{tag}/train/Char/output_losses'] = np.array(entry['output_losses'])
        out[f'system/{tag}/train/Char/regularization_loss'] = np.array(entry['regularization_loss'])
        for p, per_line in enumerate(context['char_pred']):
            for l, pred in enumerate(per_line):
                assert pred.shape == (monos[p][l].shape[2], N_CHARS)
                sample_prediction(f'system/{tag}/train/char_pred{p}_{l}', pred, out)
        for pname, param in char_net.params().items():
            mg.sample_param(f'system/{tag}/final/{pname}', param.value, out)


def main():
    out = {}
    gen_gather(out)
    gen_stage(out)
    gen_system(out)
    save_reproducible('line_crop', out)


if __name__ == '__main__':
    main()
