#!/usr/bin/env python3
"""Generate tests/golden/rotation.npz: inputs and expected outputs of the rotation search of the ParagraphCrop stage,
taken from the REFERENCE (needs the reference checkout and scipy; see make_golden.py, whose import stand-ins this script
reuses by importing it).

    python tests/golden/make_golden_rotation.py

Route taken: the reference's functions are called directly -- `label_layer` (interpreter/interpreter.py:16-21),
`rotate_array` (:188-192), `FindObjectHeightInRotated._func` (:228-231) and `CropAndRotateSingleParagraph._func`
(:319-347), the last with stand-in queue objects whose `put` computes the height and whose `get` returns it; constructing
the classes would start their worker processes.  The crop to the component's box that precedes `_func` (:303-308) is
restated as in make_golden_crops.py's `reference_crops`; the zero frame is the reference's own `make_divisible_by`.
`_func` does not return its angle: it is replayed from the recorded heights by the rule of :330-336 and then confirmed --
the crops `rotate_array` gives at that angle must be the ones `_func` returned.  Only inputs and outputs are stored.

Contents
  (a) probe/   two pages of component masks: probe/page{j}/labels (uint8 H x W, scipy's numbering); probe/names; per mask
               {n}: /page, /label, /box (y0, x0, height, width), /angles (float64), /extents (int32 per angle: y0, y1,
               x0, x1 of find_objects of the order-0 rotation of the mask cut to its box), /out_shapes.  Page 0: seven
               tilted rectangles (tilts 0, 17, -33, 58, 90, 123.4, 3 degrees); page 1: an L with a block inside its box
               (two components whose boxes overlap), a ring, a 2 x 7 bar, a 3 x 5 block and a 3 x 3 block.  The angles
               of a mask are the 26 of its own search, then 1, 45, 90, 135, 179 and three random ones.
  (b) rot/     for the masks in rot/names: companions rot/{n}/img{c} (1, H, W, c) of the mask's page with c = 1, 2, 4,
               rot/{n}/angles (4), and per angle k the reference's order-1 crops rot/{n}/c{c}/{k}: float64, cut to the
               region of the rotated mask, unpadded (every 5th element, `@stride5`, where a crop is large).
  (c) stage/   one page of 96 x 160 with four paragraphs -- upright (angle None), tilted 58 and 17 degrees, a 3 x 5
               speck: stage/paragraph (1, H, W, 1), stage/img1, stage/img2; per paragraph p in label order
               stage/{p}/trace (13 x 4: a, b, height_a, height_b), stage/{p}/angle (NaN for None), stage/{p}/c{c} the
               crops of both companions padded to multiples of 16.

A mask of one row or one column is not in here, nor a single pixel: scipy keeps a pixel only where 0 <= coordinate <=
n - 1, which for n = 1 is the one float64 value 0 -- such a rotation has no pixel that survives a shift of 1e-9.  A 2 x 2
block is not either: some angles of its search leave no pixel set, and the reference raises there.

Conditions asserted, so that the reference alone decides every stored number (the NumPy restatement below is used for
nothing else):
  * every stored extent and every stored height equals the restatement's with all coordinates shifted by +1e-9 and by
    -1e-9: no source pixel is chosen by a tie at k + 0.5 (the centre of the output plane maps onto the centre of the box,
    which is x.5 when a side is even) and none stands on the border 0 or n - 1
  * for (b) and (c), no sampled coordinate lies within 1e-9 of 0 or of n - 1 on its axis, where the value jumps
One of the fixed or random angles that fails is replaced by the next one that passes in steps of 0.37 degrees (printed);
a search angle cannot be replaced, so a mask with one that fails has to be changed by hand.
Companions are multiples of 1/64 in [0, 1): the same numbers in binary16, float32 and float64.
"""
import os
import sys

import numpy as np
from scipy import ndimage

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (installs the stand-ins, puts the reference on sys.path)
from make_golden_crops import save_reproducible  # noqa: E402

from components.interpreter import interpreter as ref_interp  # noqa: E402
from components.my_model import model as ref_mm  # noqa: E402

SHIFT = 1e-9
FIXED_ANGLES = (1.0, 45.0, 90.0, 135.0, 179.0)
TILTS = (0, 17, -33, 58, 90, 123.4, 3)


# ---- the restatement: used ONLY to test the two conditions ---------------------------------------------------------------
def coordinates(ih, iw, angle, shift=0.0):
    c, s = np.cos(np.deg2rad(angle)), np.sin(np.deg2rad(angle))
    M = np.array([[c, s], [-s, c]])
    out_shape = (np.ptp(M @ [[0, 0, ih, ih], [0, iw, 0, iw]], axis=1) + 0.5).astype(int)
    offset = (np.array([ih, iw]) - 1) / 2 - M @ ((out_shape - 1) / 2)
    oy, ox = np.mgrid[:out_shape[0], :out_shape[1]].astype(np.float64)
    return (offset[0] + oy * M[0, 0]) + ox * M[0, 1] + shift, (offset[1] + oy * M[1, 0]) + ox * M[1, 1] + shift


def restated_extent(mask, angle, shift=0.0):
    """mask (h, w) bool -> (y0, y1, x0, x1) of its order-0 rotation, zeros when empty"""
    ih, iw = mask.shape
    cy, cx = coordinates(ih, iw, angle, shift)
    inside = (cy >= 0) & (cy <= ih - 1) & (cx >= 0) & (cx <= iw - 1)
    sy, sx = np.floor(cy + 0.5).astype(int).clip(0, ih - 1), np.floor(cx + 0.5).astype(int).clip(0, iw - 1)
    ys, xs = np.nonzero(inside & mask[sy, sx])
    return (int(ys.min()), int(ys.max()) + 1, int(xs.min()), int(xs.max()) + 1) if len(ys) else (0, 0, 0, 0)


def clear_of_the_borders(ih, iw, angle, region):
    cy, cx = coordinates(ih, iw, angle)
    ry, rx = region
    cy, cx = cy[ry, rx], cx[ry, rx]
    return all(np.min(np.abs(c - edge)) > SHIFT for c, n in ((cy, ih), (cx, iw)) for edge in (0, n - 1))


# ---- the reference's results -------------------------------------------------------------------------------------------
def as4d(mask):
    return mask[None, :, :, None]


def reference_extent(mask, angle):
    """(y0, y1, x0, x1), (out_h, out_w) of :340-341 on the (h, w) bool mask; the height is also asked of
    FindObjectHeightInRotated._func"""
    rotated = ref_interp.rotate_array(as4d(mask), angle, good_rotation=False)
    _, region_y, region_x, _ = ndimage.find_objects(rotated)[0]
    assert ref_interp.FindObjectHeightInRotated._func(as4d(mask), angle) == region_y.stop - region_y.start
    return (region_y.start, region_y.stop, region_x.start, region_x.stop), rotated.shape[1:3]


def stable(mask, angle):
    """the first condition for one probe"""
    try:
        extent, out_shape = reference_extent(mask, angle)
    except IndexError:                                                  # (no pixel set: the reference raises)
        return False
    cy, _ = coordinates(*mask.shape, angle)
    return cy.shape == tuple(out_shape) and all(restated_extent(mask, angle, shift) == extent for shift in (SHIFT, -SHIFT))


class HeightQueue:
    """stands for an input and an output queue of one height finder: put computes, get returns"""

    def __init__(self):
        self.asked = []

    def put(self, item):
        mask, angle = item
        self.asked.append((angle, ref_interp.FindObjectHeightInRotated._func(mask, angle)))

    def get(self):
        return self.asked[-1][1]


def reference_search(mask, arrays=()):
    """CropAndRotateSingleParagraph._func on the (h, w) mask and its (1, h, w, c) companions -> trace (rounds, 4), angle or
    None, crops"""
    a, b = HeightQueue(), HeightQueue()
    crops = ref_interp.CropAndRotateSingleParagraph._func(True, 1.0, a, a, b, b, as4d(mask), list(arrays))
    trace = np.array([(pa[0], pb[0], pa[1], pb[1]) for pa, pb in zip(a.asked, b.asked)], np.float64)
    low, high = 0.0, 180.0                                              # :330-336 replayed from the recorded heights
    for pa, pb, height_a, height_b in trace:
        if height_a < height_b:
            high = pb
        else:
            low = pa
    angle = (high + low) / 2
    if not 1.0 <= angle <= 179.0:
        angle = None
    for crop, array in zip(crops, arrays):                              # the angle is the one _func used
        if angle is None:
            assert crop is array or np.array_equal(crop, array)
        else:
            (y0, y1, x0, x1), _ = reference_extent(mask, angle)
            assert np.array_equal(crop, ref_interp.rotate_array(array, angle)[:, y0:y1, x0:x1, :])
    return trace, angle, crops


# ---- masks ---------------------------------------------------------------------------------------------------------
def tilted_rectangle(length, thickness, tilt):
    half = int(length) // 2 + 3
    yy, xx = np.mgrid[-half:half + 1, -half:half + 1]
    t = np.deg2rad(tilt)
    u, v = xx * np.cos(t) + yy * np.sin(t), -xx * np.sin(t) + yy * np.cos(t)
    m = (np.abs(u) <= length / 2) & (np.abs(v) <= thickness / 2)
    ys, xs = np.nonzero(m)
    return m[ys.min():ys.max() + 1, xs.min():xs.max() + 1]


def l_shape():
    m = np.zeros((15, 12), bool)
    m[:, :3] = m[12:, :] = True
    return m


def ring():
    yy, xx = np.mgrid[-6:7, -6:7]
    d = np.sqrt(yy ** 2 + xx ** 2)
    return (d <= 6.3) & (d >= 3.5)


class Page:
    def __init__(self, h, w):
        self.on = np.zeros((h, w), bool)
        self.placed = []

    def place(self, name, mask, y, x):
        h, w = mask.shape
        self.on[y:y + h, x:x + w] |= mask
        ys, xs = np.nonzero(mask)
        self.placed.append((name, mask, (y, x, h, w), (y + ys[0], x + xs[0])))

    def components(self):
        """labels (H, W) by the reference's label_layer; per placed mask (name, label, box) -- the component must be the
        mask, nothing joined to it"""
        layers = ref_interp.label_layer(self.on[None, :, :, None].astype(np.float64))
        labels = np.zeros(self.on.shape, np.int32)
        for k, layer in enumerate(layers, 1):
            labels[layer[0, :, :, 0]] = k
        found = []
        for name, mask, (y, x, h, w), pixel in self.placed:
            k = int(labels[pixel])
            assert np.array_equal(labels[y:y + h, x:x + w] == k, mask) and (labels == k).sum() == mask.sum(), name
            found.append((name, k, (y, x, h, w), mask))
        return labels, found


def probe_pages():
    first = Page(148, 148)
    for i, tilt in enumerate(TILTS):
        mask = tilted_rectangle(31 + 2 * (i % 3), 7 + i % 2, tilt)
        assert mask.shape[0] <= 44 and mask.shape[1] <= 44
        first.place(f'tilt{i}', mask, 2 + 48 * (i // 3), 2 + 48 * (i % 3))
    second = Page(40, 64)
    second.place('l', l_shape(), 2, 3)
    block = np.ones((6, 5), bool)
    second.place('in_l', block, 4, 9)                                   # inside the L's box, two pixels clear of it
    second.place('ring', ring(), 3, 22)
    second.place('bar', np.ones((2, 7), bool), 30, 3)
    second.place('block', np.ones((3, 5), bool), 25, 40)
    second.place('dot', np.ones((3, 3), bool), 34, 55)
    return [first, second]


# ---- (a) ---------------------------------------------------------------------------------------------------------------
def next_stable(mask, angle, what):
    tried = angle
    while not stable(mask, tried):
        tried += 0.37
        assert tried < angle + 10, what
    if tried != angle:
        print(f'  {what}: angle {angle} fails a condition, replaced by {tried}')
    return tried


def gen_probes(out):
    r = np.random.default_rng(401)
    names, components_of = [], {}
    for j, page in enumerate(probe_pages()):
        labels, found = page.components()
        assert labels.max() < 256
        out[f'probe/page{j}/labels'] = labels.astype(np.uint8)
        for name, k, box, mask in found:
            trace, angle, _ = reference_search(mask)
            assert len(trace) == 13
            search = [float(v) for row in trace for v in row[:2]]
            for a in search:
                assert stable(mask, a), f'{name}: the search angle {a} fails a condition -- change the mask'
            others = [next_stable(mask, a, name) for a in FIXED_ANGLES + tuple(np.round(r.uniform(0, 180, 3), 3))]
            angles = search + others
            results = [reference_extent(mask, a) for a in angles]
            out[f'probe/{name}/page'], out[f'probe/{name}/label'] = np.array(j), np.array(k)
            out[f'probe/{name}/box'] = np.array(box, np.int32)
            out[f'probe/{name}/angles'] = np.array(angles, np.float64)
            out[f'probe/{name}/extents'] = np.array([e for e, _ in results], np.int32)
            out[f'probe/{name}/out_shapes'] = np.array([s for _, s in results], np.int32)
            names.append(name)
            components_of[name] = (j, k, box, mask)
            print(f'{name:6s} page {j} label {k} box {box}: search ends at {angle}')
    out['probe/names'] = np.array(names)
    return components_of


# ---- (b) ---------------------------------------------------------------------------------------------------------------
def sampled(name, crop, store):
    if crop.size <= 1500:
        store[name] = crop
    else:
        store[name + '@stride5'] = crop.reshape(-1)[::5].copy()


def gen_rotations(out, components_of):
    r = np.random.default_rng(402)
    names = ['l', 'ring', 'tilt6']
    pages = probe_pages()
    for name in names:
        j, k, (y, x, h, w), mask = components_of[name]
        page_shape = pages[j].on.shape
        angles = []
        for a in np.round(r.uniform(1, 179, 4), 2):
            while True:
                a = next_stable(mask, float(a), f'rot/{name}')
                (y0, y1, x0, x1), _ = reference_extent(mask, a)
                if clear_of_the_borders(h, w, a, (slice(y0, y1), slice(x0, x1))):
                    break
                print(f'  rot/{name}: angle {a} samples a border, replaced')
                a += 0.37
            angles.append(a)
        out[f'rot/{name}/angles'] = np.array(angles, np.float64)
        on_page = np.zeros(page_shape, bool)
        on_page[y:y + h, x:x + w] = mask
        for c in (1, 2, 4):
            image = r.integers(0, 64, (1, *page_shape, c)) / 64.0
            out[f'rot/{name}/img{c}'] = image.astype(np.float16)
            cropped = (image * as4d(on_page))[:, y:y + h, x:x + w, :]  # :304-308
            for i, a in enumerate(angles):
                (y0, y1, x0, x1), _ = reference_extent(mask, a)
                sampled(f'rot/{name}/c{c}/{i}', ref_interp.rotate_array(cropped, a)[:, y0:y1, x0:x1, :], out)
    out['rot/names'] = np.array(names)


# ---- (c) ---------------------------------------------------------------------------------------------------------------
def gen_stage(out):
    r = np.random.default_rng(403)
    page = Page(96, 160)
    page.place('upright', np.ones((13, 43), bool), 5, 8)
    page.place('tilt17', tilted_rectangle(45, 9, 17), 30, 6)
    page.place('tilt58', tilted_rectangle(41, 9, 58), 8, 90)
    page.place('speck', np.ones((3, 5), bool), 80, 140)
    paragraph = page.on[None, :, :, None].astype(np.float64)
    arrays = [r.integers(0, 64, (1, 96, 160, c)) / 64.0 for c in (1, 2)]
    out['stage/paragraph'] = paragraph.astype(np.float16)
    out['stage/img1'], out['stage/img2'] = (a.astype(np.float16) for a in arrays)
    components = ref_interp.label_layer(paragraph)
    assert len(components) == 4
    found = []
    for p, component in enumerate(components):
        _, region_y, region_x, _ = ndimage.find_objects(component)[0]  # :303-308
        mask = component[0, region_y, region_x, 0]
        cropped = [(image * component)[:, region_y, region_x, :] for image in arrays]
        trace, angle, crops = reference_search(mask, cropped)
        assert len(trace) == 13
        for a in trace[:, :2].reshape(-1):
            assert stable(mask, float(a)), f'stage paragraph {p}: the search angle {a} fails a condition -- change the mask'
        if angle is not None:
            assert stable(mask, angle), f'stage paragraph {p}: the final angle fails a condition'
            (y0, y1, x0, x1), _ = reference_extent(mask, angle)
            assert clear_of_the_borders(*mask.shape, angle, (slice(y0, y1), slice(x0, x1))), f'stage paragraph {p}'
        out[f'stage/{p}/trace'] = trace
        out[f'stage/{p}/angle'] = np.array(np.nan if angle is None else angle)
        for c, crop in zip((1, 2), crops):
            out[f'stage/{p}/c{c}'] = ref_mm.make_divisible_by(crop, 16, 16)
        found.append(angle)
        print(f'stage paragraph {p}: box {mask.shape}, angle {angle}, crop {crops[0].shape} -> {out[f"stage/{p}/c1"].shape}')
    assert found[0] is None and sum(a is not None for a in found) >= 2, 'the upright paragraph is not rotated, the tilted ones are'


def main():
    out = {}
    components_of = gen_probes(out)
    gen_rotations(out, components_of)
    gen_stage(out)
    save_reproducible('rotation', out)


if __name__ == '__main__':
    main()
