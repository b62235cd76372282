#!/usr/bin/env python3
"""Generate tests/golden/paragraph_crop.npz: inputs and expected outputs of the ParagraphCrop stage and of the
TRAIN_LINE model system, taken from the REFERENCE (needs the reference checkout and scipy; see make_golden.py, whose
import stand-ins this script reuses by importing it).

    python tests/golden/make_golden_crops.py

Route taken: the reference's `interpreter` module imports with make_golden.py's stand-ins, so the labels of the 'mean'
rule come from its own `label_layer` (interpreter.py:16-21).  The other two threshold rules have no function of their own
in the reference (they are expressions inside methods, :437-438 and :549), so they are restated here as
`ndimage.label(x > t)` with the reference's arguments (default structure).  Boxes are `ndimage.find_objects`
(:303) and centres `ndimage.center_of_mass` (:36-39) of each component's boolean mask.  The crop restates :303-308:
the companion array times the component's mask, cut to the component's box; the zero frame is the reference's own
`make_divisible_by` (my_model/model.py:26-34).  Only inputs and outputs are stored.

Contents
  (a) ops     m{i}/x, and per threshold rule r in mean / mean_max / value: m{i}/{r}/labels (int32 H x W), /table (int64
              count x 8: first pixel, area, y0, y1, x0, x1, sum y, sum x), /centers (float64 count x 2); m{i}/value_t;
              crops of a 1-, 2- and 4-channel companion for every component ('mean' rule) of the masks in `crop_masks`:
              m{i}/img{c}, m{i}/crop{c}/{k} (unpadded).  Companions are non-negative, as every layer of the data path is
              (image * mask gives -0.0 for negative pixels outside the mask, the device writes +0.0).
  (b) system  the layers of make_page_batch(1, 128, 192, seed=1236), its two paragraphs' crops padded to multiples of
              16, and the reference's Line net trained for two steps (SGD and Adam) over [crop_0, crop_1] through the
              reference's LineSelector (one system.train call = one step per paragraph): accumulated losses,
              per-paragraph predictions (the larger one as every 5th element, `@stride5`), final weights, in the key
              format of model_system_lists.npz under the prefixes sgd/ and adam/.

Every input keeps a distance of more than 1e-3 from each of its thresholds (asserted), so that a float32 or binary16
mean cannot flip a pixel: the reference alone decides every pixel.
"""
import os
import sys

import numpy as np
from scipy import ndimage

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (installs the stand-ins, puts the reference on sys.path)

from components.interpreter import interpreter as ref_interp  # noqa: E402
from components.my_model import model as ref_mm  # noqa: E402
from components.nn import optimizers as ref_opt  # noqa: E402
from components.nn.model_system import ModelComponent, ModelSystem  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(mg.OUT_DIR)))
MARGIN = 1e-3
RULES = ('mean', 'mean_max', 'value')


# ---- masks ---------------------------------------------------------------------------------------------------------
def blobs(h, w, seed, count=9):
    r = np.random.default_rng(seed)
    yy, xx = np.mgrid[:h, :w]
    m = np.zeros((h, w))
    for _ in range(count):
        cy, cx, ry, rx = r.integers(0, h), r.integers(0, w), r.integers(2, h // 4), r.integers(3, w // 5)
        m[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1] = 1
    return m


def u_shapes(h, w):
    """U's whose prongs begin at different rows and only join at the bottom; a nested pair; an upside-down U"""
    m = np.zeros((h, w))
    m[3:40, 4:7] = m[9:40, 16:19] = m[37:40, 4:19] = 1             # right prong starts later
    m[12:30, 30:32] = m[5:30, 44:46] = m[28:30, 30:46] = 1          # left prong starts later
    m[15:25, 35:37] = m[17:25, 40:42] = m[23:25, 35:42] = 1         # a U inside the second one, not touching it
    m[4:7, 55:85] = m[4:45, 55:58] = m[4:33, 82:85] = 1             # upside down
    m[20:48, 66:72] = 1                                             # a bar inside it
    m[44:47, 2:30] = 1
    return m


def comb(h, w):
    m = np.zeros((h, w))
    m[h - 6:h - 3, 3:w - 3] = 1
    for i, x in enumerate(range(4, w - 4, 7)):
        m[3 + (i * 5) % 17:h - 3, x:x + 2] = 1
    m[2:4, 10:w - 30:3] = 1
    return m


def diagonal_contacts(h, w):
    """pixels and 2x2 blocks that touch only at corners: each stays its own component"""
    m = np.zeros((h, w))
    for i in range(min(h, w) - 2):
        m[i, i] = 1
    for i in range(0, h - 3, 2):
        m[i:i + 2, w - 4 - i:w - 2 - i] = 1 if i % 4 == 0 else m[i:i + 2, w - 4 - i:w - 2 - i]
    yy, xx = np.mgrid[:h, :w]
    m[(yy >= h // 2) & (xx < w // 3) & ((yy + xx) % 2 == 0)] = 1    # a checkerboard patch
    return m


def rings(h, w):
    yy, xx = np.mgrid[:h, :w]
    d = np.maximum(np.abs(yy - h // 2) * (w / h), np.abs(xx - w // 2))
    m = ((d.astype(int) // 5) % 2 == 0).astype(float)
    m[h // 2, w // 2:w // 2 + 23] = 1                                # a bridge joins the inner rings
    return m


def spiral(h, w):
    m = np.zeros((h, w))
    top, left, bottom, right = 1, 1, h - 2, w - 2
    y, x = top, left
    while bottom - top > 3 and right - left > 3:
        m[top, left:right + 1] = 1
        m[top:bottom + 1, right] = 1
        m[bottom, left + 2:right + 1] = 1
        m[top + 2:bottom + 1, left + 2] = 1
        m[top + 2, left + 2:left + 4] = 1
        top, left, bottom, right = top + 2, left + 2, bottom - 2, right - 2
    return m


def noise(h, w, seed, density):
    return (np.random.default_rng(seed).random((h, w)) < density).astype(float)


def lines_and_dots(h, w):
    m = np.zeros((h, w))
    m[0, :] = m[h - 1, :] = 1
    m[3:h - 3, 0] = m[2:h - 2, w - 1] = 1
    m[5, 5] = m[7, 7] = m[h // 2, 3:w - 3] = 1
    m[h // 2 - 6:h // 2 + 7, w // 2] = 1
    return m


def soft(h, w, seed, count):
    """sigmoid-like prediction: blurred blobs of different strength plus noise, values in (0, 1)"""
    r = np.random.default_rng(seed)
    base = blobs(h, w, seed, count) * r.uniform(0.55, 1.0, (h, w))
    z = ndimage.gaussian_filter(base, 1.5) * 9.0 - 3.0 + r.normal(0, 0.4, (h, w))
    return np.round(4096.0 / (1.0 + np.exp(-z))) / 4096.0         # (dyadic values: the archive compresses)


def thresholds(x, value_t):
    mean, mx = np.mean(x), np.max(x)
    return {'mean': mean, 'mean_max': 0.5 * (mean + mx), 'value': value_t}


def keep_clear_of_thresholds(x, value_t):
    """move the few values that lie within 2 * MARGIN of a threshold away from it until none does"""
    x = x.copy()
    for _ in range(100):
        moved = False
        for t in thresholds(x, value_t).values():
            near = np.abs(x - t) <= 2 * MARGIN
            if near.any():
                x[near] = np.where(x[near] > t, t + 5 * MARGIN, t - 5 * MARGIN)
                moved = True
        if not moved:
            break
    for rule, t in thresholds(x, value_t).items():
        assert np.min(np.abs(x - t)) > MARGIN, f'{rule}: a value lies within {MARGIN} of the threshold {t}'
    return x


# ---- the reference's results ---------------------------------------------------------------------------------------
def reference_labels(x, rule, t):
    """int32 (H, W) labels of x (1, H, W, 1)"""
    if rule == 'mean':
        masks = ref_interp.label_layer(x)                          # interpreter.py:16-21
        labels = np.zeros(x.shape, np.int32)
        for k, mask in enumerate(masks, 1):
            labels[mask] = k
    else:
        labels, _ = ndimage.label(x > t)                           # :437-438 / :549 (t = (mean + max) / 2), or a given t
    return labels.astype(np.int32)[0, :, :, 0]


def component_table(labels):
    count = int(labels.max())
    h, w = labels.shape
    table = np.zeros((count, 8), np.int64)
    centers = np.zeros((count, 2))
    for k in range(1, count + 1):
        mask = labels == k
        sy, sx = ndimage.find_objects(mask)[0]                     # :303
        ys, xs = np.nonzero(mask)
        table[k - 1] = [ys[0] * w + xs[0], mask.sum(), sy.start, sy.stop, sx.start, sx.stop, ys.sum(), xs.sum()]
        centers[k - 1] = ndimage.center_of_mass(mask)              # :36-39
    return table, centers


def reference_crops(mask, arrays):
    """result[array_id][paragraph_id] of CropAndRotateParagraphs with find_rotation=False (:362-378, :303-308, :345-347)"""
    result = [[] for _ in arrays]
    for component in ref_interp.label_layer(mask):
        _, region_y, region_x, _ = ndimage.find_objects(component)[0]
        for i, image in enumerate(arrays):
            result[i].append((image * component)[:, region_y, region_x, :])
    return result


def gen_ops(out):
    masks = [
        ('blobs', blobs(40, 70, 1), 0.5),
        ('u_shapes', u_shapes(50, 90), 0.5),
        ('comb', comb(45, 100), 0.5),
        ('diagonal', diagonal_contacts(40, 70), 0.5),
        ('rings', rings(64, 128), 0.5),
        ('spiral', spiral(55, 75), 0.5),
        ('noise', noise(60, 110, 2, 0.5), 0.5),
        ('lines_dots', lines_and_dots(41, 71), 0.5),
        ('soft_a', soft(70, 150, 3, 12), 0.62),
        ('soft_b', soft(48, 97, 4, 7), 0.3),
    ]
    crop_masks = ['u_shapes', 'soft_a']
    r = np.random.default_rng(77)
    for name, m, value_t in masks:
        x = keep_clear_of_thresholds(m, value_t)[None, :, :, None]
        out[f'{name}/x'] = x
        out[f'{name}/value_t'] = np.array(value_t)
        for rule, t in thresholds(x, value_t).items():
            labels = reference_labels(x, rule, t)
            table, centers = component_table(labels)
            out[f'{name}/{rule}/labels'], out[f'{name}/{rule}/table'], out[f'{name}/{rule}/centers'] = labels, table, centers
            print(f'{name:10s} {x.shape[1]:3d} x {x.shape[2]:3d} {rule:8s} t = {t:.4f}: {len(table)} components')
        if name in crop_masks:
            # multiples of 1 / 64 in [0, 1): exact in binary16 too, so a crop must come back bit for bit in every dtype
            images = [r.integers(0, 64, (1, *x.shape[1:3], c)) / 64.0 for c in (1, 2, 4)]
            crops = reference_crops(x, images)
            for image, per_component in zip(images, crops):
                c = image.shape[3]
                out[f'{name}/img{c}'] = image
                assert len(per_component) == len(out[f'{name}/mean/table'])
                for k, crop in enumerate(per_component, 1):
                    out[f'{name}/crop{c}/{k}'] = crop
    out['mask_names'] = np.array([name for name, _, _ in masks])
    out['crop_masks'] = np.array(crop_masks)


def sample_prediction(name, pred, store):
    """whole prediction when small, every 5th element otherwise (the archive has to stay small)"""
    if pred.size <= 10000:
        store[name] = pred
    else:
        store[name + '@stride5'] = pred.reshape(-1)[::5].copy()


def gen_system(out):
    from univer_ocr_amd.my_model.synthetic import make_page_batch
    page = make_page_batch(1, 128, 192, seed=1236)
    for tag in ('monochrome', 'paragraph', 'line'):
        out[f'page/{tag}'] = page[tag]
    t = np.mean(page['paragraph'])
    assert np.min(np.abs(page['paragraph'] - t)) > MARGIN
    crops = reference_crops(page['paragraph'], [page['monochrome'], page['line']])
    assert [c.shape[1:3] for c in crops[0]] == [(68, 178), (28, 126)], [c.shape for c in crops[0]]
    padded = [[ref_mm.make_divisible_by(c, 16, 16) for c in per_array] for per_array in crops]   # model.py:552-556, :572-573
    assert [c.shape[1:3] for c in padded[0]] == [(80, 192), (32, 128)]
    for p in range(2):
        out[f'cropped_monochrome{p}'], out[f'cropped_line{p}'] = padded[0][p], padded[1][p]
    for tag, make_opt in (('sgd', lambda: ref_opt.Momentum(lr=0.01, momentum=0)), ('adam', lambda: ref_opt.Adam(lr=0.0015))):
        np.random.seed(11)
        line = ref_mm.make_line(padded[0][0].shape, make_opt())
        mg.set_analytic_weights(line)
        system = ModelSystem([ModelComponent(
            'Line', line, ref_mm.LineSelector('cropped_monochrome', 'cropped_line', 'line_pred'), delist_result=True)])
        context = {'cropped_monochrome': list(padded[0]), 'cropped_line': list(padded[1])}
        system.train(context)                                      # two steps: one per paragraph
        entry = context['losses']['Line']
        assert len(entry['output_losses']) == 2 and len(context['line_pred']) == 2
        out[f'{tag}/train/Line/output_losses'] = np.array(entry['output_losses'])
        out[f'{tag}/train/Line/regularization_loss'] = np.array(entry['regularization_loss'])
        for p, pred in enumerate(context['line_pred']):
            sample_prediction(f'{tag}/train/line_pred{p}', pred, out)
        for pname, param in line.params().items():
            mg.sample_param(f'{tag}/final/{pname}', param.value, out)


def save_reproducible(name, arrays):
    """an .npz like np.savez_compressed writes, but with fixed member timestamps: the same bytes on every run"""
    import io
    import zipfile
    path = os.path.join(mg.OUT_DIR, name + '.npz')
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as archive:
        for key, value in arrays.items():
            member = zipfile.ZipInfo(key + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            member.compress_type = zipfile.ZIP_DEFLATED
            member.external_attr = 0o644 << 16
            buffer = io.BytesIO()
            np.lib.format.write_array(buffer, np.asanyarray(value), allow_pickle=False)
            archive.writestr(member, buffer.getvalue())
    print(f'{name}.npz: {len(arrays)} arrays, {os.path.getsize(path) / 1024:.1f} KiB')


def main():
    out = {}
    gen_ops(out)
    gen_system(out)
    save_reproducible('paragraph_crop', out)


if __name__ == '__main__':
    main()
