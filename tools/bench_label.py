#!/usr/bin/env python3
"""Device ParagraphCrop stage (uocr_label_components + uocr_masked_crop) against the host route it replaces.

Per mask: event time of label + table and of all crops (a 1-channel and a 2-channel companion, padded to multiples of
16), after warm-up and on rotating buffers; the bytes each has to move at least (label: read x, write labels; crops:
read the boxes of the companions and of the labels, write the padded crops) and the GB/s that makes, next to the d2d
copy rate of profiles/r03_membw.txt.  Host route: D2H of the mask and the companions, ndimage.label / find_objects,
the masked crop and the zero frame in NumPy, H2D of the crops (wall time; "n/a" where scipy does not import).

    python tools/bench_label.py [--reps 20] > profiles/label_microbench.txt
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

COPY_GBS = 5176.0          # profiles/r03_membw.txt: d2d copy (1 read + 1 write)
ROTATE = 4
MAX_COMPONENTS = 4096


def serpentine(h, w):
    m = np.zeros((h, w))
    m[::2] = 1
    for i, y in enumerate(range(1, h, 2)):
        m[y, w - 1 if i % 2 == 0 else 0] = 1
    return m


def cases():
    from univer_ocr_amd.my_model.synthetic import make_page_batch
    rng = np.random.default_rng(0)
    for h, w in ((256, 512), (1024, 2048)):
        page = make_page_batch(1, h, w, seed=1236)
        yield f'1x{h}x{w} paragraph layer', page['paragraph'], page['monochrome'], page['line'], None
    h, w = 1024, 2048
    mono, line = (rng.random((1, h, w, 1)) < 0.1).astype(float), (rng.random((1, h, w, 2)) < 0.1).astype(float)
    # (x > mean(x) is empty for a constant layer: these two use a given threshold)
    yield f'1x{h}x{w} all foreground', np.ones((1, h, w, 1)), mono, line, 0.5
    yield f'1x{h}x{w} serpentine', serpentine(h, w).reshape(1, h, w, 1), mono, line, 0.5


def padded(n):
    return n + 16 - n % 16


def host_route(mask_dev, companions_dev, threshold, CP, rt):
    try:
        from scipy import ndimage
    except ImportError:
        return None
    rt.synchronize()
    start = time.perf_counter()
    mask = mask_dev.numpy()
    companions = [a.numpy() for a in companions_dev]
    labels, count = ndimage.label(mask > (np.mean(mask) if threshold is None else threshold))
    crops = []
    for k, (_, ry, rx, _) in enumerate(ndimage.find_objects(labels), 1):
        for image in companions:
            crop = (image * (labels == k))[:, ry, rx, :]
            _, ch, cw, c = crop.shape
            out = np.zeros((1, padded(ch), padded(cw), c), crop.dtype)
            py, px = (out.shape[1] - ch) // 2, (out.shape[2] - cw) // 2
            out[:, py:py + ch, px:px + cw] = crop
            crops.append(CP.copy(out, np.float32))
    rt.synchronize()
    return (time.perf_counter() - start) * 1e6


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--reps', type=int, default=20)
    args = parser.parse_args()
    from univer_ocr_amd.hip import lib as hiplib
    from univer_ocr_amd.nn import CP
    CP.use_gpu(0)
    rt = CP.runtime()
    ev = [ctypes.c_void_p() for _ in range(2)]
    for e in ev:
        assert rt.lib.uocr_event_create(ctypes.byref(e)) == 0

    def timed(fn, reps):
        for i in range(3):
            fn(i)
        rt.synchronize()
        rt.call('uocr_event_record', ev[0])
        for i in range(reps):
            fn(i)
        rt.call('uocr_event_record', ev[1])
        ms = ctypes.c_float()
        assert rt.lib.uocr_event_elapsed_ms_sync(ev[0], ev[1], ctypes.byref(ms)) == 0
        return ms.value * 1e3 / reps

    print(f'{"mask":34s} {"comps":>5s} {"launches":>8s} | {"label+table":>11s} {"MB":>7s} {"GB/s":>6s} {"of copy":>7s} | '
          f'{"crops":>9s} {"MB":>7s} {"GB/s":>6s} | {"device":>9s} {"host route":>11s}')
    for name, mask, mono, line, threshold in cases():
        _, h, w, _ = mask.shape
        xs = [CP.copy(mask, np.float32) for _ in range(ROTATE)]
        monos = [CP.copy(mono, np.float32) for _ in range(ROTATE)]
        lines = [CP.copy(line, np.float32) for _ in range(ROTATE)]
        labels = [CP.empty((1, h, w), np.int32) for _ in range(ROTATE)]
        tables = [CP.empty((1, MAX_COMPONENTS, 8), np.int64) for _ in range(ROTATE)]
        counts = [CP.zeros((1,), np.int32) for _ in range(ROTATE)]

        mode = hiplib.THRESH_MEAN if threshold is None else hiplib.THRESH_VALUE

        def label(i):
            j = i % ROTATE
            rt.call('uocr_label_components', hiplib.F32, xs[j].ptr, 1, h, w, mode, float(threshold or 0.0), labels[j].ptr,
                    tables[j].ptr, MAX_COMPONENTS, counts[j].ptr)
        label_us = timed(label, args.reps)
        launches = rt.last_label()[2]
        count = int(counts[0].numpy()[0])
        boxes = tables[0].numpy()[0, :count, 2:6]
        outs, crop_bytes = [], 0
        for y0, y1, x0, x1 in boxes:
            ch, cw = int(y1 - y0), int(x1 - x0)
            per_rot = [[CP.empty((1, padded(ch), padded(cw), c), np.float32) for c in (1, 2)] for _ in range(ROTATE)]
            outs.append(per_rot)
            crop_bytes += ch * cw * 4 * (3 + 2) + padded(ch) * padded(cw) * 4 * 3   # companions + labels twice; crops

        def crops(i):
            j = i % ROTATE
            for k, (y0, y1, x0, x1) in enumerate(boxes, 1):
                for slot, src in enumerate((monos[j], lines[j])):
                    out = outs[k - 1][j][slot]
                    rt.call('uocr_masked_crop', hiplib.F32, src.ptr, labels[j].ptr, 1, h, w, src.shape[3], 0, k, int(y0),
                            int(x0), int(y1 - y0), int(x1 - x0), out.ptr, out.shape[1], out.shape[2])
        crops_us = timed(crops, args.reps)
        host_us = host_route(xs[0], [monos[0], lines[0]], threshold, CP, rt)
        label_bytes = h * w * 8
        label_gbs = label_bytes / label_us / 1e3
        print(f'{name:34s} {count:5d} {launches:8d} | {label_us:8.1f} us {label_bytes / 1e6:7.2f} {label_gbs:6.0f} '
              f'{100 * label_gbs / COPY_GBS:6.1f}% | {crops_us:6.1f} us {crop_bytes / 1e6:7.2f} '
              f'{crop_bytes / crops_us / 1e3:6.0f} | {label_us + crops_us:6.1f} us '
              + (f'{host_us:8.0f} us' if host_us is not None else f'{"n/a":>11s}'))


if __name__ == '__main__':
    main()
