#!/usr/bin/env python3
"""Device rotation search and rotated crops of the ParagraphCrop stage (uocr_rotated_extent, uocr_rotate_crop) per page.

Two pages: the page of tests/golden/rotation.npz (96 x 160, four paragraphs, two of them rotated) and a 256 x 512 page
with eight tilted paragraphs of 105 x 29 pixels.  Per page, after the labelling:
  search  the 14 uocr_rotated_extent calls of CropAndRotateParagraphs -- 13 rounds that hold both probes of every
          paragraph, one call for the regions at the final angles -- INCLUDING the host read of 16 bytes per probe after
          each call and the host arithmetic between them: event time from before the first call to after the last, and
          the wall-clock time of the same span (the two differ by what the host does before its first and after its
          last call)
  crop    the ONE uocr_rotate_crop call for a 1-channel and a 2-channel companion of every rotated paragraph, framed to
          multiples of 16, outputs allocated by the call's wrapper: event time per call, per dtype
Event times after warm-up, mean over --reps repetitions.

    python tools/bench_rotation.py [--reps 30] > profiles/rotation_microbench.txt
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)

TILTS = (8, -15, 27, 41, -52, 63, 76, -5)


def tilted_page(h=256, w=512):
    yy, xx = np.mgrid[:h, :w]
    page = np.zeros((h, w))
    for i, tilt in enumerate(TILTS):
        cy, cx, t = 64 + 128 * (i // 4), 64 + 128 * (i % 4), np.deg2rad(tilt)
        u, v = (xx - cx) * np.cos(t) + (yy - cy) * np.sin(t), -(xx - cx) * np.sin(t) + (yy - cy) * np.cos(t)
        page[(np.abs(u) <= 52) & (np.abs(v) <= 14)] = 1
    return page[None, :, :, None]


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--reps', type=int, default=30)
    args = parser.parse_args()
    from univer_ocr_amd.my_model.crop import CropAndRotateParagraphs
    from univer_ocr_amd.nn import CP, ops
    CP.use_gpu(0)
    rt = CP.runtime()
    ev = [ctypes.c_void_p() for _ in range(2)]
    for e in ev:
        assert rt.lib.uocr_event_create(ctypes.byref(e)) == 0

    def timed(fn, reps):
        """(event us, wall us) per repetition"""
        for _ in range(3):
            fn()
        rt.synchronize()
        start = time.perf_counter()
        rt.call('uocr_event_record', ev[0])
        for _ in range(reps):
            fn()
        rt.call('uocr_event_record', ev[1])
        ms = ctypes.c_float()
        assert rt.lib.uocr_event_elapsed_ms_sync(ev[0], ev[1], ctypes.byref(ms)) == 0
        return ms.value * 1e3 / reps, (time.perf_counter() - start) * 1e6 / reps

    golden = np.load(os.path.join(ROOT, 'tests', 'golden', 'rotation.npz'))
    pages = (('fixture 96 x 160', np.asarray(golden['stage/paragraph'], np.float64)), ('tilted 256 x 512', tilted_page()))
    rng = np.random.default_rng(0)
    stage = CropAndRotateParagraphs()
    print(f'rotation search and rotated crops per page on {rt.device_info()["name"]}, {args.reps} repetitions')
    for name, page in pages:
        mask = CP.copy(page, 'float32')
        components = ops.label_components(mask, 'mean')
        paragraphs = int(components.count[0])
        found = {}

        def search():
            angles = stage.find_angles(components, paragraphs)
            rotated = [p for p in range(paragraphs) if angles[p] is not None]
            found['angles'], found['rotated'] = angles, rotated
            found['regions'] = ops.rotated_extent(components, 0, [(p + 1, angles[p]) for p in rotated])
        before = rt.launches
        search()
        calls = rt.launches - before
        event_us, wall_us = timed(search, args.reps)
        shown = ', '.join('None' if a is None else f'{a:.2f}' for a in found['angles'])
        print(f'{name}: {paragraphs} paragraphs, angles {shown}')
        print(f'  search  {calls:3d} extent calls, {2 * paragraphs} probes per round | {event_us:8.1f} us by events, {wall_us:8.1f} us wall clock')
        for dtype in ('float32', 'float64', 'float16'):
            arrays = [CP.copy(rng.integers(0, 64, (1, *page.shape[1:3], c)) / 64.0, dtype) for c in (1, 2)]
            entries = [(a, components, 0, p + 1, found['angles'][p], tuple(int(v) for v in region))
                       for a in arrays for p, region in zip(found['rotated'], found['regions'])]
            keep = []

            def crop():
                keep[:] = ops.rotate_crop(entries, (16, 16))
            event_us, wall_us = timed(crop, args.reps)
            pixels = sum(out.shape[1] * out.shape[2] for out in keep)
            print(f'  crop    {dtype:8s} {len(entries):3d} entries, {rt.last_rotate()[3]} launch, {pixels} output pixels | '
                  f'{event_us:8.1f} us by events, {wall_us:8.1f} us wall clock')
    print('reference: CropAndRotateSingleParagraph (interpreter/interpreter.py:234-347) runs 27 ndimage.rotate calls per paragraph on '
          'a pool of worker processes, between a device-to-host and a host-to-device copy of every array; it was not timed by this run')


if __name__ == '__main__':
    main()
