#!/usr/bin/env python3
"""The angle search of the ParagraphCrop stage per page: the device search (ONE uocr_rotation_search call, one readback,
the host replay of the leaves) against the host search (13 uocr_rotated_extent calls, a readback and host arithmetic
after each), my_model/crop.py: CropAndRotateParagraphs(search='device' / 'host').

The two pages of tools/bench_rotation.py: the page of tests/golden/rotation.npz (96 x 160, four paragraphs) and a
256 x 512 page with eight tilted paragraphs of 105 x 29 pixels.  Per page, after the labelling, the span from the
component table to the angles: both forms end in a readback, so the wall clock ends in a synchronised device; the event
time is taken on the stream around the same span.  The two forms ALTERNATE: a run is --reps repetitions of one form,
--runs runs of each, host and device in turn; printed are the median run and the fastest and slowest, per repetition.
Both forms must give the same angles.

    python tools/bench_rotation_search.py [--reps 30] [--runs 7] > profiles/rotation_search_microbench.txt
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_rotation import tilted_page  # noqa: E402


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--reps', type=int, default=30)
    parser.add_argument('--runs', type=int, default=7)
    args = parser.parse_args()
    from univer_ocr_amd.my_model.crop import CropAndRotateParagraphs
    from univer_ocr_amd.nn import CP, ops
    CP.use_gpu(0)
    rt = CP.runtime()
    ev = [ctypes.c_void_p() for _ in range(2)]
    for e in ev:
        assert rt.lib.uocr_event_create(ctypes.byref(e)) == 0

    def run(fn):
        """(event us, wall us) per repetition of one run"""
        rt.synchronize()
        start = time.perf_counter()
        rt.call('uocr_event_record', ev[0])
        for _ in range(args.reps):
            fn()
        rt.call('uocr_event_record', ev[1])
        ms = ctypes.c_float()
        assert rt.lib.uocr_event_elapsed_ms_sync(ev[0], ev[1], ctypes.byref(ms)) == 0
        return ms.value * 1e3 / args.reps, (time.perf_counter() - start) * 1e6 / args.reps

    golden = np.load(os.path.join(ROOT, 'tests', 'golden', 'rotation.npz'))
    pages = (('fixture 96 x 160', np.asarray(golden['stage/paragraph'], np.float64)), ('tilted 256 x 512', tilted_page()))
    stage = CropAndRotateParagraphs()
    print(f'angle search per page, device against host, on {rt.device_info()["name"]}: {args.runs} alternating runs of '
          f'{args.reps} repetitions each, us per repetition as median (fastest .. slowest) of the runs')
    for name, page in pages:
        components = ops.label_components(CP.copy(page, 'float32'), 'mean')
        paragraphs = int(components.count[0])
        found = {}

        def host():
            found['host'] = stage.find_angles(components, paragraphs)

        def device():
            found['device'] = ops.rotation_search(components, 0, range(1, paragraphs + 1), stage.eps)[0]
        forms = (('host', host), ('device', device))
        calls = {}
        for form, fn in forms:                                          # warm-up, and the C calls of one search
            for _ in range(3):
                before = rt.launches
                fn()
                calls[form] = rt.launches - before
        assert found['host'] == found['device'], (found['host'], found['device'])
        times = {form: [] for form, _ in forms}
        for _ in range(args.runs):
            for form, fn in forms:
                times[form].append(run(fn))
        shown = ', '.join('None' if a is None else f'{a:.2f}' for a in found['device'])
        rounds, per_launch, launches = rt.last_rotation_search()
        print(f'{name}: {paragraphs} paragraphs, angles {shown} (equal in both forms)')
        for form, _ in forms:
            event, wall = ([t[i] for t in times[form]] for i in (0, 1))
            what = (f'{calls[form]:2d} C calls, {rounds} rounds read back one by one' if form == 'host' else
                    f'{calls[form]:2d} C call,  {launches} kernels in stream order, one readback')
            print(f'  {form:6s} {what} | events {statistics.median(event):8.1f} ({min(event):.1f} .. {max(event):.1f}) us | '
                  f'wall clock {statistics.median(wall):8.1f} ({min(wall):.1f} .. {max(wall):.1f}) us')
        ratio = statistics.median(t[1] for t in times['host']) / statistics.median(t[1] for t in times['device'])
        print(f'  host / device by the wall clock: {ratio:.2f}')


if __name__ == '__main__':
    main()
