#!/usr/bin/env python3
"""The line finding of the LineCrop stage per page: all masks of the page in ONE uocr_label_batch call with one readback
(my_model/crop.py: CropLines(labelling='page')) against one split, two uocr_label_components calls and four readbacks per
paragraph (labelling='paragraph', the default).

Two pages: (a) the four stage paragraphs of tests/golden/line_crop.npz (36-52 x 44-52 pixels, two or three lines each)
and (b) eight paragraphs of 160 x 160 pixels with six lines each; masks are multiples of 1/64.  Per page the span from
the masks on the device to `found` on the host (CropLines.find_lines: rotation and line boxes of every paragraph): both
forms end in a readback, so the wall clock ends in a synchronised device; the event time is taken on the stream around
the same span.  The two forms ALTERNATE: a run is --reps repetitions of one form, --runs runs of each, 'paragraph' and
'page' in turn; printed are the median run and the fastest and slowest, per repetition.  Both forms must find the same
lines.  Both forms end in the same host work on the component tables (arrange_lines, line_boxes: NumPy on a few rows per
paragraph); it is timed on its own, on tables read back before, so that what the labelling costs can be told from it.

    python tools/bench_line_labels.py [--reps 30] [--runs 7] > profiles/line_labels_microbench.txt
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

STAGE_NAMES = ('upright', 'shared', 'turned', 'stray')


def lined_paragraph(rng, size=160, lines=6):
    """(1, size, size, 2): `lines` upright lines, a soft top band in channel 0 and a bottom band in channel 1, on noise
    below the threshold; multiples of 1/64"""
    mask = rng.integers(0, 9, (1, size, size, 2)).astype(np.float64)
    pitch = (size - 10) // lines
    for i in range(lines):
        y, left, right = 6 + pitch * i, 8 + int(rng.integers(0, 8)), size - 8 - int(rng.integers(0, 8))
        for channel, first in ((0, y), (1, y + pitch - 10)):
            mask[0, first:first + 4, left:right, channel] = 48
            mask[0, first + 1:first + 3, left + 1:right - 1, channel] = 64
    return mask / 64


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--reps', type=int, default=30)
    parser.add_argument('--runs', type=int, default=7)
    args = parser.parse_args()
    from univer_ocr_amd.my_model.crop import CropLines
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

    golden = np.load(os.path.join(ROOT, 'tests', 'golden', 'line_crop.npz'))
    rng = np.random.default_rng(160)
    pages = (('fixture, 4 paragraphs of 36-52 x 44-52', [np.asarray(golden[f'stage/{name}/mask'], np.float64) for name in STAGE_NAMES]),
             ('8 paragraphs of 160 x 160, 6 lines each', [lined_paragraph(rng) for _ in range(8)]))
    stages = {form: CropLines(labelling=form) for form in ('paragraph', 'page')}
    print(f'line finding per page, one labelling call per page against two per paragraph, on {rt.device_info()["name"]}: '
          f'{args.runs} alternating runs of {args.reps} repetitions each, us per repetition as median (fastest .. slowest) '
          f'of the runs')
    for name, host_masks in pages:
        assert all(np.array_equal(m * 64, np.round(m * 64)) for m in host_masks), 'multiples of 1/64'
        masks = [CP.copy(m, 'float32') for m in host_masks]
        found, calls = {}, {}
        forms = [(form, (lambda form=form: found.__setitem__(form, stages[form].find_lines(masks)))) for form in stages]
        for form, fn in forms:                                          # warm-up, and the C calls of one page
            for _ in range(3):
                before = rt.launches
                fn()
                calls[form] = rt.launches - before
        assert found['paragraph'] == found['page'], (found['paragraph'], found['page'])
        times = {form: [] for form, _ in forms}
        for _ in range(args.runs):
            for form, fn in forms:
                times[form].append(run(fn))
        _, _, per_group, launches = rt.last_label_batch()
        one = rt.last_label()[2]
        print(f'{name}: lines per paragraph {[len(boxes) for _, boxes in found["page"]]} (equal in both forms)')
        for form, _ in forms:
            event, wall = ([t[i] for t in times[form]] for i in (0, 1))
            what = (f'{calls[form]:3d} C calls, {len(masks)} splits + {2 * len(masks)} x {one} kernels, {4 * len(masks)} readbacks of '
                    f'{2 * len(masks) * (4096 * 64 + 4) / 1024:.0f} KiB' if form == 'paragraph' else
                    f'{calls[form]:3d} C calls, {launches} kernels for {2 * len(masks)} entries ({per_group} per group), 1 readback of '
                    f'{2 * len(masks) * (256 * 64 + 4) / 1024:.0f} KiB')
            print(f'  {form:9s} {what} | events {statistics.median(event):8.1f} ({min(event):.1f} .. {max(event):.1f}) us | '
                  f'wall clock {statistics.median(wall):8.1f} ({min(wall):.1f} .. {max(wall):.1f}) us')
        by_wall = {form: statistics.median(t[1] for t in times[form]) for form, _ in forms}
        print(f'  paragraph / page by the wall clock: {by_wall["paragraph"] / by_wall["page"]:.2f}')
        # the host work both forms end in, on tables that are on the host already
        tables = ops.label_batch([(mask, channel) for mask in masks for channel in (0, 1)], 'mean_max')
        label_batch, ops.label_batch = ops.label_batch, lambda entries, threshold, max_components: tables
        try:
            assert stages['page'].find_lines(masks) == found['page']
            host = []
            for _ in range(args.runs):
                start = time.perf_counter()
                for _ in range(args.reps):
                    stages['page'].find_lines(masks)
                host.append((time.perf_counter() - start) * 1e6 / args.reps)
        finally:
            ops.label_batch = label_batch
        host = statistics.median(host)
        print(f'  of which arrange_lines and line_boxes on the host, in both forms: {host:.1f} us; labelling and readback: '
              f'paragraph {by_wall["paragraph"] - host:.1f} us, page {by_wall["page"] - host:.1f} us, '
              f'ratio {(by_wall["paragraph"] - host) / (by_wall["page"] - host):.2f}')


if __name__ == '__main__':
    main()
