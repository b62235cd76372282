#!/usr/bin/env python3
"""Device LineCrop gather (uocr_line_crop) on one page's worth of lines: 32 lines cut out of a 1-channel and a 9-channel
companion (64 entries), upright and quarter-turned, per dtype.

A line is a 16 x 128 box of a 160 x 160 paragraph (zoom factor 2: a 32 x 256 output), upright or -- the same box turned,
128 x 16 read at 90 degrees -- quarter-turned, so both orientations write the same bytes and differ in the read side only:
consecutive outputs of an upright line read ascending addresses of a source row, those of a turned line walk down a
source column.  One call crops all 64 entries.  Event time per call after warm-up, on rotating buffers, for calls issued
one after the other from the host and for one call (on the first buffer set) captured into a HIP graph and replayed; the
launches of a call; the bytes it has to move at least (every box element read once, every output element written once)
and the time the d2d copy rate of profiles/r03_membw.txt would need for them (the HBM floor).  The last line is the
turned / upright ratio that decides whether an LDS transpose for turned lines would be worth building.

    python tools/bench_line_crop.py [--reps 50] > profiles/line_crop_microbench.txt
"""
import argparse
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

COPY_GBS = 5176.0          # profiles/r03_membw.txt: d2d copy (1 read + 1 write)
ROTATE = 4
LINES, PAGE, BOX_H, BOX_W, CHANNELS = 32, 160, 16, 128, (1, 9)
ZOOMED_HEIGHT, MINIMAL_WIDTH = 32, 8


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--reps', type=int, default=50)
    args = parser.parse_args()
    import torch
    from univer_ocr_amd.hip import lib as hiplib
    from univer_ocr_amd.nn import CP
    from univer_ocr_amd.nn.ops import line_crop_shape
    CP.use_gpu(0)
    rt = CP.runtime()
    ev = [ctypes.c_void_p() for _ in range(2)]
    for e in ev:
        assert rt.lib.uocr_event_create(ctypes.byref(e)) == 0

    def timed(fn, reps):
        for i in range(5):
            fn(i)
        rt.synchronize()
        rt.call('uocr_event_record', ev[0])
        for i in range(reps):
            fn(i)
        rt.call('uocr_event_record', ev[1])
        ms = ctypes.c_float()
        assert rt.lib.uocr_event_elapsed_ms_sync(ev[0], ev[1], ctypes.byref(ms)) == 0
        return ms.value * 1e3 / reps

    n = LINES * len(CHANNELS)
    ints = lambda values: (ctypes.c_int * n)(*values)
    print(f'uocr_line_crop, {LINES} lines of {BOX_H} x {BOX_W} out of a {PAGE} x {PAGE} paragraph with {" and ".join(map(str, CHANNELS))} '
          f'channels ({n} entries) in one call, zoomed to {ZOOMED_HEIGHT} rows, on {rt.device_info()["name"]}')
    print(f'{"dtype":8s} {"lines":8s} {"launches":>8s} | {"call":>9s} {"graph replay":>12s} | {"MB moved":>8s} {"HBM floor":>9s} {"call / floor":>12s}')
    results, graphs = {}, []        # (the graphs live to the end: a pool must not be released while the next capture runs)
    rng = np.random.default_rng(0)
    for dtype in ('float32', 'float64', 'float16'):
        code = hiplib.dtype_code(dtype)
        pages = [[CP.copy(rng.integers(1, 65, (1, PAGE, PAGE, c)) / 64.0, dtype) for c in CHANNELS] for _ in range(ROTATE)]
        for kind, turns in (('upright', 0), ('turned', 1)):
            bh, bw = (BOX_H, BOX_W) if turns == 0 else (BOX_W, BOX_H)
            zoom_h, zoom_w, out_w = line_crop_shape(bh, bw, turns, ZOOMED_HEIGHT, MINIMAL_WIDTH)
            y0 = [int(v) for v in rng.integers(0, PAGE - bh + 1, LINES)] * len(CHANNELS)
            x0 = [int(v) for v in rng.integers(0, PAGE - bw + 1, LINES)] * len(CHANNELS)
            cs = [c for c in CHANNELS for _ in range(LINES)]
            outs = [[CP.empty((1, zoom_h, out_w, c), dtype) for c in cs] for _ in range(ROTATE)]
            src_ptrs = [(ctypes.c_void_p * n)(*[page[CHANNELS.index(c)].ptr for c in cs]) for page in pages]
            out_ptrs = [(ctypes.c_void_p * n)(*[a.ptr for a in group]) for group in outs]
            out_ws = ints([out_w] * n)
            fixed = [ints([PAGE] * n), ints([PAGE] * n), ints(cs), ints(y0), ints(x0), ints([bh] * n), ints([bw] * n),
                     ints([turns] * n), ints([zoom_h] * n), ints([zoom_w] * n)]

            def call(i):
                j = i % ROTATE
                rt.call('uocr_line_crop', code, n, src_ptrs[j], *fixed, out_ptrs[j], out_ws)
            call_us = timed(call, args.reps)
            launches = rt.last_line_crop()[3]
            with rt.capture(torch.cuda.MemPool()) as graph:
                call(0)
            graphs.append(graph)
            replay_us = timed(lambda i: graph.replay(), args.reps)
            moved = sum((bh * bw + zoom_h * out_w) * c for c in cs) * np.dtype(dtype).itemsize
            floor_us = moved / COPY_GBS / 1e3
            results[dtype, kind] = replay_us
            print(f'{dtype:8s} {kind:8s} {launches:8d} | {call_us:6.1f} us {replay_us:9.1f} us | {moved / 1e6:8.2f} {floor_us:6.1f} us '
                  f'{call_us / floor_us:11.1f}x')
    for dtype in ('float32', 'float64', 'float16'):
        print(f'{dtype}: turned / upright = {results[dtype, "turned"] / results[dtype, "upright"]:.2f} (graph replay)')
    print('reference: CropRotateAndZoomLines (interpreter/interpreter.py:421-523) hands every (array, line) pair to a pool of at most '
          '8 processes that run ndimage.rotate and ndimage.zoom, between a device-to-host and a host-to-device copy of every '
          'array; it was not timed by this run')


if __name__ == '__main__':
    main()
