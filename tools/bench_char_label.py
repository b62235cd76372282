#!/usr/bin/env python3
"""Device CharLabel stage (uocr_char_label) on one page's worth of lines: 64 lines of 32 x 256 x 9, per dtype.

One call labels all 64 lines.  Event time per call after warm-up, on rotating buffers, for calls issued one after the
other from the host and for one call (on the first buffer set) captured into a HIP graph and replayed; the launches of a
call; the bytes it has to move at least (every line is read twice -- statistics, then vote -- and its labels are written once) and the time the d2d
copy rate of profiles/r03_membw.txt would need for them (the HBM floor).  The expected regime is launch latency: two
small launches.  The last lines set the figure beside the reference's, which was measured elsewhere: see the note.

    python tools/bench_char_label.py [--reps 50] > profiles/char_label_microbench.txt
"""
import argparse
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

COPY_GBS = 5176.0          # profiles/r03_membw.txt: d2d copy (1 read + 1 write)
ROTATE = 4
LINES, H, W, C, BITS, N_CHARS = 64, 32, 256, 9, 8, 162
REFERENCE_MS_PER_LINE = 68.0


def page(seed):
    """64 lines of bit layers with a class per column and a third of the pixels replaced: multiples of 1/64"""
    rng = np.random.default_rng(seed)
    codes = np.repeat(rng.integers(0, N_CHARS, (LINES, 1, W)), H, axis=1)
    codes = np.where(rng.random((LINES, H, W)) < 0.33, rng.integers(0, 1 << BITS, (LINES, H, W)), codes)
    bits = (codes[..., None] >> np.arange(C)) & 1
    bits[..., BITS:] = rng.integers(0, 2, (LINES, H, W, C - BITS))
    return np.where(bits == 1, rng.integers(56, 65, bits.shape), rng.integers(0, 9, bits.shape)) / 64.0


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--reps', type=int, default=50)
    args = parser.parse_args()
    import torch
    from univer_ocr_amd.hip import lib as hiplib
    from univer_ocr_amd.nn import CP
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

    print(f'uocr_char_label, {LINES} lines of {H} x {W} x {C} in one call, {N_CHARS} classes, on {rt.device_info()["name"]}')
    print(f'{"dtype":8s} {"launches":>8s} | {"call":>9s} {"graph replay":>12s} | {"MB moved":>8s} {"HBM floor":>9s} {"call / floor":>12s}')
    results, graphs = {}, []        # (the graphs live to the end: a pool must not be released while the next capture runs)
    for dtype in ('float32', 'float64', 'float16'):
        hosts = [page(seed) for seed in range(ROTATE)]
        xs = [[CP.copy(host[i:i + 1], dtype) for i in range(LINES)] for host in hosts]
        labels = [[CP.empty((W, N_CHARS), dtype) for _ in range(LINES)] for _ in range(ROTATE)]
        hs, ws = (ctypes.c_int * LINES)(*[H] * LINES), (ctypes.c_int * LINES)(*[W] * LINES)
        x_ptrs = [(ctypes.c_void_p * LINES)(*[a.ptr for a in group]) for group in xs]
        label_ptrs = [(ctypes.c_void_p * LINES)(*[a.ptr for a in group]) for group in labels]
        code = hiplib.dtype_code(dtype)

        def call(i):
            j = i % ROTATE
            rt.call('uocr_char_label', code, LINES, x_ptrs[j], hs, ws, C, BITS, N_CHARS, label_ptrs[j], None)
        call_us = timed(call, args.reps)
        launches = rt.last_char_label()[3]
        with rt.capture(torch.cuda.MemPool()) as graph:
            call(0)
        graphs.append(graph)
        replay_us = timed(lambda i: graph.replay(), args.reps)
        elem = np.dtype(dtype).itemsize
        moved = LINES * (2 * H * W * C + W * N_CHARS) * elem
        floor_us = moved / COPY_GBS / 1e3
        results[dtype] = call_us
        print(f'{dtype:8s} {launches:8d} | {call_us:6.1f} us {replay_us:9.1f} us | {moved / 1e6:8.2f} {floor_us:6.1f} us '
              f'{call_us / floor_us:11.1f}x')
    per_line = results['float32'] / LINES
    print(f'float32: {per_line:.2f} us per line inside one call of {LINES} lines, on the GPU named above (measured by this run)')
    print(f'reference: LabelChar._func1 (interpreter/interpreter.py:547-571, a Python loop per pixel) took '
          f'{REFERENCE_MS_PER_LINE:.0f} ms for ONE {H} x {W} x {C} line on a CPU-only development machine (timed there when the '
          f'stage was specified, not by this run); its worker pool spreads the lines of a page over at most 8 processes')


if __name__ == '__main__':
    main()
