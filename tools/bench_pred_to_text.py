#!/usr/bin/env python3
"""Device PredToText stage (uocr_pred_to_text) on one page's worth of lines: 64 lines of 256 x 162, one dtype per run.

One call reads all 64 lines.  Reported, each as the median over --reps repetitions on rotating buffers:
  call       device time of one uocr_pred_to_text call between two events (its launches included)
  wrapper    wall time of nn/ops.py: pred_to_text -- the call, the one device-to-host copy of counts and ids, the lists
  host path  wall time of what the stage replaces: a device-to-host copy of every line's prediction, then the NumPy
             restatement of the reference's rules (my_model/crop.py: pred_to_text_rules) on each
The expected regime is launch latency: two small launches over 64 x 256 x 162 elements.  Nobody set a target.

    (for d in float32 float64 float16; do timeout -k 10 120 python tools/bench_pred_to_text.py --dtype $d || exit; done) \\
        > profiles/pred_to_text_microbench.txt
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

ROTATE = 4
LINES, W = 64, 256


def page(seed, cls):
    """64 predictions with one clear maximum per row: a tenth tabs, a third of the neighbours in one pair class"""
    rng = np.random.default_rng(seed)
    n_chars, paired = len(cls), np.flatnonzero(cls >= 0)
    x = rng.integers(-32, 33, (LINES, W, n_chars))
    for line in x:
        last = 0
        for row in line:
            u = rng.random()
            mates = np.flatnonzero(cls == cls[last]) if cls[last] >= 0 else []
            last = 0 if u < 0.1 else int(rng.choice(mates)) if len(mates) and u < 0.45 else int(rng.choice(paired)) if u < 0.7 else int(rng.integers(1, n_chars))
            row[last] = 48 + rng.integers(0, 17)
    return x / 64.0


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--reps', type=int, default=50)
    parser.add_argument('--dtype', default='float32', choices=('float32', 'float64', 'float16'))
    args = parser.parse_args()
    from univer_ocr_amd.hip import lib as hiplib
    from univer_ocr_amd.my_model.crop import pair_classes, pred_to_text_rules
    from univer_ocr_amd.nn import CP, ops
    CP.use_gpu(0)
    rt = CP.runtime()
    cls = pair_classes()
    n_chars, dtype = len(cls), args.dtype
    ev = [ctypes.c_void_p() for _ in range(2)]
    for e in ev:
        assert rt.lib.uocr_event_create(ctypes.byref(e)) == 0

    hosts = [page(seed, cls) for seed in range(ROTATE)]
    xs = [[CP.copy(host[i], dtype) for i in range(LINES)] for host in hosts]
    ids = [[CP.empty((W,), np.uint8) for _ in range(LINES)] for _ in range(ROTATE)]
    counts = [CP.empty((LINES,), np.int32) for _ in range(ROTATE)]
    pointers = lambda values: (ctypes.c_void_p * LINES)(*values)
    x_ptrs = [pointers([a.ptr for a in group]) for group in xs]
    id_ptrs = [pointers([a.ptr for a in group]) for group in ids]
    count_ptrs = [pointers([c.ptr + 4 * i for i in range(LINES)]) for c in counts]
    ws, caps, table = (ctypes.c_int * LINES)(*[W] * LINES), (ctypes.c_int * LINES)(*[W] * LINES), (ctypes.c_int * n_chars)(*cls.tolist())
    code = hiplib.dtype_code(dtype)

    def call(i):
        j = i % ROTATE
        rt.call('uocr_pred_to_text', code, LINES, x_ptrs[j], ws, n_chars, table, id_ptrs[j], caps, count_ptrs[j])

    def device_us(i):
        rt.call('uocr_event_record', ev[0])
        call(i)
        rt.call('uocr_event_record', ev[1])
        ms = ctypes.c_float()
        assert rt.lib.uocr_event_elapsed_ms_sync(ev[0], ev[1], ctypes.byref(ms)) == 0
        return ms.value * 1e3

    def wall_us(fn, i):
        rt.synchronize()
        start = time.perf_counter()
        fn(i)
        return (time.perf_counter() - start) * 1e6

    def host_path(i):
        return [pred_to_text_rules(CP.asnumpy(a), cls) for a in xs[i % ROTATE]]

    def wrapper(i):
        return ops.pred_to_text(xs[i % ROTATE], cls)

    assert wrapper(0) == host_path(0), 'the device and the NumPy restatement read the page differently'
    emitted = sum(len(v) for v in wrapper(0))
    for i in range(5):
        call(i), wrapper(i)
    rt.synchronize()
    call_us = float(np.median([device_us(i) for i in range(args.reps)]))
    launches = rt.last_pred_to_text()[2]
    wrapper_us = float(np.median([wall_us(wrapper, i) for i in range(args.reps)]))
    host_us = float(np.median([wall_us(host_path, i) for i in range(max(3, args.reps // 10))]))
    print(f'uocr_pred_to_text, {LINES} lines of {W} x {n_chars} {dtype} in one call ({emitted} of {LINES * W} rows emit), '
          f'on {rt.device_info()["name"]}; medians of {args.reps}')
    print(f'  {dtype:8s} launches {launches} | call {call_us:8.1f} us | wrapper (call + readback) {wrapper_us:8.1f} us | '
          f'host path (copy every line + NumPy rules) {host_us:10.1f} us = {host_us / wrapper_us:6.1f}x the wrapper')


if __name__ == '__main__':
    main()
