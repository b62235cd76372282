#!/usr/bin/env python3
"""Device label overlap (uocr_label_overlap) on label planes with paragraph-like blobs: 8 pairs of 256 x 512 planes in one
call, and one pair of 1024 x 2048, caps 64 and 64.

Three forms, measured in turn -- a run is --reps repetitions of one form on rotating buffers, the forms alternate for
--runs runs each, and the figure of a form is its median run (each run: the median of its repetitions):
  call       device time of one uocr_label_overlap call between two events (its memset and launches included)
  wrapper    wall time of nn/ops.py: label_overlap -- the call and the one device-to-host copy of summary, rows and cols
  host path  wall time of what the call replaces: a device-to-host copy of both planes of every pair, the buckets and
             np.bincount on the pair index (--host-reps repetitions per run)
Beside them the read floor: the bytes of both planes over the HBM rate of profiles/r03_membw.txt (`add`, two reads and a
write: 5452 GB/s).  Nobody set a target.

    timeout -k 10 300 python tools/bench_mask_score.py > profiles/mask_score_microbench.txt
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

ROTATE = 4
CAP = 64
HBM_GB_S = 5452.0                                                  # profiles/r03_membw.txt: add (2 reads + 1 write)
WORKLOADS = (('8 pairs of 256 x 512', 8, 256, 512), ('1 pair of 1024 x 2048', 1, 1024, 2048))


def blobs(rng, h, w, count):
    """an (h, w) int32 plane of `count` rectangles that do not touch, numbered in reading order from 1 on: what
    uocr_label_batch makes of a paragraph mask"""
    plane = np.zeros((h, w), np.int32)
    boxes = []
    for _ in range(20 * count):
        bh, bw = int(rng.integers(h // 16, h // 4)), int(rng.integers(w // 8, w // 2))
        y, x = int(rng.integers(1, h - bh)), int(rng.integers(1, w - bw))
        if not plane[y - 1:y + bh + 1, x - 1:x + bw + 1].any():
            plane[y:y + bh, x:x + bw] = 1
            boxes.append((y, x, bh, bw))
        if len(boxes) == count:
            break
    for label, (y, x, bh, bw) in enumerate(sorted(boxes), 1):
        plane[y:y + bh, x:x + bw] = label
    return plane


def pair(rng, h, w):
    """the expected plane and a predicted one: the same blobs a few pixels off, one of them missing"""
    a = blobs(rng, h, w, 6)
    b = np.roll(a, (int(rng.integers(-3, 4)), int(rng.integers(-3, 4))), axis=(0, 1))
    b[b == 2] = 0
    return a, b


def host_table(a, b):
    bucket = lambda plane: np.minimum(plane.astype(np.int64) & 0xffffffff, CAP + 1)
    return np.bincount(bucket(a).ravel() * (CAP + 2) + bucket(b).ravel(), minlength=(CAP + 2) ** 2).reshape(CAP + 2, CAP + 2)


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--reps', type=int, default=30)
    parser.add_argument('--host-reps', type=int, default=5)
    parser.add_argument('--runs', type=int, default=7)
    args = parser.parse_args()
    from univer_ocr_amd.nn import CP, ops
    CP.use_gpu(0)
    rt = CP.runtime()
    ev = [ctypes.c_void_p() for _ in range(2)]
    for e in ev:
        assert rt.lib.uocr_event_create(ctypes.byref(e)) == 0

    for name, n, h, w in WORKLOADS:
        rng = np.random.default_rng(h)
        hosts = [[pair(rng, h, w) for _ in range(n)] for _ in range(ROTATE)]
        device = [[(CP.copy(a, np.int32), CP.copy(b, np.int32)) for a, b in group] for group in hosts]
        pointers = lambda values: (ctypes.c_void_p * n)(*values)
        a_ptrs = [pointers([a.ptr for a, _ in group]) for group in device]
        b_ptrs = [pointers([b.ptr for _, b in group]) for group in device]
        hs, ws = (ctypes.c_int * n)(*[h] * n), (ctypes.c_int * n)(*[w] * n)
        side = CAP + 2
        outs = [(CP.empty((n, side, side), np.int32), CP.empty((n, side, 4), np.int32), CP.empty((n, side, 4), np.int32),
                 CP.empty((n, 8), np.int64)) for _ in range(ROTATE)]

        def call(i):
            j = i % ROTATE
            rt.call('uocr_label_overlap', n, a_ptrs[j], b_ptrs[j], hs, ws, CAP, CAP, *(ctypes.c_void_p(o.ptr) for o in outs[j]))

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
            return [host_table(CP.asnumpy(a), CP.asnumpy(b)) for a, b in device[i % ROTATE]]

        def wrapper(i):
            return ops.label_overlap(device[i % ROTATE], CAP, CAP)

        call(0)
        assert np.array_equal(CP.asnumpy(outs[0][0]), np.array(host_path(0))), 'the device and the host path count differently'
        summary = wrapper(0)[0]
        assert np.array_equal(summary, CP.asnumpy(outs[0][3]))
        for i in range(5):
            call(i), wrapper(i)
        rt.synchronize()
        runs = {'call': [], 'wrapper': [], 'host': []}
        for run in range(args.runs):                                     # the forms in turn
            runs['call'].append(float(np.median([device_us(i) for i in range(args.reps)])))
            runs['wrapper'].append(float(np.median([wall_us(wrapper, i) for i in range(args.reps)])))
            runs['host'].append(float(np.median([wall_us(host_path, i) for i in range(args.host_reps)])))
        call_us, wrapper_us, host_us = (float(np.median(runs[form])) for form in ('call', 'wrapper', 'host'))
        spread = {form: (min(values), max(values)) for form, values in runs.items()}
        read_bytes = 2 * 4 * n * h * w
        floor_us = read_bytes / (HBM_GB_S * 1e3)
        print(f'uocr_label_overlap, {name} int32 label planes in one call, caps {CAP} and {CAP} ({int(summary[:, 4].sum())} expected, '
              f'{int(summary[:, 5].sum())} predicted, {int(summary[:, 6].sum())} matched components), on {rt.device_info()["name"]}; '
              f'the median of {args.runs} runs of {args.reps} repetitions ({args.host_reps} of the host path), the forms in turn')
        print(f'  call {call_us:8.1f} us ({spread["call"][0]:.1f} .. {spread["call"][1]:.1f}) | read floor {floor_us:6.1f} us '
              f'({read_bytes / 1e6:.1f} MB at {HBM_GB_S:.0f} GB/s) | wrapper (call + readback) {wrapper_us:8.1f} us '
              f'({spread["wrapper"][0]:.1f} .. {spread["wrapper"][1]:.1f}) | host path (copy both planes + np.bincount) '
              f'{host_us:10.1f} us ({spread["host"][0]:.1f} .. {spread["host"][1]:.1f}) = {host_us / wrapper_us:6.1f}x the wrapper')


if __name__ == '__main__':
    main()
