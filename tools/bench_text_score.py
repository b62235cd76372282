#!/usr/bin/env python3
"""Device text score (uocr_text_score) on one page's worth of lines: 64 lines of 256 x 162 predictions and labels, one
dtype per run.

One call scores all 64 lines.  Three forms, measured in turn -- a run is --reps repetitions of one form on rotating
buffers, the forms alternate for --runs runs each, and the figure of a form is its median run (each run: the median of
its repetitions):
  call       device time of one uocr_text_score call between two events (its launches included)
  wrapper    wall time of nn/ops.py: text_score with want_ids=True -- the call, the one device-to-host copy of scores
             and ids, the lists
  host path  wall time of what the stage replaces: a device-to-host copy of every line's prediction and labels, the
             reading of both in NumPy, the edit distance as a Python loop (--host-reps repetitions per run: it is slow)
Nobody set a target.

    (for d in float32 float64 float16; do timeout -k 10 300 python tools/bench_text_score.py --dtype $d || exit; done) \\
        > profiles/text_score_microbench.txt
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


def page(seed, n_chars):
    """64 (prediction, labels) pairs: the labels one-hot with runs of 1 to 4 columns and a background column now and
    then; the prediction a clear maximum per row, at the label's id nine times in ten"""
    rng = np.random.default_rng(seed)
    preds = rng.integers(-32, 33, (LINES, W, n_chars))
    labels = np.zeros((LINES, W, n_chars))
    for pred, label in zip(preds, labels):
        row = 0
        while row < W:
            char_id = 0 if rng.random() < 0.25 else int(rng.integers(1, n_chars))
            for r in range(row, min(W, row + int(rng.integers(1, 5)))):
                label[r, char_id] = 1.0
                pred[r, char_id if rng.random() < 0.9 else int(rng.integers(0, n_chars))] = 48 + rng.integers(0, 17)
                row = r + 1
    return preds / 64.0, labels


def host_reading(M):
    """the reading of M (W, n_chars) in NumPy"""
    M = M.astype(np.float32) if M.dtype == np.float16 else M
    with np.errstate(invalid='ignore'):
        maxima = M.max(axis=1)
        ids = np.where(np.isnan(maxima) | (maxima == 0.0), -1, np.argmax(M == maxima[:, None], axis=1))
    keep = (ids > 0) & np.concatenate([[True], ids[1:] != ids[:-1]])
    return ids[keep].tolist()


def host_distance(a, b, canon):
    a, b = [canon[x] for x in a], [canon[y] for y in b]
    row = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        above, row = row, [i]
        for j, y in enumerate(b, 1):
            row.append(min(above[j] + 1, row[j - 1] + 1, above[j - 1] + (x != y)))
    return row[-1]


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--reps', type=int, default=30)
    parser.add_argument('--host-reps', type=int, default=3)
    parser.add_argument('--runs', type=int, default=7)
    parser.add_argument('--dtype', default='float32', choices=('float32', 'float64', 'float16'))
    args = parser.parse_args()
    from univer_ocr_amd.hip import lib as hiplib
    from univer_ocr_amd.my_model.crop import canonical_ids
    from univer_ocr_amd.nn import CP, ops
    CP.use_gpu(0)
    rt = CP.runtime()
    canon = canonical_ids().tolist()
    n_chars, dtype = len(canon), args.dtype
    ev = [ctypes.c_void_p() for _ in range(2)]
    for e in ev:
        assert rt.lib.uocr_event_create(ctypes.byref(e)) == 0

    hosts = [page(seed, n_chars) for seed in range(ROTATE)]
    xs = [[CP.copy(preds[i], dtype) for i in range(LINES)] for preds, _ in hosts]
    ys = [[CP.copy(labels[i], dtype) for i in range(LINES)] for _, labels in hosts]
    ids = [[CP.empty((2 * W,), np.uint8) for _ in range(LINES)] for _ in range(ROTATE)]
    scores = [CP.empty((LINES, 4), np.int32) for _ in range(ROTATE)]
    pointers = lambda values: (ctypes.c_void_p * LINES)(*values)
    x_ptrs = [pointers([a.ptr for a in group]) for group in xs]
    y_ptrs = [pointers([a.ptr for a in group]) for group in ys]
    read_ptrs = [pointers([a.ptr for a in group]) for group in ids]
    expected_ptrs = [pointers([a.ptr + W for a in group]) for group in ids]
    ws, table = (ctypes.c_int * LINES)(*[W] * LINES), (ctypes.c_int * n_chars)(*canon)
    code = hiplib.dtype_code(dtype)

    def call(i):
        j = i % ROTATE
        rt.call('uocr_text_score', code, LINES, x_ptrs[j], y_ptrs[j], ws, n_chars, table, read_ptrs[j], expected_ptrs[j], scores[j].ptr)

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
        result = []
        for x, y in zip(xs[i % ROTATE], ys[i % ROTATE]):
            read, expected = host_reading(CP.asnumpy(x)), host_reading(CP.asnumpy(y))
            result.append(([host_distance(expected, read, canon), len(expected), len(read)], read, expected))
        return result

    def wrapper(i):
        return ops.text_score(xs[i % ROTATE], ys[i % ROTATE], canon, want_ids=True)

    got, reference = wrapper(0), host_path(0)
    assert got[0].tolist() == [r[0] for r in reference] and got[1] == [r[1] for r in reference] and got[2] == [r[2] for r in reference], \
        'the device and the host path score the page differently'
    expected_chars, read_chars, distance = (int(got[0][:, k].sum()) for k in (1, 2, 0))
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
    print(f'uocr_text_score, {LINES} lines of {W} x {n_chars} {dtype} predictions and labels in one call ({expected_chars} expected, '
          f'{read_chars} read characters, distance {distance}), on {rt.device_info()["name"]}; the median of {args.runs} runs of '
          f'{args.reps} repetitions ({args.host_reps} of the host path), the forms in turn')
    print(f'  {dtype:8s} call {call_us:8.1f} us ({spread["call"][0]:.1f} .. {spread["call"][1]:.1f}) | wrapper (call + readback) '
          f'{wrapper_us:8.1f} us ({spread["wrapper"][0]:.1f} .. {spread["wrapper"][1]:.1f}) | host path (copy every matrix + NumPy '
          f'reading + Python distance) {host_us:10.1f} us ({spread["host"][0]:.1f} .. {spread["host"][1]:.1f}) = '
          f'{host_us / wrapper_us:6.1f}x the wrapper')


if __name__ == '__main__':
    main()
