#!/usr/bin/env python3
"""Largest relative error of the library's float32 Sigmoid, 1.f / (1.f + expf(-v)), against float64.

uocr_act_fwd(SIGMOID) evaluates the expression of act_apply (uocr_common.h) with the expf of the build on a dense
grid of v in [-90, 90]; the error is counted in u = 2^-24 (half an ulp) of the float64 value, over the v whose Sigmoid
is a normal float32 (below 2^-126 the result may be flushed).  tests/elementwise_bound.py takes SIGMOID_K, the k of
its Sigmoid bound, as twice the largest figure printed here, rounded up.
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))

U32 = 2.0 ** -24
POINTS = 1 << 23


def sigmoid64(v):
    v = np.asarray(v, dtype=np.float64)
    e = np.exp(-np.abs(v))
    return np.where(v >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def main():
    from univer_ocr_amd.nn import CP, ops
    CP.use_gpu(0)
    CP.set_dtype('float32')
    rng = np.random.default_rng(0)
    grids = (('linear', np.linspace(-90.0, 90.0, POINTS + 1)),
             ('random', rng.uniform(-90.0, 90.0, POINTS)),
             ('near 0', rng.uniform(-1.0, 1.0, POINTS) * 2.0 ** rng.integers(-20, 1, POINTS)))
    worst = 0.0
    for name, grid in grids:
        v = grid.astype(np.float32)
        y = CP.asnumpy(ops.act_fwd('sigmoid', CP.copy(v))).astype(np.float64)
        ref = sigmoid64(v)
        normal = ref >= 2.0 ** -126
        err = np.abs(y - ref) / (ref * U32)
        assert not np.isnan(y).any()
        for lo, hi in ((-90, -20), (-20, -4), (-4, 4), (4, 20), (20, 90)):
            sel = normal & (v >= lo) & (v <= hi)
            if not sel.any():
                continue
            i =np.flatnonzero(sel)[np.argmax(err[sel])]
            print(f'{name:7s} v in [{lo:4d}, {hi:3d}]: largest error {err[i]:.3f} u at v = {float(v[i])!r}')
        below = ~normal
        print(f'{name:7s} Sigmoid below 2^-126: {int(below.sum())} points, largest result {y[below].max() if below.any() else 0.0:.3e}, '
              f'exactly 0 for v < -88.72: {bool(np.all(y[v < -88.73] == 0.0))}')
        worst = max(worst, float(err[normal].max()))
    print(f'largest relative error {worst:.3f} u (u = 2^-24); k = ceil(2 x {worst:.3f}) = {math.ceil(2 * worst)}')


if __name__ == '__main__':
    main()
