#!/usr/bin/env python3
"""Generate tests/golden/mask_score.npz: what the REFERENCE's binary_classification_metrics (nn/metrics.py:4-21) says of
a dozen small 0/1 arrays (needs the reference checkout; see make_golden.py, whose import stand-ins this script reuses by
importing it).  Only inputs and outputs are stored.

    python tests/golden/make_golden_mask_score.py

Contents
  names       the cases, a unicode array
  per case    {name}/prediction, {name}/truth   int64 0/1 arrays of one shape (1-D or 2-D)
              {name}/beta1, {name}/beta2        float64 (4,): accuracy, precision, recall, f1 as the reference returned
                                                them with f1beta = 1 and f1beta = 2

In every case all four counts (true / false positives / negatives) are positive (asserted): the reference divides by zero
otherwise.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402,F401  (installs the stand-ins, puts the reference on sys.path)
from make_golden_crops import save_reproducible  # noqa: E402

from components.nn.metrics import binary_classification_metrics  # noqa: E402


def cases():
    r = np.random.default_rng(29)
    yield 'four', np.array([1, 1, 0, 0]), np.array([1, 0, 1, 0])
    for index, (shape, p_pred, p_true) in enumerate([((7,), .5, .5), ((5, 9), .3, .6), ((16, 16), .1, .1), ((3, 40), .9, .8),
                                                     ((33, 17), .5, .05), ((64, 32), .02, .5), ((1, 200), .7, .7),
                                                     ((48, 48), .25, .25), ((9, 9), .5, .4)]):
        while True:
            prediction, truth = (r.random(shape) < p_pred).astype(np.int64), (r.random(shape) < p_true).astype(np.int64)
            if all(((prediction == p) & (truth == t)).any() for p in (0, 1) for t in (0, 1)):
                break
        yield f'random{index}', prediction, truth
    truth = np.zeros((24, 24), np.int64)
    truth[4:12, 3:20] = truth[14:22, 3:20] = 1                       # two blocks, predicted as one with a margin missing
    prediction = np.zeros_like(truth)
    prediction[5:22, 4:21] = 1
    yield 'blocks', prediction, truth
    yield 'inverted', 1 - prediction, truth


def main():
    out, names = {}, []
    for name, prediction, truth in cases():
        prediction, truth = prediction.astype(np.int64), truth.astype(np.int64)
        counts = [int(((prediction == p) & (truth == t)).sum()) for p, t in ((1, 1), (1, 0), (0, 1), (0, 0))]
        assert min(counts) > 0, (name, counts)
        names.append(name)
        out[f'{name}/prediction'], out[f'{name}/truth'] = prediction, truth
        for beta in (1, 2):
            result = binary_classification_metrics(prediction, truth, f1beta=beta)
            out[f'{name}/beta{beta}'] = np.array([result.accuracy, result.precision, result.recall, result.f1], np.float64)
        print(f'{name:9s} {str(prediction.shape):9s} tp fp fn tn = {counts}  {out[f"{name}/beta1"]}')
    assert len(names) == 12
    out['names'] = np.array(names)
    save_reproducible('mask_score', out)


if __name__ == '__main__':
    main()
