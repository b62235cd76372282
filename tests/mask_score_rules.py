"""The rules of the label overlap (uocr_label_overlap) and of the numbers taken from it, restated in NumPy from their
statement in include/univer_hip.h, not from the kernels: buckets, the overlap table, its rows and columns, the summary,
and the ratios of my_model/evaluate.py.  Counts are integers: every comparison against this file is by equality."""
import numpy as np


def bucket(labels, cap):
    """l where 0 <= l <= cap, else cap + 1 (the overflow); int32 labels are compared as unsigned: a negative one overflows"""
    unsigned = np.asarray(labels, np.int32).astype(np.int64) & 0xffffffff
    return np.where(unsigned <= cap, unsigned, cap + 1)


def overlap_table(a, b, cap_a, cap_b):
    """int64 (cap_a + 2, cap_b + 2): the pixels per pair of buckets of the expected plane a and the predicted plane b"""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape
    pair = bucket(a, cap_a).ravel() * (cap_b + 2) + bucket(b, cap_b).ravel()
    return np.bincount(pair, minlength=(cap_a + 2) * (cap_b + 2)).reshape(cap_a + 2, cap_b + 2).astype(np.int64)


def table_rows(table):
    """int64 (rows of the table, 4) = area, best, inter, other per row: best among the columns 1 .. cap (the last column
    is the overflow) with the largest count > 0, the smallest index on a tie, 0 without one"""
    table = np.asarray(table, np.int64)
    cap = table.shape[1] - 2
    out = np.zeros((table.shape[0], 4), np.int64)
    out[:, 0] = table.sum(axis=1)
    column_area = table.sum(axis=0)
    if cap >= 1:
        inner = table[:, 1:cap + 1]
        first_largest = inner.argmax(axis=1)                            # (argmax keeps the first of equal maxima)
        inter = inner[np.arange(len(inner)), first_largest]
        found = inter > 0
        out[found, 1] = first_largest[found] + 1
        out[found, 2] = inter[found]
        out[found, 3] = column_area[out[found, 1]]
    return out


def summary(table):
    """int64 (8,) = tp, fp, fn, tn, expected, predicted, matched, overflow"""
    table = np.asarray(table, np.int64)
    rows, cols = table_rows(table), table_rows(table.T)
    cap_a, cap_b = table.shape[0] - 2, table.shape[1] - 2
    inner = rows[1:cap_a + 1]
    matched = (inner[:, 1] > 0) & (2 * inner[:, 2] > inner[:, 0] + inner[:, 3] - inner[:, 2])
    overflow = table[cap_a + 1].sum() + table[:, cap_b + 1].sum() - table[cap_a + 1, cap_b + 1]
    return np.array([table[1:, 1:].sum(), table[0, 1:].sum(), table[1:, 0].sum(), table[0, 0],
                     (rows[1:cap_a + 1, 0] > 0).sum(), (cols[1:cap_b + 1, 0] > 0).sum(), matched.sum(), overflow], np.int64)


def everything(a, b, cap_a, cap_b):
    """(overlap, rows, cols, summary) of one pair of planes"""
    table = overlap_table(a, b, cap_a, cap_b)
    return table, table_rows(table), table_rows(table.T), summary(table)


def ratio(numerator, denominator):
    return numerator / denominator if denominator else None


def pixel_numbers(tp, fp, fn, tn, beta=1):
    """accuracy, precision, recall, f-beta from the four counts, by the reference's formulas (nn/metrics.py:
    binary_classification_metrics); None where a denominator is 0"""
    tp, fp, fn, tn = int(tp), int(fp), int(fn), int(tn)
    precision, recall = ratio(tp, tp + fp), ratio(tp, tp + fn)
    f = None
    if precision is not None and recall is not None:
        f = ratio((1 + beta ** 2) * precision * recall, beta ** 2 * precision + recall)
    return ratio(tp + tn, tp + tn + fp + fn), precision, recall, f


def matched_ious(rows):
    """the IoU of every expected component 1 .. cap that has a match, from its row"""
    inner = np.asarray(rows, np.int64)[1:-1]
    ok = (inner[:, 1] > 0) & (2 * inner[:, 2] > inner[:, 0] + inner[:, 3] - inner[:, 2])
    return [int(i) / int(a + o - i) for a, _, i, o in inner[ok]]
