"""The rules of the text score (csrc/text_score.hip), restated in NumPy and plain Python: what the device must EQUAL.
No tolerance anywhere: the rules compare and count.  tests/test_text_score_host.py pins them; the GPU tests compare the
library with them."""
import numpy as np


def row_ids(M):
    """the id of every row of M (W, n_chars): -1 where the row holds a NaN or its maximum == 0.0 (-0.0 too), otherwise the
    smallest column that equals the row's maximum (a negative maximum is an ordinary one).  binary16 is widened, which is
    exact."""
    M = np.asarray(M)
    M = M.astype(np.float32) if M.dtype == np.float16 else M
    ids = []
    for row in M:
        if np.isnan(row).any() or row.max() == 0.0:
            ids.append(-1)
        else:
            ids.append(int(np.flatnonzero(row == row.max())[0]))
    return ids


def collapse(ids):
    """one id per run of equal row ids; id 0 (the tab, the background class) and -1 emit nothing and end a run"""
    return [i for r, i in enumerate(ids) if i > 0 and (r == 0 or i != ids[r - 1])]


def reading(M):
    """the ids a matrix (W, n_chars) reads as: the Char net's raw output and the one-hot labels alike"""
    return collapse(row_ids(M))


def distance(a, b, canon):
    """the unit-cost Levenshtein distance between the id lists a and b; x and y match when canon[x] == canon[y]"""
    a, b = [int(canon[x]) for x in a], [int(canon[y]) for y in b]
    row = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        above, row = row, [i]
        for j, y in enumerate(b, 1):
            row.append(min(above[j] + 1, row[j - 1] + 1, above[j - 1] + (x != y)))
    return row[-1]


def score(pred, label, canon):
    """(distance, len(reading(label)), len(reading(pred))) of one line, and the two readings: (scores, read, expected)"""
    read, expected = reading(pred), reading(label)
    return (distance(expected, read, canon), len(expected), len(read)), read, expected


def identity(n_chars):
    return np.arange(n_chars, dtype=np.int32)


def look_alikes_equal(pairs, n_chars):
    """both members of every (Cyrillic, Latin) pair map to the Cyrillic one"""
    canon = identity(n_chars)
    for cyrillic, latin in pairs:
        canon[latin] = cyrillic
    return canon
