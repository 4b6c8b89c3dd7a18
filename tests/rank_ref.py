"""The samples' doubled mid-ranks (include/genrich_amd.h, gx_coverage_distinct .. gx_coverage_spearman_group) and the --spearman
text in numpy and Python integers, for the tests.

x_s[b] = sample s's value of bin b.  B = the ranked bins: all of them, or with skip_zeros those that are not 0 in every sample
(taken out before ranking).  less_s(v) / equal_s(v) = the bins of B whose x_s is below / equal to v;
R_s[b] = 2 less + equal + 1 on B (twice the average rank, counted from 1) and 0 outside B.  Spearman's rho is Pearson's r of the
rows R over B: gram_ref's arithmetic with n = |B| and no zero bins."""
from __future__ import annotations

import numpy as np

import gram_ref


def distinct(row):
    """(values ascending, counts) of one row, both uint64."""
    v, c = np.unique(np.asarray(row, dtype=np.uint64), return_counts=True)
    return v.astype(np.uint64), c.astype(np.uint64)


def kept(rows, skip_zeros=False):
    """The mask of B over the bins, and n_zero (the bins that are 0 in every row)."""
    X = [np.asarray(r, dtype=np.uint64) for r in rows]
    n = len(X[0]) if X else 0
    any_ = np.zeros(n, dtype=bool)
    for x in X:
        any_ |= x != 0
    return (any_ if skip_zeros else np.ones(n, dtype=bool)), int(n - any_.sum())


def table(row, keep):
    """(values ascending, rank2) of one row over the bins of the mask."""
    vals, cnt = np.unique(np.asarray(row, dtype=np.uint64)[keep], return_counts=True)
    cnt = cnt.astype(np.int64)
    less = np.cumsum(cnt) - cnt
    return vals.astype(np.uint64), (2 * less + cnt + 1).astype(np.uint64)


def tables(rows, skip_zeros=False):
    keep, _ = kept(rows, skip_zeros)
    return [table(r, keep) for r in rows]


def rank_rows(rows, skip_zeros=False):
    """(N, n_zero, R): R uint64 [S, n], 0 outside B."""
    X = [np.asarray(r, dtype=np.uint64) for r in rows]
    keep, n_zero = kept(X, skip_zeros)
    n = len(keep)
    R = np.zeros((len(X), n), dtype=np.uint64)
    for s, x in enumerate(X):
        vals, inv, cnt = np.unique(x[keep], return_inverse=True, return_counts=True)
        cnt = cnt.astype(np.int64)
        less = np.cumsum(cnt) - cnt
        R[s, keep] = (2 * less + cnt + 1)[inv.reshape(-1)].astype(np.uint64)
    return int(keep.sum()), n_zero, R


def sums_of(R, N):
    """(sum [S], gram [S][S]) of rank rows, exact Python ints."""
    if len(R) == 0 or R.shape[1] == 0:
        S = len(R)
        return [0] * S, [[0] * S for _ in range(S)]
    if 4 * R.shape[1] ** 3 < 1 << 63:   # (a rank is at most twice the number of bins)
        _, _, s, g = gram_ref.gram_int64(R.astype(np.int64))
    else:
        _, _, s, g = gram_ref.gram(list(R))
    return s, g


def spearman(rows, skip_zeros=False):
    """(N, n_zero, sum [S], gram [S][S]) of the rank rows: what gx_coverage_spearman_group gives (and n_zero)."""
    N, n_zero, R = rank_rows(rows, skip_zeros)
    s, g = sums_of(R, N)
    return N, n_zero, s, g


def spearman_text(names, rows, skip_zeros=False):
    """--spearman's file."""
    N, _, s, g = spearman(rows, skip_zeros)
    return gram_ref.correlation_text(names, N, 0, s, g, False)


def rho(rows, skip_zeros=False):
    """[S][S] of None or decimal.Decimal: gram_ref.pearson_exact of the rank rows."""
    N, _, s, g = spearman(rows, skip_zeros)
    return gram_ref.pearson_exact(N, 0, s, g, False)


def min_boundary_distance(rows, skip_zeros=False):
    N, _, s, g = spearman(rows, skip_zeros)
    return gram_ref.min_boundary_distance(N, 0, s, g, False)
