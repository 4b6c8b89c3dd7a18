"""The samples' Gram sums (include/genrich_amd.h, gx_coverage_gram) and the --correlation text in Python integers, for the tests.

x_s[b] = sample s's value of bin b.  n = the number of bins, n_zero = the bins that are 0 in every sample, sum[s] = the sum of
x_s, gram[i][j] = the sum of x_i[b] x_j[b]: Python ints, exact.  Pearson's r_ij = (N g_ij - s_i s_j) / sqrt((N g_ii - s_i^2)
(N g_jj - s_j^2)) with N = n, or n - n_zero when the all-zero bins are left out; the three differences are exact integers, the
quotient is taken with 80 decimal digits and printed with six."""
from __future__ import annotations

import decimal
from fractions import Fraction

import numpy as np

_CTX = decimal.Context(prec=80, rounding=decimal.ROUND_HALF_EVEN)


def gram(rows):
    """rows: a list of equally long integer arrays -> (n, n_zero, sum [S], gram [S][S]) as Python ints."""
    obj = [np.asarray(r).astype(object) for r in rows]
    n = len(obj[0]) if obj else 0
    assert all(len(r) == n for r in obj)
    S = len(obj)
    if n == 0:
        return 0, 0, [0] * S, [[0] * S for _ in range(S)]
    any_ = np.zeros(n, dtype=bool)
    for r in rows:
        any_ |= np.asarray(r) != 0
    sums = [int(r.sum()) for r in obj]
    g = [[0] * S for _ in range(S)]
    for i in range(S):
        for j in range(i, S):
            g[i][j] = g[j][i] = int(np.dot(obj[i], obj[j]))
    return n, int(n - any_.sum()), sums, g


def gram_int64(rows):
    """gram() for values small enough that every sum fits an int64 (checked): one integer matrix product."""
    X = np.asarray(rows, dtype=np.int64)
    S, n = X.shape
    assert n == 0 or int(X.max()) ** 2 * n < 1 << 63 and int(X.min()) >= 0
    G = X @ X.T
    return n, int(n - (X != 0).any(axis=0).sum()), [int(v) for v in X.sum(axis=1)], [[int(v) for v in row] for row in G]


def add(a, b):
    """The sums of two contexts (or of two sets of bins), added."""
    return (a[0] + b[0], a[1] + b[1], [x + y for x, y in zip(a[2], b[2])],
            [[x + y for x, y in zip(ra, rb)] for ra, rb in zip(a[3], b[3])])


def differences(n, n_zero, sums, g, skip_zeros=False):
    """(N, cov [S][S]): cov[i][j] = N g_ij - s_i s_j, exact."""
    N = n - n_zero if skip_zeros else n
    S = len(sums)
    return N, [[N * g[i][j] - sums[i] * sums[j] for j in range(S)] for i in range(S)]


def pearson_exact(n, n_zero, sums, g, skip_zeros=False):
    """[S][S] of None (no correlation: a flat sample, or N < 2; off the diagonal only) or r as a decimal.Decimal of 80 digits."""
    N, cov = differences(n, n_zero, sums, g, skip_zeros)
    S = len(sums)
    out = [[None] * S for _ in range(S)]
    for i in range(S):
        for j in range(S):
            if i == j:
                out[i][j] = decimal.Decimal(1)
            elif N >= 2 and cov[i][i] != 0 and cov[j][j] != 0:
                assert cov[i][i] > 0 and cov[j][j] > 0
                den = _CTX.sqrt(_CTX.multiply(decimal.Decimal(cov[i][i]), decimal.Decimal(cov[j][j])))
                out[i][j] = _CTX.divide(decimal.Decimal(cov[i][j]), den)
    return out


def boundary_distance(r):
    """How far r is from the nearest value at which its %.6f text changes (a half of 1e-6)."""
    x = Fraction(r) * 10 ** 6 - Fraction(1, 2)
    return float(abs(x - round(x))) * 1e-6


def value_text(r):
    if r is None:
        return "nan"
    q = r.quantize(decimal.Decimal("0.000001"), rounding=decimal.ROUND_HALF_EVEN, context=_CTX)
    text = f"{abs(q):.6f}"
    return ("-" if r < 0 else "") + text   # (printf's "-0.000000" for a small negative value)


def correlation_text(names, n, n_zero, sums, g, skip_zeros=False):
    """--correlation's file: a tab and the names, then per sample its name and its row."""
    r = pearson_exact(n, n_zero, sums, g, skip_zeros)
    lines = ["".join("\t" + s for s in names)]
    for i, name in enumerate(names):
        lines.append(name + "".join("\t" + value_text(v) for v in r[i]))
    return "\n".join(lines) + "\n"


def min_boundary_distance(n, n_zero, sums, g, skip_zeros=False):
    r = pearson_exact(n, n_zero, sums, g, skip_zeros)
    return min([boundary_distance(v) for i, row in enumerate(r) for j, v in enumerate(row) if i != j and v is not None], default=1.0)
