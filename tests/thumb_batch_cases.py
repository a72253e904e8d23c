"""Inputs of tests/test_thumb_batch_gpu.py that are constructed rather than drawn, and the restatement of the thumbnail growth
they are checked with.  Every promised property is asserted without a device in tests/test_thumb_batch_cpu.py.
Test helper, not part of the package."""
import numpy as np

GROW_N, GROW_M = 60, 4              # R = 57; band 0 and limits (0, 1): only the cells below the diagonal are masked


def walk(filtered, row, col, m_filter):
    """audioSegmentation._grow_thumbnail (audioSegmentation.py:1167-1182) with a record of how it went:
    ((i1, i2, j1, j2), backward steps, forward steps, forward steps taken on equal or unordered neighbours,
    the four break conditions at the end -- all False when the thumbnail reached m_filter cells)."""
    i1 = i2 = int(row)
    j1 = j2 = int(col)
    last = filtered.shape[0] - 2
    back = fwd = ties = 0
    stop = (False,) * 4
    while i2 - i1 < m_filter:
        stop = (i1 <= 0, j1 <= 0, i2 >= last, j2 >= last)
        if any(stop):
            break
        stop = (False,) * 4
        a, b = filtered[i1 - 1, j1 - 1], filtered[i2 + 1, j2 + 1]
        if a > b:
            i1, j1, back = i1 - 1, j1 - 1, back + 1
        else:
            i2, j2, fwd = i2 + 1, j2 + 1, fwd + 1
            ties += int(not a < b)
    return (i1, i2, j1, j2), back, fwd, ties, stop


def stripe_matrix(n, d, m_filter, profile, nan_at=None):
    """Symmetric n x n matrix that is zero except on the diagonals +-d, chosen so that its window sums along that diagonal are
    the given profile: filtered[i][i + d] = profile.get(i, 0) (solved backwards from the end of the diagonal; multiples of
    1/16 stay exact).  nan_at: a position of the diagonal that is overwritten by NaN afterwards."""
    length = n - d
    g = np.zeros(length + m_filter)
    for i in range(length - m_filter, -1, -1):
        g[i] = profile.get(i, 0.0) - g[i + 1:i + m_filter].sum()
    if nan_at is not None:
        g[nan_at] = np.nan
    S = np.zeros((n, n))
    i = np.arange(length)
    S[i, i + d] = g[:length]
    S[i + d, i] = g[:length]
    return S


def grow_cases():
    """name -> (similarity matrix [GROW_N][GROW_N], expected arg-max, what the walk must do: the break conditions at its end,
    backward steps, forward steps, forward steps on equal neighbours).  R = 57, so R - 2 = 55."""
    n, m = GROW_N, GROW_M
    hill = {20: 0.25, 21: 0.5, 22: 0.75, 23: 1.0, 24: 1.0, 25: 0.75, 26: 0.5, 27: 0.25}          # symmetric about row 23.5
    none = (False,) * 4
    return {
        "row_0": (stripe_matrix(n, 7, m, {0: 1.0}), (0, 7), ((True, False, False, False), 0, 0, 0)),
        "column_0": (stripe_matrix(n, 0, m, {0: 1.0}), (0, 0), ((True, True, False, False), 0, 0, 0)),
        "row_R_minus_2": (stripe_matrix(n, 1, m, {55: 1.0}), (55, 56), ((False, False, True, True), 0, 0, 0)),
        "column_R_minus_2": (stripe_matrix(n, 5, m, {50: 1.0}), (50, 55), ((False, False, False, True), 0, 0, 0)),
        # 0.75 ahead against 0.5 behind: forward; 0.5 = 0.5: forward, into column R - 2
        "walks_into_column_R_minus_2": (stripe_matrix(n, 5, m, {47: 0.5, 48: 1.0, 49: 0.75, 50: 0.5}), (48, 53),
                                        ((False, False, False, True), 0, 2, 1)),
        # first maximum at row 23 (= row 24).  1 ahead, 0.75 behind: forward; 0.75 = 0.75: forward; 0.75 behind, 0.5 ahead:
        # backward; 0.5 = 0.5: forward -> m_filter cells
        "interior_both_ways": (stripe_matrix(n, 10, m, hill), (23, 33), (none, 1, 3, 2)),
        "equal_neighbours": (stripe_matrix(n, 3, m, {30: 1.0}), (30, 33), (none, 0, 4, 4)),
        "backward_only": (stripe_matrix(n, 20, m, {8: 0.0625, 9: 0.125, 10: 0.25, 11: 0.5, 12: 1.0}), (12, 32), (none, 4, 0, 0)),
        # a NaN makes the minimum NaN, so every masked cell is NaN and numpy's arg-max is the first of them, (1, 0): the walk ends
        # at once in column 0 -- through the filter a NaN neighbour is never walked over
        "nan": (stripe_matrix(n, 12, m, {30: 1.0}, nan_at=20), (1, 0), ((False, True, False, False), 0, 0, 0)),
    }


def symmetric_matrix(n, seed):
    """Symmetric bit for bit, entries uniform in [-1, 1], unit diagonal."""
    rng = np.random.default_rng(seed)
    A = rng.uniform(-1.0, 1.0, (n, n))
    S = np.triu(A, 1) + np.triu(A, 1).T
    np.fill_diagonal(S, 1.0)
    return np.ascontiguousarray(S)
