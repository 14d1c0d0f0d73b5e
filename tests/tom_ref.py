"""numpy restatement of the topological overlap step of the from-data path
(NR_NET_TOM), as the test oracle: WGCNA's unsigned TOM with TOMDenom = "min"
of an adjacency a >= 0, its diagonal taken as 0.

    k_i  = sum_u a_ui                                   (u != i since a_ii = 0)
    L_ij = sum_u a_iu a_uj
    t_ij = (L_ij + a_ij) / (min(k_i, k_j) + 1 - a_ij)   i != j
    t_ii = 1

NaN propagates through every step (np.minimum keeps a NaN of either degree);
the diagonal is 1 whatever the rest holds. Since a <= 1 and k_i >= a_ij the
denominator is >= 1: nothing cancels.

The bar is relative: L and k are sums of n non-negative terms, so any
summation order is within (n - 1) 2^-53 of the exact sum, relative; the
denominator is >= 1 and at least as large as k, so its relative error is of
the same size; the add, the subtract and the divide put a few ulps on top:
(n + 16) 2^-52. Checked on the CPU in numpy fp64, in BLAS order and in a
shuffled sequential order, against a long-double evaluation for n = 17 .. 257
and the three network types: the worst case stayed below 3e-15 relative
against the bar's 6.1e-14 at n = 257.
"""
import numpy as np


def tom(a):
    """The TOM of a square adjacency (its diagonal is ignored)."""
    a = np.array(a, dtype=np.float64)
    n = a.shape[0]
    assert a.shape == (n, n)
    np.fill_diagonal(a, 0.0)
    with np.errstate(invalid="ignore"):
        k = a.sum(axis=0)
        t = (a @ a + a) / (np.minimum(k[:, None], k[None, :]) + 1.0 - a)
    np.fill_diagonal(t, 1.0)
    return t


def tom_bar(n):
    """Relative bar per element: |got - exp| <= tom_bar(n) |exp|."""
    return (n + 16) * 2.0 ** -52


def assert_tom_close(got, exp, n, what=""):
    """The criterion: same NaN pattern, |got - exp| <= tom_bar(n) |exp| per
    element (so exact where exp == 0). Returns the worst relative error."""
    got, exp = np.asarray(got), np.asarray(exp)
    nan = np.isnan(exp)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg=what)
    err = np.abs(got - exp)[~nan]
    lim = tom_bar(n) * np.abs(exp)[~nan]
    nz = lim > 0
    worst = float((err[nz] / np.abs(exp)[~nan][nz]).max()) if nz.any() else 0.0
    print(f"{what}: TOM relative error {worst:.3e} (bar {tom_bar(n):.3e})")
    assert (err <= lim).all(), f"{what}: relative error {worst:.3e} above {tom_bar(n):.3e}"
    return worst
