"""numpy restatement of the correlation types of the from-data path
(NR_COR_SPEARMAN, NR_COR_BICOR), as the test oracle. No scipy.

Both start from the *scaled* data xs (S x n; netbuild_ref.scale) and make a
second matrix z of the same shape, column by column;
corr = netbuild_ref.correlation(z) = clip(z^T z / (S - 1), -1, 1).

    Spearman: z = scale(r), r_i = L_i + (E_i + 1) / 2 with L_i the number of
        entries of the column less than x_i and E_i the number equal to it
        (itself included): R's rank(ties.method = "average"). +-Inf are
        ranked like any value; a column holding a NaN is all NaN.
    Bicor (WGCNA's, maxPOutliers = 1, pearsonFallback = "individual"):
        med = 0.5 (lo + hi), lo / hi the order statistics at 0-based positions
        (S - 1) // 2 and S // 2; d = |x - med|; mad = that median of d;
        u = (x - med) / (9 mad); w = (1 - u^2)^2 where |u| < 1, else 0;
        a = (x - med) w; mad == 0: a = x - mean(x);
        z = a sqrt(S - 1) / sqrt(sum a^2). A column with a non-finite entry is
        all NaN; an all-zero a gives 0 / 0 = NaN.
        An order statistic is taken as value + 0.0, so that a tie between
        -0.0 and +0.0 gives one result whichever entry is picked.

Bars (absolute, on corr):
    Spearman: netbuild_ref.corr_bar(S) -- the ranks are exact (multiples of
        1/2) and the rest is the Pearson pipeline on them.
    Bicor: (S + 64) 2^-52 -- S terms of summation rounding plus a few ulps
        each for u, w, a and the norm, with sum |z_i z_j| <= S - 1; med, mad
        and the mad == 0 decision are exact order statistics plus one exact
        halving and carry no error.
    net: netbuild_ref.net_bar's rule with the corresponding corr bar.
Checked on the CPU: for S = 2 .. 1,025 with continuous data, data rounded to
1/2 and Student-t (1.5 df) data, this float64 bicor and an 80-bit restatement
of it (from the same med and mad) differ on corr by at most 11.5 2^-52 (at
S = 257 and 500), against bars of 321 and 564 2^-52.
"""
import numpy as np

import netbuild_ref as R

COR_TYPES = ("spearman", "bicor")


def ranks(x):
    """Average ranks of each column of x (S x n), exact; O(S log S) a column."""
    x = np.asarray(x, dtype=np.float64)
    out = np.empty(x.shape)
    for j in range(x.shape[1]):
        col = x[:, j]
        if np.isnan(col).any():
            out[:, j] = np.nan
            continue
        _u, inv, cnt = np.unique(col, return_inverse=True, return_counts=True)
        less = np.cumsum(cnt) - cnt
        out[:, j] = less[inv] + (cnt[inv] + 1) / 2.0
    return out


def median(col):
    """0.5 (lo + hi) of the two middle order statistics (one for odd S)."""
    s = np.sort(col)
    n = s.shape[0]
    return 0.5 * ((s[(n - 1) // 2] + 0.0) + (s[n // 2] + 0.0))


def bicor_column(col):
    """(med, mad, a) of one finite column."""
    med = median(col)
    mad = median(np.abs(col - med))
    if mad == 0.0:
        return med, mad, col - col.mean()
    dx = col - med
    u = dx / (9.0 * mad)
    h = 1.0 - u * u
    return med, mad, dx * np.where(np.abs(u) < 1.0, h * h, 0.0)


def spearman_z(xs):
    return R.scale(ranks(xs))


def bicor_z(xs):
    xs = np.asarray(xs, dtype=np.float64)
    s = xs.shape[0]
    out = np.empty(xs.shape)
    for j in range(xs.shape[1]):
        col = xs[:, j]
        if not np.isfinite(col).all():
            out[:, j] = np.nan
            continue
        a = bicor_column(col)[2]
        with np.errstate(invalid="ignore", divide="ignore"):
            out[:, j] = a * np.sqrt(float(s - 1)) / np.sqrt((a * a).sum())
    return out


def z_of(xs, cor_type):
    return {"spearman": spearman_z, "bicor": bicor_z}[cor_type](xs)


def build(data, beta, net_type="unsigned", cor_type="spearman", do_scale=True):
    """(corr, net) of a data matrix (S x n) for a correlation type."""
    xs = R.scale(data) if do_scale else np.asarray(data, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        c = R.correlation(z_of(xs, cor_type))
    return c, R.network(c, beta, net_type)


def corr_bar(n_samples, cor_type):
    if cor_type == "spearman":
        return R.corr_bar(n_samples)
    assert cor_type == "bicor"
    return (n_samples + 64) * 2.0 ** -52


def net_bar(n_samples, beta, cor_type):
    """netbuild_ref.net_bar with the correlation type's corr bar."""
    assert beta >= 1
    return beta * corr_bar(n_samples, cor_type) + 1e-15
