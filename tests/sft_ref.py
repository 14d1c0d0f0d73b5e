"""numpy restatement of the soft-threshold pick (nr_soft_connectivity,
netrep_ScaleFreeFit, netrep_PickSoftThreshold), as the test oracle. WGCNA is
not available to the tests: the definitions in include/netrep_gpu.h are the
contract, restated here.

Connectivity, from a correlation matrix c (clamped to [-1, 1] already):

    b = |c|                      unsigned
        (1 + c) / 2              signed
        c where c > 0, else 0    signed_hybrid (NaN stays NaN)
    k[i, m] = sum over u != i of b[i, u] ** powers[m]

Scale-free fit of one k (scaleFreeFitIndex with R's cut): B = n_breaks bins,
dx = max - min, edges e_m = min + m (dx / B); node i is in bin
1 + #{m in 1 .. B-1 : k_i > e_m}; p_m = count_m / n; d_m = the bin's mean of
k, or the bin's midpoint if the bin is empty or that mean is 0;
x = log10(d), y = log10(p + 1e-9); remove_first drops bin 1. Fit 1: y ~ x by
least squares, R^2 = 1 - SSR / SST and the slope. Fit 2: y ~ x + d, adjusted
R^2 = 1 - (1 - R^2) (N - 1) / (N - 3) (NaN for N <= 3). A constant or
non-finite k gives three NaNs.

The two bars, and where they come from:

CONNECTIVITY, relative per entry: (n + 2 p_max + 16) 2^-52, exact where the
expected value is 0. A sum of n - 1 non-negative terms in any order is within
(n - 1) 2^-53 of the exact sum, relative; each term is a chain of at most
p - 1 multiplications (half an ulp each) or one pow (an ulp), against numpy's
power (an ulp): 2 p_max 2^-53 for the two together; a few ulps for the base
(the divide by S - 1, the add and the halving of the signed type). The bar
holds only if the oracle starts from the engine's own correlation bits (the
corr that set_dataset_from_data(...).matrices() exports for the same data,
type and cor_type): the kernel's g comes from the same main loop in the same
K order, and where it computes tile (I, J) for I < J the operands of every
product are swapped against the from-data kernel's tile (J, I), which changes
no bit. Checked on the CPU (worst_connectivity_ratio below) against a
long-double evaluation, for the GPU cases' shapes n = 2 .. 193, the three
types, the power sets [1..10, 12..20], [64], [0.5, 2.5, 6] and 32 powers up
to 32: numpy's power summed pairwise and a sequential multiplication chain
summed in a shuffled order both stayed at or below 0.051 of the bar.

FIT, absolute on each of R^2, slope and adjusted R^2: FIT_BAR = 16 times the
worst disagreement between this file's lstsq evaluation and the same fits
from centred normal equations in long double (scale_free_fit with
long_double=True), over the cases of tests/test_sft_host.py (heavy-tailed
n = 500, an empty bin, a zero-mean bin, removeFirst, B = 3 .. 20: worst
2.7e-15) and the GPU end-to-end case (the bundled 150-node test data, the
default powers, the three types, each k from this file's connectivity of
numpy's correlation: worst 9.3e-14): FIT_BAR = 16 x 9.3e-14 = 1.5e-12. Counts, bins, max.k. and median.k.
are compared exactly; mean.k. at (n + 16) 2^-52 relative (summation order).
"""
import numpy as np

NET_TYPES = ("unsigned", "signed", "signed_hybrid")
DEFAULT_POWERS = tuple(range(1, 11)) + tuple(range(12, 21, 2))
COLUMNS = ["Power", "SFT.R.sq", "slope", "truncated.R.sq", "mean.k.", "median.k.", "max.k."]
FIT_BAR = 1.5e-12


def base(corr, net_type):
    c = np.asarray(corr, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        if net_type == "unsigned":
            return np.abs(c)
        if net_type == "signed":
            return (1.0 + c) * 0.5
        if net_type == "signed_hybrid":
            return np.where(c <= 0.0, 0.0, c)   # NaN <= 0 is false: NaN stays
    raise ValueError(net_type)


def connectivity(corr, powers, net_type="unsigned"):
    """(n, P): column m the connectivities for powers[m]."""
    b = base(corr, net_type)
    n = b.shape[0]
    assert b.shape == (n, n)
    out = np.empty((n, len(powers)), order="F")
    off = ~np.eye(n, dtype=bool)
    with np.errstate(invalid="ignore"):
        for m, p in enumerate(powers):
            out[:, m] = np.where(off, b ** float(p), 0.0).sum(axis=0)
    return out


def connectivity_bar(n, powers):
    return (n + 2 * max(powers) + 16) * 2.0 ** -52


def assert_connectivity_close(got, exp, n, powers, what=""):
    """Same NaN pattern; |got - exp| <= bar |exp| per entry (exact where exp
    is 0). Returns the worst relative error."""
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    nan = np.isnan(exp)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg=what)
    bar = connectivity_bar(n, powers)
    err = np.abs(got - exp)[~nan]
    mag = np.abs(exp)[~nan]
    nz = mag > 0
    worst = float((err[nz] / mag[nz]).max()) if nz.any() else 0.0
    print(f"{what}: connectivity relative error {worst:.3e} (bar {bar:.3e})")
    assert (err <= bar * mag).all(), f"{what}: relative error {worst:.3e} above {bar:.3e}"
    return worst


def bins_of(k, n_breaks=10):
    """(bins 1 .. B per node, edges) or (None, None) for a constant or
    non-finite k."""
    k = np.asarray(k, dtype=np.float64)
    if not np.isfinite(k).all():
        return None, None
    mn, mx = k.min(), k.max()
    dx = mx - mn
    if not dx > 0.0:
        return None, None
    edges = mn + np.arange(n_breaks + 1) * (dx / n_breaks)
    bins = 1 + (k[:, None] > edges[None, 1:n_breaks]).sum(axis=1)
    return bins, edges


def _ols(cols, y, long_double):
    """R^2 = 1 - SSR / SST and the coefficients of y ~ 1 + cols."""
    if long_double:   # centred normal equations
        ld = np.longdouble
        y = y.astype(ld)
        c = [v.astype(ld) - v.astype(ld).mean() for v in cols]
        yc = y - y.mean()
        g = np.array([[(a * b).sum() for b in c] for a in c], dtype=ld)
        r = np.array([(a * yc).sum() for a in c], dtype=ld)
        if len(c) == 1:
            coef = [r[0] / g[0, 0]]
        else:
            det = g[0, 0] * g[1, 1] - g[0, 1] * g[0, 1]
            coef = [(r[0] * g[1, 1] - r[1] * g[0, 1]) / det, (r[1] * g[0, 0] - r[0] * g[0, 1]) / det]
        res = yc - sum(b * a for b, a in zip(coef, c))
        return 1 - (res * res).sum() / (yc * yc).sum(), coef
    a = np.column_stack([np.ones(y.size)] + list(cols))
    coef = np.linalg.lstsq(a, y, rcond=None)[0]
    res = y - a @ coef
    return 1.0 - (res ** 2).sum() / ((y - y.mean()) ** 2).sum(), coef[1:]


def scale_free_fit(k, n_breaks=10, remove_first=False, long_double=False):
    """{"rsq", "slope", "trunc", "bins", "counts"}."""
    k = np.asarray(k, dtype=np.float64)
    bins, edges = bins_of(k, n_breaks)
    if bins is None:
        return {"rsq": np.nan, "slope": np.nan, "trunc": np.nan, "bins": None, "counts": None}
    counts = np.bincount(bins, minlength=n_breaks + 1)[1:]
    sums = np.bincount(bins, weights=k, minlength=n_breaks + 1)[1:]
    with np.errstate(invalid="ignore", divide="ignore"):
        d = sums / counts
    d = np.where((counts == 0) | (d == 0.0), (edges[:-1] + edges[1:]) / 2.0, d)
    x, y = np.log10(d), np.log10(counts / k.size + 1e-9)
    if remove_first:
        x, y, d = x[1:], y[1:], d[1:]
    with np.errstate(invalid="ignore", divide="ignore"):
        r1, c1 = _ols([x], y, long_double)
        trunc = np.nan
        if x.size > 3:
            r2, _ = _ols([x, d], y, long_double)
            trunc = 1 - (1 - r2) * (x.size - 1) / (x.size - 3)
    return {"rsq": float(r1), "slope": float(c1[0]), "trunc": float(trunc), "bins": bins, "counts": counts}


def power_estimate(powers, rsq, slope, cut=0.85):
    """The first power with -sign(slope) rsq > cut, or None."""
    for p, r, s in zip(powers, rsq, slope):
        if -np.sign(s) * r > cut:   # False for NaN
            return float(p)
    return None


def pick(corr, powers=DEFAULT_POWERS, net_type="unsigned", cut=0.85, n_breaks=10, remove_first=False):
    """{"powerEstimate", "fitIndices": {column: array}, "connectivity"} from a
    correlation matrix."""
    k = connectivity(corr, powers, net_type)
    n = k.shape[0]
    fits = [scale_free_fit(k[:, m], n_breaks, remove_first) for m in range(len(powers))]
    table = {"Power": np.array(powers, dtype=np.float64),
             "SFT.R.sq": np.array([f["rsq"] for f in fits]),
             "slope": np.array([f["slope"] for f in fits]),
             "truncated.R.sq": np.array([f["trunc"] for f in fits]),
             "mean.k.": k.sum(axis=0) / n,
             "median.k.": np.median(k, axis=0),
             "max.k.": k.max(axis=0)}
    return {"powerEstimate": power_estimate(powers, table["SFT.R.sq"], table["slope"], cut), "fitIndices": table,
            "connectivity": k}


def worst_connectivity_ratio(shapes=(2, 15, 17, 63, 64, 65, 129, 193), seed=0):
    """The CPU check of the connectivity bar quoted above: the worst
    (relative error / bar) of two fp64 evaluations -- numpy's power summed by
    numpy, and a sequential multiplication chain (integer powers) summed in a
    shuffled order -- against long double."""
    rng = np.random.default_rng(seed)
    sets = [list(DEFAULT_POWERS), [64], [0.5, 2.5, 6.0], list(range(1, 33))]
    worst = 0.0
    for n in shapes:
        x = rng.normal(size=(n + 3, n))
        x = (x - x.mean(axis=0)) / x.std(axis=0, ddof=1)
        c = np.clip(x.T @ x / (n + 2), -1.0, 1.0)
        for net_type in NET_TYPES:
            b = base(c, net_type)
            np.fill_diagonal(b, 0.0)
            bl = b.astype(np.longdouble)
            for powers in sets:
                got = connectivity(c, powers, net_type)
                for m, p in enumerate(powers):
                    exact = (bl ** np.longdouble(p)).sum(axis=0)
                    cands = [got[:, m]]
                    if float(p).is_integer():
                        v = b.copy()
                        for _ in range(int(p) - 1):
                            v = v * b
                        t = np.zeros(n)
                        for u in rng.permutation(n):
                            t = t + v[u]
                        cands.append(t)
                    for cand in cands:
                        nz = exact > 0
                        if nz.any():
                            rel = np.abs(cand.astype(np.longdouble) - exact)[nz] / exact[nz]
                            worst = max(worst, float(rel.max()) / connectivity_bar(n, powers))
    return worst
