"""numpy restatement of the from-data path (nr_set_dataset_from_data): the
correlation and network a NetRep user derives from the data matrix
(R/example-data.R:111-116: cor(data), abs(correlation)^5), as the test oracle.

    x^ = (x - mean) / sd(ddof = 1)          per column (Scale, src/scale.cpp:14-25)
    c  = clip(x^T x^ / (S - 1), -1, 1)      R's cor clamps
    w  = |c|^beta                           unsigned
         ((1 + c) / 2)^beta                 signed
         c^beta where c > 0, else 0         signed_hybrid
NaN propagates through every step (a constant column has sd 0: its row and
column of c and w are NaN, where R's cor gives NA).
"""
import numpy as np

NET_TYPES = ("unsigned", "signed", "signed_hybrid")


def scale(x):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (x - x.mean(axis=0)) / x.std(axis=0, ddof=1)


def correlation(xs):
    """xs: the scaled data (S x n)."""
    xs = np.asarray(xs, dtype=np.float64)
    return np.clip(xs.T @ xs / (xs.shape[0] - 1), -1.0, 1.0)


def network(c, beta, net_type="unsigned"):
    with np.errstate(invalid="ignore"):
        if net_type == "unsigned":
            return np.abs(c) ** beta
        if net_type == "signed":
            return ((1.0 + c) / 2.0) ** beta
        if net_type == "signed_hybrid":
            return np.where(c <= 0.0, 0.0, np.abs(c) ** beta)  # NaN <= 0 is false: NaN stays
    raise ValueError(net_type)


def build(data, beta, net_type="unsigned", do_scale=True):
    """(corr, net) of a data matrix (S x n)."""
    xs = scale(data) if do_scale else np.asarray(data, dtype=np.float64)
    c = correlation(xs)
    return c, network(c, beta, net_type)


def corr_bar(n_samples):
    """Summation-order rounding over S terms plus the scaling's few ulps."""
    return (n_samples + 16) * 2.0 ** -52


def net_bar(n_samples, beta):
    """The transforms have slope <= beta on [-1, 1] for beta >= 1; pow adds ~2 ulp."""
    assert beta >= 1
    return beta * corr_bar(n_samples) + 1e-15
