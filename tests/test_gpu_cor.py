"""The correlation types of the from-data path on the GPU (NR_COR_SPEARMAN,
NR_COR_BICOR; cortransform.hip): corr and net against the numpy oracle
(tests/cor_ref.py) within its bars, the rank kernel's exactness bitwise against
the Pearson path run on the oracle's ranks, and everything downstream against
the host-matrix path, bitwise.

Bars (cor_ref): Spearman netbuild_ref.corr_bar(S) -- exact ranks, then the
Pearson pipeline; bicor (S + 64) 2^-52 absolute on corr; net: beta times the
corr bar + 1e-15."""
import numpy as np
import pytest

import netrep_amd as N
from netrep_amd import _lib as L
from netrep_amd.api import RMatrix

import cor_ref as CR
import netbuild_ref as R
import tom_ref as TR
from conftest import assert_stats_close
from test_gpu_dual import _case
from test_gpu_netbuild import MODULES, _bits, _bundled_call, _set_modules
from test_gpu_parity import _engine_from

pytestmark = pytest.mark.gpu

LDS = N.Engine.COR_LDS_ROWS

KINDS = ("normal", "halves", "student-t")


def _data(kind, s, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "normal":
        return rng.normal(size=(s, n))
    if kind == "halves":                     # heavy ties; at small S, mad == 0 and constant columns
        return np.round(rng.normal(size=(s, n)) * 2.0) / 2.0
    return rng.standard_t(1.5, size=(s, n))  # outliers past |u| = 1


def _check(eng, x, beta, net_type, cor_type, scale, what):
    s = x.shape[0]
    c_exp, w_exp = CR.build(x, beta, net_type, cor_type, do_scale=scale)
    eng.set_dataset_from_data(x, beta, net_type, scale=scale, cor_type=cor_type)
    c, w = eng.matrices()
    nan_c, nan_w = np.isnan(c_exp), np.isnan(w_exp)
    np.testing.assert_array_equal(np.isnan(c), nan_c, err_msg=what)
    np.testing.assert_array_equal(np.isnan(w), nan_w, err_msg=what)
    ce = np.abs(c - c_exp)[~nan_c].max(initial=0.0)
    we = np.abs(w - w_exp)[~nan_w].max(initial=0.0)
    cb, wb = CR.corr_bar(s, cor_type), CR.net_bar(s, beta, cor_type)
    print(f"{what}: corr error {ce:.3e} (bar {cb:.3e}), net error {we:.3e} (bar {wb:.3e}), "
          f"NaN columns {int(nan_c.all(axis=0).sum())}")
    assert ce <= cb, what
    assert we <= wb, what
    np.testing.assert_array_equal(_bits(c), _bits(c.T))
    np.testing.assert_array_equal(_bits(w), _bits(w.T))
    assert eng.symmetric()
    assert eng.finite() == (not nan_c.any(), not nan_w.any()), what
    assert eng.cor_ms() > 0.0
    assert eng.netbuild_ms() > 0.0
    return c, w


# S: the minimum (2), odd and even medians (3, 4, 5), one row below, at and
# above a wave (63, 64, 65) and a workgroup (255, 256, 257), several rows per
# thread and sweep (500, 1025: the second in the workgroup-per-column shape),
# and both sides of the global-memory instantiation. n: 1, below, across and
# beyond the four columns of a workgroup and the 64-tile.
EDGE_SHAPES = [(2, 3), (3, 5), (4, 1), (5, 17), (63, 9), (64, 9), (65, 9), (255, 5), (256, 5), (257, 5), (500, 65),
               (1025, 4), (LDS, 3), (LDS + 1, 3)]
NETS = [("unsigned", 5.0), ("signed", 5.0), ("signed_hybrid", 6.5), ("unsigned", 1.0)]


@pytest.mark.parametrize("cor_type", CR.COR_TYPES)
@pytest.mark.parametrize("s,n", EDGE_SHAPES)
def test_edges_against_the_oracle(s, n, cor_type):
    with N.Engine(0) as eng:
        for k, kind in enumerate(KINDS):
            net_type, beta = NETS[(EDGE_SHAPES.index((s, n)) + k) % len(NETS)]
            x = _data(kind, s, n, 14 + 1000 * s + n + k)
            c, _w = _check(eng, x, beta, net_type, cor_type, True,
                           f"{cor_type} S={s} n={n} {kind} {net_type} beta={beta}")
            # the tied small-S cases are what they say: constant columns (NaN in
            # both oracle and engine), and non-constant columns with mad == 0
            if kind == "halves" and s in (2, 3):
                assert 1 <= np.isnan(c).all(axis=0).sum() < n
            if kind == "halves" and (s, n) == (5, 17):
                xs = R.scale(x)
                assert sum(CR.bicor_column(xs[:, j])[1] == 0.0 for j in range(n)) >= 1


@pytest.mark.parametrize("cor_type", CR.COR_TYPES)
@pytest.mark.parametrize("s,n", [(65, 9), (500, 65)])
def test_prescaled_data(s, n, cor_type):
    with N.Engine(0) as eng:
        for k, kind in enumerate(KINDS):
            x = _data(kind, s, n, 7 * s + n + k)
            c1, w1 = _check(eng, x, 5.0, "signed", cor_type, True, f"{cor_type} S={s} n={n} {kind} raw")
            c2, w2 = _check(eng, R.scale(x), 5.0, "signed", cor_type, False, f"{cor_type} S={s} n={n} {kind} pre-scaled")
            assert np.abs(c1 - c2).max() <= 2 * CR.corr_bar(s, cor_type)


@pytest.mark.parametrize("s,n,kind", [(5, 17, "halves"), (65, 9, "normal"), (257, 5, "halves"), (500, 65, "student-t"),
                                      (LDS + 1, 3, "halves")])
def test_spearman_is_bitwise_pearson_of_the_ranks(s, n, kind):
    """The exactness test of the counting kernel: from the same pre-scaled
    block, Spearman and Pearson-of-the-oracle's-ranks share every bit (both
    scale the ranks with the same kernel)."""
    xs = R.scale(_data(kind, s, n, 31 * s + n))
    with N.Engine(0) as a, N.Engine(0) as b:
        a.set_dataset_from_data(xs, 5.0, "unsigned", scale=False, cor_type="spearman")
        b.set_dataset_from_data(CR.ranks(xs), 5.0, "unsigned", scale=True, cor_type="pearson")
        (ca, wa), (cb, wb) = a.matrices(), b.matrices()
        assert np.isfinite(ca).any()
        np.testing.assert_array_equal(_bits(ca), _bits(cb))
        np.testing.assert_array_equal(_bits(wa), _bits(wb))
        assert a.cor_ms() > 0.0 and b.cor_ms() == 0.0


def test_pearson_untouched():
    x = _data("normal", 61, 130, 4)
    with N.Engine(0) as a, N.Engine(0) as b:
        a.set_dataset_from_data(x, 5.0, "signed_hybrid")
        b.set_dataset_from_data(x, 5.0, "signed_hybrid", cor_type="pearson")
        for m0, m1 in zip(a.matrices(), b.matrices()):
            np.testing.assert_array_equal(_bits(m0), _bits(m1))
        assert a.cor_ms() == 0.0 and b.cor_ms() == 0.0
        b.set_dataset_from_data(x, 5.0, "signed_hybrid", cor_type="bicor")
        assert b.cor_ms() > 0.0
        b.set_dataset_from_data(x, 5.0, "signed_hybrid")
        assert b.cor_ms() == 0.0


@pytest.mark.parametrize("cor_type", CR.COR_TYPES)
def test_nan_takes_its_column_only(cor_type):
    s, n, j = 40, 7, 2
    xs = R.scale(_data("normal", s, n, 12))
    bad = xs.copy()
    bad[3, j] = np.nan
    with N.Engine(0) as eng:
        eng.set_dataset_from_data(xs, 5.0, scale=False, cor_type=cor_type)
        c0, w0 = eng.matrices()
        assert eng.finite() == (True, True)
        eng.set_dataset_from_data(bad, 5.0, scale=False, cor_type=cor_type)
        c1, w1 = eng.matrices()
        assert eng.finite() == (False, False)
    cross = np.zeros((n, n), bool)
    cross[j, :] = cross[:, j] = True
    for m0, m1 in ((c0, c1), (w0, w1)):
        np.testing.assert_array_equal(np.isnan(m1), cross)
        np.testing.assert_array_equal(_bits(m1[~cross]), _bits(m0[~cross]))


def test_inf_is_ranked_by_spearman_and_takes_the_column_for_bicor():
    s, n, j = 40, 7, 4
    xs = R.scale(_data("normal", s, n, 13))
    xs[5, j] = np.inf
    xs[9, j] = -np.inf
    with N.Engine(0) as eng:
        c, _w = _check(eng, xs, 5.0, "unsigned", "spearman", False, "spearman with +-Inf")
        assert np.isfinite(c).all()
        c, _w = _check(eng, xs, 5.0, "unsigned", "bicor", False, "bicor with +-Inf")
    cross = np.zeros((n, n), bool)
    cross[j, :] = cross[:, j] = True
    np.testing.assert_array_equal(np.isnan(c), cross)


@pytest.mark.parametrize("cor_type", CR.COR_TYPES)
def test_constant_column(bundled, bundled_expected, cor_type):
    x = bundled["test_data"].copy()
    x[:, 37] = 2.5
    with N.Engine(0) as eng:
        eng.set_dataset_from_data(x, 5.0, cor_type=cor_type)
        assert eng.finite() == (False, False)
        assert eng.symmetric()
    with pytest.raises(N.NetRepError) as ei:
        _bundled_call(bundled, bundled_expected, data=x, corType=cor_type)
    assert ei.value.code == L.NR_ERR_NONFINITE


@pytest.mark.parametrize("cor_type,net_type", [("spearman", "signed"), ("bicor", "unsigned")])
def test_with_the_tom(cor_type, net_type):
    n, s = 2 * N.Engine.NETBUILD_TILE + 1, 61
    x = _data("student-t", s, n, 21)
    with N.Engine(0) as eng:
        eng.set_dataset_from_data(x, 5.0, net_type, cor_type=cor_type)
        c0, w0 = eng.matrices()
        assert eng.tom_ms() == 0.0 and eng.cor_ms() > 0.0
        eng.set_dataset_from_data(x, 5.0, net_type, tom=True, cor_type=cor_type)
        c1, t = eng.matrices()
        np.testing.assert_array_equal(_bits(c1), _bits(c0))
        TR.assert_tom_close(t, TR.tom(w0), n, f"{cor_type} with the TOM")
        np.testing.assert_array_equal(_bits(t), _bits(t.T))
        assert eng.tom_ms() > 0.0 and eng.cor_ms() > 0.0 and eng.netbuild_ms() > 0.0
        assert eng.finite() == (True, True)


@pytest.mark.parametrize("cor_type", CR.COR_TYPES)
@pytest.mark.parametrize("sizes,s,n,table", [([40, 20, 7], 30, 150, False), ([130, 120], 140, 400, True)])
def test_downstream_bitwise_equal_to_host_matrix_path(sizes, s, n, table, cor_type):
    """The data block is still the scaled data: build from data, export, feed
    the export and the scaled block to a second engine through set_dataset;
    observed(), run() and the re-export bitwise equal."""
    lay, mi, disc, txs, _tc, _tn = _case(sizes, s, 31, n_nodes=n)
    a = N.Engine(0)
    try:
        a.set_dataset_from_data(txs, 5.0, "unsigned", scale=False, cor_type=cor_type)
        c, w = a.matrices()
        c_exp, _w = CR.build(txs, 5.0, "unsigned", cor_type, do_scale=False)
        assert np.abs(c - c_exp).max() <= CR.corr_bar(s, cor_type)
        assert a.cor_ms() > 0.0
        _set_modules(a, mi, disc)
        b = _engine_from(mi, disc, txs, c, w)
        try:
            assert b.symmetric() and b.finite() == (True, True)
            assert b.cor_ms() == 0.0
            np.testing.assert_array_equal(_bits(a.observed()), _bits(b.observed()))
            np.testing.assert_array_equal(_bits(a.run(0, 8, 77)), _bits(b.run(0, 8, 77)))
            assert a.gram_table() == b.gram_table() == table
            for eng in (a, b):
                c2, w2 = eng.matrices()
                np.testing.assert_array_equal(_bits(c2), _bits(c))
                np.testing.assert_array_equal(_bits(w2), _bits(w))
        finally:
            b.close()
    finally:
        a.close()


@pytest.mark.parametrize("cor_type", CR.COR_TYPES)
def test_reference_interface_on_bundled_data(bundled, bundled_expected, cor_type):
    """PermutationProcedureFromData(corType=...) against PermutationProcedure
    on host matrices that BuildNetwork(corType=...) exported."""
    b, e = bundled, bundled_expected
    names = b["test_network_colnames"].tolist()
    raw = RMatrix(b["test_data"], None, names)
    corr, net = N.BuildNetwork(raw, 5.0, corType=cor_type)
    c_exp, w_exp = CR.build(b["test_data"], 5.0, "unsigned", cor_type)
    assert np.abs(corr.values - c_exp).max() <= CR.corr_bar(30, cor_type)
    assert np.abs(net.values - w_exp).max() <= CR.net_bar(30, 5.0, cor_type)
    assert list(corr.colnames) == names and list(net.colnames) == names

    got = _bundled_call(b, e, corType=cor_type)
    ma = dict(zip(b["module_labels_names"].tolist(), b["module_labels"].tolist()))
    disc = {key: {m: e[f"disc_{key}_{m}_data"] for m in MODULES} for key in ("degree", "corr", "contribution")}
    exp = N.PermutationProcedure(disc, N.Scale(raw), corr, net, ma, MODULES, e["pis"].shape[0], pi=e["pis"])
    eo = assert_stats_close(got["observed"], exp["observed"], what=f"observed ({cor_type} from data)")
    en = assert_stats_close(got["nulls"], exp["nulls"], what=f"nulls ({cor_type} from data)")
    print(f"{cor_type} from-data bundled: observed {eo:.3e}, nulls {en:.3e}")
    # and the correlation is not Pearson's: the network statistics moved
    plain = _bundled_call(b, e)
    assert not np.array_equal(plain["observed"], got["observed"])


def test_copy_reports_its_sources_cor_ms():
    x = _data("normal", 12, 70, 9)
    with N.Engine(0) as src, N.Engine(0) as dst:
        src.set_dataset_from_data(x, 5.0, cor_type="bicor")
        dst.copy_dataset_from(src)
        assert dst.cor_ms() == src.cor_ms() > 0.0
        np.testing.assert_array_equal(_bits(dst.matrices()[0]), _bits(src.matrices()[0]))
