"""The from-data path on the GPU (nr_set_dataset_from_data, netbuild.hip): the
{corr, net} pair array built from the data matrix alone, against the
reference's recorded matrices and the numpy restatement (tests/netbuild_ref.py),
and everything downstream of it against the host-matrix path, bitwise.

Bars (netbuild_ref): corr (S + 16) 2^-52 -- summation-order rounding over S
terms plus the scaling's few ulps; net beta * corr bar + 1e-15 -- the
transforms' slope is <= beta on [-1, 1] for beta >= 1, pow adds ~2 ulp."""
import os
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

import netrep_amd as N
from netrep_amd import _lib as L
from netrep_amd.api import RMatrix

import netbuild_ref as R
from conftest import assert_stats_close
from test_gpu_dual import _case
from test_gpu_parity import _engine_from

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

T = N.Engine.NETBUILD_TILE
MODULES = ["1", "2", "3", "4"]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _check_against(eng, c_exp, w_exp, s, beta, what):
    c, w = eng.matrices()
    ce, we = np.abs(c - c_exp).max(), np.abs(w - w_exp).max()
    print(f"{what}: corr error {ce:.3e} (bar {R.corr_bar(s):.3e}), net error {we:.3e} (bar {R.net_bar(s, beta):.3e})")
    assert ce <= R.corr_bar(s), what
    assert we <= R.net_bar(s, beta), what
    np.testing.assert_array_equal(_bits(c), _bits(c.T))
    np.testing.assert_array_equal(_bits(w), _bits(w.T))
    assert eng.symmetric()
    assert eng.finite() == (True, True)
    return c, w


def test_reference_fixture(bundled):
    """test_data (30 x 150), beta 5, unsigned: the reference's own
    test_correlation / test_network within the bars."""
    with N.Engine(0) as eng:
        eng.set_dataset_from_data(bundled["test_data"], 5.0, "unsigned", scale=True)
        assert eng.shape() == (150, 30)
        _check_against(eng, bundled["test_correlation"], bundled["test_network"], 30, 5.0, "fixture")
        assert eng.netbuild_ms() > 0.0
        assert not eng.gram_table()


# n: below one MFMA tile (1, 15), just past it (17), around the workgroup tile
# (63, 65), three tile rows with a ragged edge (129) and four (3 T + 1:
# interior off-diagonal tiles). S: below one MFMA K-step (2, 3), not a multiple
# of 4 (5, 17, 61, 130), none a multiple of the 32-sample chunk (61 and 130
# span several chunks).
EDGE_CASES = [
    (1, 2, "unsigned", 1.0), (1, 17, "signed", 5.0), (15, 3, "signed", 5.0), (15, 61, "signed_hybrid", 6.5),
    (17, 5, "unsigned", 6.5), (17, 130, "signed_hybrid", 1.0), (63, 17, "signed_hybrid", 5.0),
    (63, 2, "signed", 6.5), (65, 61, "unsigned", 5.0), (65, 3, "signed_hybrid", 5.0),
    (129, 130, "signed", 1.0), (129, 5, "unsigned", 5.0), (3 * T + 1, 61, "signed", 6.5),
    (3 * T + 1, 17, "unsigned", 5.0),
]


@pytest.mark.parametrize("n,s,net_type,beta", EDGE_CASES)
def test_tile_and_k_edges(n, s, net_type, beta):
    x = np.random.default_rng(1000 * n + s).normal(size=(s, n))
    c_exp, w_exp = R.build(x, beta, net_type)
    with N.Engine(0) as eng:
        eng.set_dataset_from_data(x, beta, net_type, scale=True)
        _check_against(eng, c_exp, w_exp, s, beta, f"n={n} S={s} {net_type} beta={beta}")


@pytest.mark.parametrize("n,s,net_type,beta", [(65, 61, "signed", 5.0), (3 * T + 1, 5, "signed_hybrid", 6.5)])
def test_prescaled_data(n, s, net_type, beta):
    xs = R.scale(np.random.default_rng(7 * n + s).normal(size=(s, n)))
    c_exp, w_exp = R.build(xs, beta, net_type, do_scale=False)
    with N.Engine(0) as eng:
        eng.set_dataset_from_data(xs, beta, net_type, scale=False)
        _check_against(eng, c_exp, w_exp, s, beta, f"pre-scaled n={n} S={s}")


def _set_modules(eng, mi, disc):
    mods = mi.mods_present
    node_off = np.concatenate([[0], np.cumsum([mi.test_idx[m].size for m in mods])])
    eng.set_modules(len(mi.modules), [mi.modules.index(m) for m in mods], node_off,
                    np.concatenate([mi.test_idx[m] for m in mods]), np.concatenate([mi.null_pos[m] for m in mods]),
                    np.concatenate([disc["corr"][m] for m in mods]), np.concatenate([disc["degree"][m] for m in mods]),
                    np.concatenate([disc["contribution"][m] for m in mods]))
    eng.set_null_pool(mi.null_idx)


@pytest.mark.parametrize("sizes,s,n,table", [([40, 20, 7], 30, 150, False), ([130, 120], 140, 400, True)])
def test_downstream_bitwise_equal_to_host_matrix_path(sizes, s, n, table):
    """Build from data, export, feed the export and the scaled block to a
    second engine through set_dataset: observed() and run() bitwise equal."""
    lay, mi, disc, txs, _tc, _tn = _case(sizes, s, 31, n_nodes=n)
    a = N.Engine(0)
    try:
        a.set_dataset_from_data(txs, 5.0, "unsigned", scale=False)
        c, w = a.matrices()
        _set_modules(a, mi, disc)
        b = _engine_from(mi, disc, txs, c, w)
        try:
            assert b.symmetric() and b.finite() == (True, True)
            np.testing.assert_array_equal(_bits(a.observed()), _bits(b.observed()))
            np.testing.assert_array_equal(_bits(a.run(0, 8, 77)), _bits(b.run(0, 8, 77)))
            assert a.gram_table() == b.gram_table() == table
            # the export reads either layout
            for eng in (a, b):
                c2, w2 = eng.matrices()
                np.testing.assert_array_equal(_bits(c2), _bits(c))
                np.testing.assert_array_equal(_bits(w2), _bits(w))
        finally:
            b.close()
    finally:
        a.close()


def _bundled_call(b, e, data=None, **kw):
    ma = dict(zip(b["module_labels_names"].tolist(), b["module_labels"].tolist()))
    t_names = b["test_network_colnames"].tolist()
    disc = {key: {m: e[f"disc_{key}_{m}_data"] for m in MODULES} for key in ("degree", "corr", "contribution")}
    t_data = RMatrix(b["test_data"] if data is None else data, None, t_names)
    return N.PermutationProcedureFromData(disc, t_data, 5.0, ma, MODULES, e["pis"].shape[0], pi=e["pis"],
                                          networkType="unsigned", scaleData=True, **kw)


def test_reference_interface_on_bundled_data(bundled, bundled_expected):
    r = _bundled_call(bundled, bundled_expected)
    eo = assert_stats_close(r["observed"], bundled_expected["observed_data"], what="observed (from data)")
    en = assert_stats_close(r["nulls"], bundled_expected["nulls_data"], what="nulls (from data)")
    print(f"from-data bundled: observed {eo:.3e}, nulls {en:.3e}")


def test_constant_column(bundled, bundled_expected):
    x = bundled["test_data"].copy()
    x[:, 37] = 2.5
    with N.Engine(0) as eng:
        eng.set_dataset_from_data(x, 5.0)
        assert eng.finite() == (False, False)
        assert eng.symmetric()
    with pytest.raises(N.NetRepError) as ei:
        _bundled_call(bundled, bundled_expected, data=x)
    assert ei.value.code == L.NR_ERR_NONFINITE
    assert "non-finite" in str(ei.value)
    names = bundled["test_network_colnames"].tolist()
    corr, net = N.BuildNetwork(RMatrix(x, None, names), 5.0)
    bad = np.zeros((150, 150), bool)
    bad[37, :] = bad[:, 37] = True
    np.testing.assert_array_equal(np.isnan(corr.values), bad)
    np.testing.assert_array_equal(np.isnan(net.values), bad)
    assert list(net.colnames) == names
    c_exp, w_exp = R.build(x, 5.0)
    assert np.abs(corr.values - c_exp)[~bad].max() <= R.corr_bar(30)
    assert np.abs(net.values - w_exp)[~bad].max() <= R.net_bar(30, 5.0)


def test_only_the_data_crosses_pcie():
    n, s = 600, 40
    x = np.random.default_rng(5).normal(size=(s, n))
    with N.Engine(0) as eng:
        before = N.h2d_bytes()
        eng.set_dataset_from_data(x, 5.0)
        delta = N.h2d_bytes() - before
        eng.matrices()                                   # device -> host: not counted
        assert N.h2d_bytes() - before == delta
    print(f"h2d bytes of the from-data set-up: {delta} (host-matrix path: {16 * n * n} + data)")
    assert 8 * s * n <= delta <= 2 * 8 * s * (n + 2) + (1 << 20) < 16 * n * n


def test_engine_rejects_invalid_arguments():
    x = np.random.default_rng(2).normal(size=(6, 4))
    with N.Engine(0) as eng:
        for kw in (dict(beta=0.0), dict(beta=-1.0), dict(beta=float("nan")), dict(beta=float("inf"))):
            with pytest.raises(N.NetRepError) as ei:
                eng.set_dataset_from_data(x, **kw)
            assert ei.value.code == L.NR_ERR_INVALID and "beta" in str(ei.value)
        with pytest.raises(N.NetRepError) as ei:
            eng.set_dataset_from_data(x[:1], 5.0)
        assert ei.value.code == L.NR_ERR_INVALID
        with pytest.raises(N.NetRepError):
            eng.matrices()                                # no dataset
        assert eng.shape() == (0, 0)


def _sharded_child(_rank, out):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    with np.load(os.path.join(ROOT, "tests", "golden", "netrep_bundled.npz")) as f:
        b = {k: f[k] for k in f.files}
    with np.load(os.path.join(ROOT, "tests", "golden", "bundled_expected.npz")) as f:
        e = {k: f[k] for k in f.files}
    one = _bundled_call(b, e)
    os.environ.update(NETREP_NUM_GPUS="2", NETREP_SHARE_DEVICE="1")
    two = _bundled_call(b, e)
    np.savez(out, one_nulls=one["nulls"], two_nulls=two["nulls"], one_obs=one["observed"], two_obs=two["observed"])


def test_sharded_path_bitwise_equal(tmp_path):
    """NETREP_NUM_GPUS=2 NETREP_SHARE_DEVICE=1: the dataset built in context 0
    is broadcast device to device, each context runs its chunk; the cube is
    bitwise the one-context cube (in a fresh child process, as
    tests/test_gpu_distributed.py runs its ranks)."""
    out = str(tmp_path / "cubes.npz")
    mp.spawn(_sharded_child, args=(out,), nprocs=1, join=True)
    with np.load(out) as f:
        assert f["one_nulls"].shape == (4, 7, 16) and np.isfinite(f["one_nulls"]).any()
        np.testing.assert_array_equal(_bits(f["one_nulls"]), _bits(f["two_nulls"]))
        np.testing.assert_array_equal(_bits(f["one_obs"]), _bits(f["two_obs"]))
