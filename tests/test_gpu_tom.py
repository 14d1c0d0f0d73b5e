"""The topological-overlap option of the from-data path on the GPU
(NR_NET_TOM, netbuild.hip's tom_extract_kernel and tom_kernel): the resident
network as the TOM of the adjacency the same call builds, against the numpy
oracle (tests/tom_ref.py) started from the engine's own adjacency bits, and
everything downstream of it against the host-matrix path, bitwise.

Bar (tom_ref): (n + 16) 2^-52 relative per element -- summation-order rounding
of the two sums of n non-negative terms, a few ulps for the add, the subtract
and the divide; exact where the expected value is 0."""
import os
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

import netrep_amd as N
from netrep_amd import _lib as L
from netrep_amd.api import RMatrix

import netbuild_ref as R
import tom_ref as TR
from conftest import assert_stats_close
from test_gpu_dual import _case
from test_gpu_netbuild import MODULES, _bits, _bundled_call, _set_modules
from test_gpu_parity import _engine_from

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

T = N.Engine.NETBUILD_TILE   # the TOM kernel's tile too (tests/test_tom_host.py pins it)


def _check_tom(x, beta, net_type, scale, what):
    """Build twice in one engine, without and with the TOM; the oracle starts
    from the first build's adjacency bits."""
    n = x.shape[1]
    with N.Engine(0) as eng:
        eng.set_dataset_from_data(x, beta, net_type, scale=scale, tom=False)
        c0, w0 = eng.matrices()
        assert eng.tom_ms() == 0.0
        eng.set_dataset_from_data(x, beta, net_type, scale=scale, tom=True)
        c1, t = eng.matrices()
        np.testing.assert_array_equal(_bits(c1), _bits(c0))
        TR.assert_tom_close(t, TR.tom(w0), n, what)
        np.testing.assert_array_equal(_bits(t), _bits(t.T))
        np.testing.assert_array_equal(np.diag(t), np.ones(n))
        assert eng.symmetric()
        assert eng.finite() == (True, True)
        assert eng.tom_ms() > 0.0
        assert eng.netbuild_ms() > 0.0
    return w0, t


# K = n here, so n carries the tile edges and the chunk edges (32 rows of A per
# chunk): below one MFMA tile with only a partial chunk (1, 2, 15), just past
# one (17), exactly one whole chunk and no partial (32), around the workgroup
# tile (63, 64: whole chunks only, 65), three whole chunks (96), three tile
# rows with a ragged edge (129), four with interior off-diagonal tiles
# (3 T + 1); the last with few samples and beta 1: many exact-zero adjacencies.
EDGE_CASES = [
    (1, 5, "unsigned", 5.0), (2, 5, "signed", 5.0), (15, 3, "signed_hybrid", 6.5), (17, 5, "unsigned", 1.0),
    (32, 9, "signed", 5.0), (63, 17, "signed_hybrid", 5.0), (64, 7, "unsigned", 5.0), (65, 61, "unsigned", 5.0),
    (96, 5, "signed", 1.0), (129, 17, "signed_hybrid", 6.5), (3 * T + 1, 61, "signed", 6.5),
    (3 * T + 1, 8, "signed_hybrid", 1.0),
]


@pytest.mark.parametrize("n,s,net_type,beta", EDGE_CASES)
def test_tile_and_k_edges(n, s, net_type, beta):
    x = np.random.default_rng(1000 * n + s).normal(size=(s, n))
    w0, _t = _check_tom(x, beta, net_type, True, f"n={n} S={s} {net_type} beta={beta}")
    if (n, s) == (3 * T + 1, 8):
        assert (w0 == 0.0).mean() > 0.25   # the case is what it says


@pytest.mark.parametrize("n,s,net_type,beta", [(65, 61, "signed", 5.0), (3 * T + 1, 5, "signed_hybrid", 6.5)])
def test_prescaled_data(n, s, net_type, beta):
    xs = R.scale(np.random.default_rng(7 * n + s).normal(size=(s, n)))
    _check_tom(xs, beta, net_type, False, f"pre-scaled n={n} S={s}")


def test_constant_column(bundled, bundled_expected):
    x = bundled["test_data"].copy()
    x[:, 37] = 2.5
    with N.Engine(0) as eng:
        eng.set_dataset_from_data(x, 5.0, tom=True)
        assert eng.finite() == (False, False)
        assert eng.symmetric()
        corr, net = eng.matrices()
    bad = np.zeros((150, 150), bool)
    bad[37, :] = bad[:, 37] = True
    np.testing.assert_array_equal(np.isnan(corr), bad)
    np.testing.assert_array_equal(np.isnan(net), ~np.eye(150, dtype=bool))
    np.testing.assert_array_equal(np.diag(net), np.ones(150))
    with pytest.raises(N.NetRepError) as ei:
        _bundled_call(bundled, bundled_expected, data=x, tom=True)
    assert ei.value.code == L.NR_ERR_NONFINITE


@pytest.mark.parametrize("sizes,s,n,table", [([40, 20, 7], 30, 150, False), ([130, 120], 140, 400, True)])
def test_downstream_bitwise_equal_to_host_matrix_path(sizes, s, n, table):
    """Build with the TOM, export, feed the export and the scaled block to a
    second engine through set_dataset: observed(), run() and the re-export
    (either pair layout) bitwise equal."""
    lay, mi, disc, txs, _tc, _tn = _case(sizes, s, 31, n_nodes=n)
    a = N.Engine(0)
    try:
        a.set_dataset_from_data(txs, 5.0, "unsigned", scale=False, tom=True)
        c, t = a.matrices()
        assert a.tom_ms() > 0.0
        _set_modules(a, mi, disc)
        b = _engine_from(mi, disc, txs, c, t)
        try:
            assert b.symmetric() and b.finite() == (True, True)
            assert b.tom_ms() == 0.0
            np.testing.assert_array_equal(_bits(a.observed()), _bits(b.observed()))
            np.testing.assert_array_equal(_bits(a.run(0, 8, 77)), _bits(b.run(0, 8, 77)))
            assert a.gram_table() == b.gram_table() == table
            for eng in (a, b):
                c2, t2 = eng.matrices()
                np.testing.assert_array_equal(_bits(c2), _bits(c))
                np.testing.assert_array_equal(_bits(t2), _bits(t))
        finally:
            b.close()
    finally:
        a.close()


def test_reference_interface_on_bundled_data(bundled, bundled_expected):
    """PermutationProcedureFromData(tom=True) against PermutationProcedure on
    host matrices that BuildNetwork(tom=True) exported."""
    b, e = bundled, bundled_expected
    names = b["test_network_colnames"].tolist()
    raw = RMatrix(b["test_data"], None, names)
    corr, net = N.BuildNetwork(raw, 5.0, tom=True)
    _c0, adj = N.BuildNetwork(raw, 5.0, tom=False)
    np.testing.assert_array_equal(_bits(corr.values), _bits(_c0.values))
    TR.assert_tom_close(net.values, TR.tom(adj.values), 150, "BuildNetwork(tom=True)")
    assert list(net.colnames) == names

    got = _bundled_call(b, e, tom=True)
    ma = dict(zip(b["module_labels_names"].tolist(), b["module_labels"].tolist()))
    disc = {key: {m: e[f"disc_{key}_{m}_data"] for m in MODULES} for key in ("degree", "corr", "contribution")}
    exp = N.PermutationProcedure(disc, N.Scale(raw), corr, net, ma, MODULES, e["pis"].shape[0], pi=e["pis"])
    eo = assert_stats_close(got["observed"], exp["observed"], what="observed (TOM from data)")
    en = assert_stats_close(got["nulls"], exp["nulls"], what="nulls (TOM from data)")
    print(f"TOM from-data bundled: observed {eo:.3e}, nulls {en:.3e}")
    # and the TOM is not the adjacency: the network statistics moved
    plain = _bundled_call(b, e)
    assert not np.array_equal(plain["observed"], got["observed"])


def test_only_the_data_crosses_pcie():
    n, s = 600, 40
    x = np.random.default_rng(5).normal(size=(s, n))
    with N.Engine(0) as eng:
        before = N.h2d_bytes()
        eng.set_dataset_from_data(x, 5.0, tom=True)
        delta = N.h2d_bytes() - before
        assert eng.tom_ms() > 0.0
    print(f"h2d bytes of the from-data set-up with the TOM: {delta} (host-matrix path: {16 * n * n} + data)")
    assert 8 * s * n <= delta <= 2 * 8 * s * (n + 2) + (1 << 20) < 16 * n * n


def test_copy_reports_its_sources_tom_ms():
    x = np.random.default_rng(9).normal(size=(12, 70))
    with N.Engine(0) as src, N.Engine(0) as dst:
        src.set_dataset_from_data(x, 5.0, tom=True)
        dst.copy_dataset_from(src)
        assert dst.tom_ms() == src.tom_ms() > 0.0
        np.testing.assert_array_equal(_bits(dst.matrices()[1]), _bits(src.matrices()[1]))


def _sharded_child(_rank, out):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    with np.load(os.path.join(ROOT, "tests", "golden", "netrep_bundled.npz")) as f:
        b = {k: f[k] for k in f.files}
    with np.load(os.path.join(ROOT, "tests", "golden", "bundled_expected.npz")) as f:
        e = {k: f[k] for k in f.files}
    one = _bundled_call(b, e, tom=True)
    os.environ.update(NETREP_NUM_GPUS="2", NETREP_SHARE_DEVICE="1")
    two = _bundled_call(b, e, tom=True)
    np.savez(out, one_nulls=one["nulls"], two_nulls=two["nulls"], one_obs=one["observed"], two_obs=two["observed"])


def test_sharded_path_bitwise_equal(tmp_path):
    """NETREP_NUM_GPUS=2 NETREP_SHARE_DEVICE=1: the TOM dataset built in
    context 0 is broadcast device to device; the cube is bitwise the
    one-context cube (in one fresh child process)."""
    out = str(tmp_path / "cubes.npz")
    mp.spawn(_sharded_child, args=(out,), nprocs=1, join=True)
    with np.load(out) as f:
        assert f["one_nulls"].shape == (4, 7, 16) and np.isfinite(f["one_nulls"]).any()
        np.testing.assert_array_equal(_bits(f["one_nulls"]), _bits(f["two_nulls"]))
        np.testing.assert_array_equal(_bits(f["one_obs"]), _bits(f["two_obs"]))
