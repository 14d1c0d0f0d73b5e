"""The average-linkage dendrogram of a resident from-data dataset
(nr_hclust_average / FromDataDataset.hclust / DetectModulesFromData): the raw
discovery-order output bit for bit against the numpy restatement run on the
dataset's own exported network, the finished tree against scipy on the same
matrix, independence of the launch size and of the pair layout, the edge
cases, and modules detected and tested for preservation end to end."""
import ctypes as C

import numpy as np
import pytest
import scipy.cluster.hierarchy as scipy_hierarchy
from scipy.spatial.distance import squareform

import netrep_amd as N
from netrep_amd import _lib as L
from netrep_amd.api import RMatrix

import hclust_ref as H
import netbuild_ref as NR
from test_gpu_dual import _case
from test_gpu_netbuild import _bits, _set_modules
from test_hclust_host import assert_same_tree, scipy_tree_with_gaps

pytestmark = pytest.mark.gpu

S = 40


def _scratch_bytes(eng):
    b = C.c_int64()
    assert L.load().nr_scratch_bytes(eng._h, C.byref(b)) == L.NR_OK
    return b.value


def _assert_raw_equal(a, b, what):
    np.testing.assert_array_equal(a[0], b[0], err_msg=f"{what}: id_lo")
    np.testing.assert_array_equal(a[1], b[1], err_msg=f"{what}: id_hi")
    np.testing.assert_array_equal(_bits(a[2]), _bits(b[2]), err_msg=f"{what}: height")
    np.testing.assert_array_equal(_bits(a[3]), _bits(b[3]), err_msg=f"{what}: size")


def _assert_tree_equal(a, b, what):
    assert set(a) == set(b), what
    np.testing.assert_array_equal(a["merge"], b["merge"], err_msg=what)
    np.testing.assert_array_equal(_bits(a["height"]), _bits(b["height"]), err_msg=what)
    np.testing.assert_array_equal(a["order"], b["order"], err_msg=what)
    assert a["labels"] == b["labels"] and a["method"] == b["method"] and a["n_repairs"] == b["n_repairs"], what


# 1 -------------------------------------------------------------------------

# 97: not a multiple of the wave or of a 16-byte pair; 600: several waves; 2,500:
# a column longer than one pass of the 1,024-thread workgroup (2 x 1,024 rows)
@pytest.mark.parametrize("n,net_type,tom", [(97, "unsigned", True), (600, "unsigned", True),
                                            (2500, "unsigned", True), (97, "signed", False)])
def test_raw_output_bitwise_against_the_restatement(n, net_type, tom):
    x, _which = H.module_data(n, S, 100 + n)
    with N.Engine(0) as eng:
        eng.set_dataset_from_data(x, 5.0, net_type, tom=tom)
        _corr, net = eng.matrices()
        got = eng.hclust_average()
        info, ms = eng.hclust_info(), eng.hclust_ms()
    np.testing.assert_array_equal(net, net.T)
    exp = H.chain(1.0 - net)
    print(f"n = {n} {net_type} tom={tom}: {info['searches'] / n:.2f} searches per node, {info['launches']} launches, "
          f"{ms:.2f} ms on the device")
    _assert_raw_equal(got, exp[:4], f"n={n}")
    assert info["searches"] == exp[4] < 3 * n
    ld = n + n % 2
    assert info["scratch_bytes"] == 8 * n * ld + 64 + 40 * n
    assert info["launches"] == -(-(n - 1) // 512) and ms > 0.0


# 2 -------------------------------------------------------------------------

def test_handle_tree_against_scipy():
    n = 600
    x, _which = H.module_data(n, S, 100 + n)
    names = [f"g{i}" for i in range(n)]
    with N.FromDataDataset(RMatrix(x, None, names), 5.0, tom=True) as ds:
        tree = ds.hclust()
        _corr, net = ds.matrices()
    assert tree["labels"] == names and tree["method"] == "average"
    assert tree["merge"].shape == (n - 1, 2) and tree["height"].shape == (n - 1,) and tree["order"].shape == (n,)
    assert sorted(tree["order"].tolist()) == list(range(1, n + 1))
    assert (np.diff(tree["height"]) >= 0).all() and tree["n_repairs"] == 0
    d = 1.0 - net.values
    np.fill_diagonal(d, 0.0)
    Z = scipy_tree_with_gaps(n, d)
    assert_same_tree(n, H.clusters_of_merge(n, tree["merge"], tree["height"]), H.clusters(n, Z[:, :2], Z[:, 2]),
                     "FromDataDataset.hclust vs scipy")
    # and the finished tree is the restatement's, bit for bit
    id_lo, id_hi, height, _size, _searches = H.chain(d)
    merge, h, order, repairs = H.finish(n, id_lo, id_hi, height)
    np.testing.assert_array_equal(tree["merge"], merge)
    np.testing.assert_array_equal(_bits(tree["height"]), _bits(h))
    np.testing.assert_array_equal(tree["order"], order)
    assert tree["n_repairs"] == repairs


# 3 -------------------------------------------------------------------------

def test_result_does_not_depend_on_the_launch_size():
    n = 97
    x, _which = H.module_data(n, S, 100 + n)
    with N.Engine(0) as eng:
        eng.set_dataset_from_data(x, 5.0, tom=True)
        base = eng.hclust_average()
        searches = eng.hclust_info()["searches"]
        assert eng.hclust_info()["launches"] == 1
        for m, launches in ((1, 96), (7, 14), (64, 2), (0, 1)):
            eng.set_hclust_merges_per_launch(m)
            _assert_raw_equal(eng.hclust_average(), base, f"M={m}")
            assert eng.hclust_info() == {"searches": searches, "launches": launches,
                                         "scratch_bytes": 8 * n * (n + 1) + 64 + 40 * n}
        with pytest.raises(N.NetRepError) as ei:
            eng.set_hclust_merges_per_launch(-1)
        assert ei.value.code == L.NR_ERR_INVALID


# 4 -------------------------------------------------------------------------

def test_either_pair_layout_and_nothing_resident_changes():
    """Before and after a permutation run that leaves the Gram table in place
    of the pair array: the same tree, and the call changes nothing resident."""
    lay, mi, disc, txs, _tc, _tn = _case([130, 120], 140, 31, n_nodes=400)
    names, ma, modules = list(lay.names), dict(zip(lay.names, lay.labels)), list(lay.modules)
    with N.FromDataDataset(RMatrix(np.asfortranarray(txs), None, names), 5.0, scaleData=False, tom=True) as ds:
        corr0, net0 = ds.matrices()
        tree0 = ds.hclust()                                   # on the pair array
        props0 = ds.net_props(ma, modules)
        dp = ds.intermediate_properties(names, ma, modules)
        ds.permutation_procedure(dp, ma, modules, 8, seed=77)
        props1 = ds.net_props(ma, modules)                    # on the Gram table the run left
        tree1 = ds.hclust()
        props2 = ds.net_props(ma, modules)
        corr2, net2 = ds.matrices()
    _assert_tree_equal(tree1, tree0, "Gram table vs pair array")
    np.testing.assert_array_equal(_bits(corr2.values), _bits(corr0.values))
    np.testing.assert_array_equal(_bits(net2.values), _bits(net0.values))
    for m in modules:
        for key in ("degree", "summary", "contribution"):
            np.testing.assert_array_equal(_bits(props2[m][key]), _bits(props1[m][key]))
            np.testing.assert_array_equal(_bits(props2[m][key]), _bits(props0[m][key]))
    # the same on an engine, where the layout and the scratch can be asked for
    with N.Engine(0) as eng:
        eng.set_dataset_from_data(txs, 5.0, scale=False, tom=True)
        _set_modules(eng, mi, disc)
        assert not eng.gram_table()
        before = eng.hclust_average()
        obs, nulls = eng.observed(), eng.run(0, 8, 77)
        assert eng.gram_table()
        held = _scratch_bytes(eng)
        after = eng.hclust_average()
        assert _scratch_bytes(eng) == held and eng.gram_table()
        _assert_raw_equal(after, before, "Gram table vs pair array (engine)")
        np.testing.assert_array_equal(_bits(eng.observed()), _bits(obs))
        np.testing.assert_array_equal(_bits(eng.run(0, 8, 77)), _bits(nulls))
    merge, h, order, _r = H.finish(400, *before[:3])
    np.testing.assert_array_equal(tree0["merge"], merge)
    np.testing.assert_array_equal(_bits(tree0["height"]), _bits(h))
    np.testing.assert_array_equal(tree0["order"], order)


# 5 -------------------------------------------------------------------------

def test_one_and_two_nodes():
    x = np.random.default_rng(3).normal(size=(S, 2))
    with N.FromDataDataset(RMatrix(x[:, :1], None, ["a"]), 5.0) as ds:
        t = ds.hclust()
    assert t["merge"].shape == (0, 2) and t["height"].shape == (0,) and t["order"].tolist() == [1]
    assert N.cutreeStatic(t, 0.5, 1).tolist() == [1]
    with N.FromDataDataset(RMatrix(x, None, ["a", "b"]), 5.0) as ds:
        t = ds.hclust()
        _corr, net = ds.matrices()
    assert t["merge"].tolist() == [[-1, -2]] and t["order"].tolist() == [1, 2]
    assert t["height"].tolist() == [1.0 - net.values[1, 0]]
    with N.Engine(0) as eng:
        eng.set_dataset_from_data(x[:, :1], 5.0)
        assert [a.size for a in eng.hclust_average()] == [0, 0, 0, 0]
        assert eng.hclust_info() == {"searches": 0, "launches": 0, "scratch_bytes": 0}
        eng.set_dataset_from_data(x, 5.0)
        id_lo, id_hi, height, size = eng.hclust_average()
        assert (id_lo.tolist(), id_hi.tolist(), size.tolist()) == ([0], [1], [2.0])
        assert eng.hclust_info()["searches"] == 2


def test_no_dataset_is_an_error():
    with N.Engine(0) as eng:
        with pytest.raises(N.NetRepError) as ei:
            eng._check(eng._lib.nr_hclust_average(eng._h, None, None, None, None))
        assert ei.value.code == L.NR_ERR_INVALID and "no dataset" in str(ei.value)


def test_cancel_requested_before_the_call_is_consumed():
    x, _which = H.module_data(97, S, 197)
    with N.Engine(0) as eng:
        eng.set_dataset_from_data(x, 5.0, tom=True)
        base = eng.hclust_average()
        eng._check(eng._lib.nr_cancel(eng._h))
        with pytest.raises(N.NetRepError) as ei:
            eng.hclust_average()
        assert ei.value.code == L.NR_ERR_CANCELLED
        _assert_raw_equal(eng.hclust_average(), base, "after a consumed cancellation")


def test_duplicated_columns_tie_exactly():
    """Exact ties (identical columns: d = 0 between them, equal distances to
    everything else): the call returns and the tree is valid. No comparison
    with another implementation's tie-breaking."""
    n = 61
    x = NR.scale(H.module_data(n, 9, 11)[0])
    # Columns that are scaled exactly (mean 0, sum of squares S - 1 = 8) and are
    # taken as they are: the correlation of two copies is 8 / 8 = 1 with no
    # rounding anywhere, so net = 1 and d = 0 exactly.
    x[:, 3] = x[:, 17] = x[:, 40] = [1, 1, 1, 1, -1, -1, -1, -1, 0]
    x[:, 22] = x[:, 58] = [1, -1, 0, 1, -1, 1, -1, 1, -1]
    x = np.asfortranarray(x)
    with N.FromDataDataset(RMatrix(x, None, [f"g{i}" for i in range(n)]), 5.0, scaleData=False) as ds:
        t = ds.hclust()
        _corr, net = ds.matrices()
    assert net.values[3, 17] == net.values[3, 40] == net.values[17, 40] == net.values[22, 58] == 1.0
    assert sorted(t["order"].tolist()) == list(range(1, n + 1))
    assert (np.diff(t["height"]) >= 0).all()
    assert t["height"][:3].tolist() == [0.0, 0.0, 0.0] and t["height"][3] > 0.0
    first = H.clusters_of_merge(n, t["merge"], t["height"])
    zero = {c for c, h in first.items() if h == 0.0}
    assert frozenset([3, 17, 40]) in zero and frozenset([22, 58]) in zero and len(zero) == 3
    # the restatement follows the same rules through the ties
    id_lo, id_hi, height, _size, _searches = H.chain(1.0 - net.values)
    merge, h, order, _r = H.finish(n, id_lo, id_hi, height)
    np.testing.assert_array_equal(t["merge"], merge)
    np.testing.assert_array_equal(_bits(t["height"]), _bits(h))
    np.testing.assert_array_equal(t["order"], order)


# 6 -------------------------------------------------------------------------

def test_detect_modules_then_preservation_end_to_end():
    n = 300
    x, which = H.module_data(n, S, 5)
    x2, which2 = H.module_data(n, S, 6, layout_seed=5)        # the same modules in a second dataset
    np.testing.assert_array_equal(which, which2)
    names = [f"g{i}" for i in range(n)]
    disc, test = RMatrix(x, None, names), RMatrix(x2, None, names)
    # the cut height: inside the largest height gap of scipy's tree of the same network
    _corr, net = N.BuildNetwork(disc, 5.0, tom=True)
    d = 1.0 - net.values
    np.fill_diagonal(d, 0.0)
    Z = scipy_hierarchy.linkage(squareform(d, checks=False), "average")
    at = int(np.argmax(np.diff(Z[:, 2])))
    cut = 0.5 * (Z[at, 2] + Z[at + 1, 2])
    res = N.DetectModulesFromData(disc, 5.0, cut, minSize=10)
    ma = res["moduleAssignments"]
    assert list(ma) == names and all(isinstance(v, str) for v in ma.values())
    labels = [ma[nm] for nm in names]
    assert "0" not in labels                                  # every planted module has at least 30 nodes
    assert len(set(zip(labels, which.tolist()))) == len(set(labels)) == len(set(which.tolist())) == 5
    sizes = [labels.count(str(k)) for k in range(1, 6)]
    assert sizes == sorted(sizes, reverse=True)               # numbered by decreasing size
    assert res["tree"]["labels"] == names
    out = N.modulePreservationFromData({"d": disc, "t": test}, 5.0, {"d": ma}, nPerm=64, tom=True)
    r = out["d"]["t"]
    assert r["modules"] == ["1", "2", "3", "4", "5"]
    assert r["p.values"].shape == (5, 7) and r["observed"].shape == (5, 7) and r["nulls"].shape == (5, 7, 64)
    assert np.isfinite(r["p.values"]).all()
    print("p-values of the detected modules (avg.weight, coherence):", r["p.values"][:, :2].tolist())
    assert (r["p.values"][:, 0] < 0.05).all()                 # planted in both datasets: preserved
    N.ReleaseResident()
