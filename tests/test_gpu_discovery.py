"""The resident from-data dataset (FromDataDataset / netrep_Dataset*) in every
role -- discovery properties, network properties, the permutation test -- and
the one-shots and the driver built on it: against the reference's recorded
results within the parity bar, and bitwise against the host-matrix entries fed
the handle's own exported matrices."""
import ctypes as C

import numpy as np
import pytest

import netrep_amd as N
from netrep_amd import _lib as L
from netrep_amd.api import RMatrix
from netrep_amd.pvalues import permutationTest

import netbuild_ref as R
from conftest import assert_stats_close
from test_gpu_cor import _data
from test_gpu_dual import _case
from test_gpu_netbuild import _bits

pytestmark = pytest.mark.gpu

MODULES = ["1", "2", "3", "4"]
DISC_KEYS = ("degree", "corr", "contribution")


def _bundled(b):
    ma = dict(zip(b["module_labels_names"].tolist(), b["module_labels"].tolist()))
    disc = RMatrix(b["discovery_data"], None, b["discovery_data_colnames"].tolist())
    test = RMatrix(b["test_data"], None, b["test_data_colnames"].tolist())
    return disc, test, ma


def _pooled():
    n = C.c_int64()
    assert L.load().netrep_PoolInfo(C.byref(n), None, None, None) == L.NR_OK
    return int(n.value)


def _assert_disc_bitwise(got, exp, what):
    assert set(got) == set(exp) == set(DISC_KEYS), what
    for key in DISC_KEYS:
        assert list(got[key]) == list(exp[key]), (what, key)
        for m in exp[key]:
            np.testing.assert_array_equal(_bits(got[key][m]), _bits(exp[key][m]), err_msg=f"{what} {key}/{m}")


def _assert_result_bitwise(a, b, what):
    for key in ("observed", "nulls"):
        np.testing.assert_array_equal(_bits(a[key]), _bits(b[key]), err_msg=f"{what}: {key}")


# the pair-array regime and the Gram-table regime (test_gpu_cor's shapes)
CASES = {"pairs": ([40, 20, 7], 30, 150), "table": ([130, 120], 140, 400)}


@pytest.fixture(scope="module", params=list(CASES))
def case(request):
    sizes, s, n = CASES[request.param]
    lay, _mi, _disc, txs, _tc, _tn = _case(sizes, s, 31, n_nodes=n)
    return dict(names=list(lay.names), ma=dict(zip(lay.names, lay.labels)), modules=list(lay.modules),
                txs=np.asfortranarray(txs), table=request.param == "table")


# 1 -------------------------------------------------------------------------

def test_one_shots_against_the_recorded_results(bundled, bundled_expected):
    """Raw data in, the reference's recorded discovery and network properties
    out. The discovery and test column orders differ, so names are mapped."""
    disc, test, ma = _bundled(bundled)
    e = bundled_expected
    assert list(disc.colnames) != list(test.colnames)
    got = N.IntermediatePropertiesFromData(disc, 5.0, list(test.colnames), ma, MODULES, scaleData=True)
    assert set(got) == set(DISC_KEYS)
    for key in DISC_KEYS:
        for m in MODULES:
            err = assert_stats_close(got[key][m], e[f"disc_{key}_{m}_data"], what=f"{key}/{m}")
            print(f"IntermediatePropertiesFromData {key}/{m}: {err:.3e}")
    for tag, data in (("disc", disc), ("test", test)):
        got = N.NetPropsFromData(data, 5.0, ma, MODULES)
        for m in MODULES:
            for key in ("summary", "contribution", "degree"):
                err = assert_stats_close(got[m][key], e[f"netprops_{tag}_{m}_{key}"], what=f"{tag}/{m}/{key}")
                print(f"NetPropsFromData {tag}/{m}/{key}: {err:.3e}")
            assert_stats_close([got[m]["coherence"]], [e[f"netprops_{tag}_{m}_coherence"]], what=f"{tag}/{m}")
            assert_stats_close([got[m]["avgWeight"]], [e[f"netprops_{tag}_{m}_avgWeight"]], what=f"{tag}/{m}")


# 2 -------------------------------------------------------------------------

def test_bitwise_against_the_host_matrix_route(case):
    names, ma, modules, txs = case["names"], case["ma"], case["modules"], case["txs"]
    block = RMatrix(txs, None, names)
    with N.FromDataDataset(block, 5.0, scaleData=False) as ds:
        corr, net = ds.matrices()
        got_ip = ds.intermediate_properties(names, ma, modules)
        got_np = ds.net_props(ma, modules)
    assert list(corr.colnames) == names and list(net.colnames) == names
    _assert_disc_bitwise(got_ip, N.IntermediateProperties(block, corr, net, names, ma, modules), "discovery")
    # NetProps scales the (already scaled) block once more: the network side
    # is bitwise, the data side at the parity bar
    exp_np = N.NetProps(block, net, ma, modules)
    assert list(got_np) == list(exp_np) == modules
    for m in modules:
        assert got_np[m]["node_names"] == exp_np[m]["node_names"]
        np.testing.assert_array_equal(_bits(got_np[m]["degree"]), _bits(exp_np[m]["degree"]))
        assert np.float64(got_np[m]["avgWeight"]).tobytes() == np.float64(exp_np[m]["avgWeight"]).tobytes()
        for key in ("summary", "contribution"):
            assert_stats_close(got_np[m][key], exp_np[m][key], what=f"{m}/{key}")
        assert_stats_close([got_np[m]["coherence"]], [exp_np[m]["coherence"]], what=f"{m}/coherence")
    N.ReleaseResident()


# 3 -------------------------------------------------------------------------

@pytest.mark.parametrize("cor_type,net_type", [("pearson", "signed_hybrid"), ("spearman", "signed"),
                                               ("bicor", "unsigned")])
def test_with_options(cor_type, net_type):
    """The TOM (three tiles across, the last of one column) under every
    correlation type: the discovery vectors are those of the exported
    matrices."""
    n, s = 2 * N.Engine.NETBUILD_TILE + 1, 61
    xs = np.asfortranarray(R.scale(_data("student-t", s, n, 21)))
    names = [f"g{i}" for i in range(n)]
    labels = ["1"] * 40 + ["2"] * 25 + ["3"] * 7 + ["0"] * (n - 72)
    order = np.random.default_rng(5).permutation(n)          # modules scattered over the tiles
    ma = {names[j]: labels[i] for i, j in enumerate(order)}
    modules = ["1", "2", "3"]
    absent = names[order[0]]                                  # a node of module "1" absent from the test side
    t_names = [nm for nm in reversed(names) if nm != absent]
    block = RMatrix(xs, None, names)
    with N.FromDataDataset(block, 5.0, networkType=net_type, scaleData=False, tom=True, corType=cor_type) as ds:
        corr, net = ds.matrices()
        got = ds.intermediate_properties(t_names, ma, modules)
    c0, _w0 = N.BuildNetwork(block, 5.0, networkType=net_type, scaleData=False, corType=cor_type)
    t1 = N.BuildNetwork(block, 5.0, networkType=net_type, scaleData=False, tom=True, corType=cor_type)[1]
    np.testing.assert_array_equal(_bits(corr.values), _bits(c0.values))
    np.testing.assert_array_equal(_bits(net.values), _bits(t1.values))
    assert [got["degree"][m].size for m in modules] == [39, 25, 7]
    _assert_disc_bitwise(got, N.IntermediateProperties(block, corr, net, t_names, ma, modules),
                         f"{cor_type} {net_type} TOM")
    N.ReleaseResident()


# 4 -------------------------------------------------------------------------

def test_one_handle_every_role_nothing_rebuilt():
    sizes, s, n = CASES["table"]
    lay, _mi, _disc, txs, _tc, _tn = _case(sizes, s, 31, n_nodes=n)
    names, ma, modules = list(lay.names), dict(zip(lay.names, lay.labels)), list(lay.modules)
    block = RMatrix(np.asfortranarray(txs), None, names)
    data_bytes = 8 * s * n
    h0 = N.h2d_bytes()
    ds = N.FromDataDataset(block, 5.0, scaleData=False)
    built = N.h2d_bytes() - h0
    print(f"handle creation uploaded {built} bytes (data {data_bytes})")
    assert data_bytes <= built < data_bytes + 16 * n      # the data and no n x n matrix
    try:
        corr0, net0 = ds.matrices()
        disc = ds.intermediate_properties(names, ma, modules)
        props = ds.net_props(ma, modules)                     # on the pair array
        first = ds.permutation_procedure(disc, ma, modules, 8, seed=77)
        again = ds.intermediate_properties(names, ma, modules)
        h1 = N.h2d_bytes()
        second = ds.permutation_procedure(disc, ma, modules, 8, seed=77)
        rerun = N.h2d_bytes() - h1
        print(f"second permutation_procedure uploaded {rerun} bytes")
        assert rerun < data_bytes                             # module metadata only
        corr1, net1 = ds.matrices()
        props_after = ds.net_props(ma, modules)               # on the Gram table the runs left
    finally:
        ds.close()
    one_shot = N.PermutationProcedureFromData(disc, block, 5.0, ma, modules, 8, seed=77, scaleData=False)
    assert first["nulls"].shape == (len(modules), 7, 8) and np.isfinite(first["nulls"]).all()
    _assert_result_bitwise(first, second, "first vs second call on the handle")
    _assert_result_bitwise(first, one_shot, "handle vs PermutationProcedureFromData")
    _assert_disc_bitwise(again, disc, "discovery vectors after a permutation run")
    np.testing.assert_array_equal(_bits(corr1.values), _bits(corr0.values))
    np.testing.assert_array_equal(_bits(net1.values), _bits(net0.values))
    # the same kernels read the same values in the same order from either layout
    for m in modules:
        for key in ("degree", "summary", "contribution"):
            np.testing.assert_array_equal(_bits(props[m][key]), _bits(props_after[m][key]))


# 5 -------------------------------------------------------------------------

def test_the_driver_on_the_bundled_datasets(bundled, bundled_expected):
    disc, test, ma = _bundled(bundled)
    e = bundled_expected
    res = N.modulePreservationFromData({"discovery": disc, "test": test}, 5.0, {"discovery": ma},
                                       nPerm=e["pis"].shape[0], pi=e["pis"])
    assert list(res) == ["discovery"] and list(res["discovery"]) == ["test"]
    r = res["discovery"]["test"]
    assert {"observed", "nulls", "p.values", "nVarsPresent", "propVarsPresent", "totalSize", "contingency"} <= set(r)
    assert r["contingency"] is None                           # no module assignments for the test dataset
    assert r["modules"] == MODULES                            # every label but the background "0"
    eo = assert_stats_close(r["observed"], e["observed_data"], what="observed (driver)")
    en = assert_stats_close(r["nulls"], e["nulls_data"], what="nulls (driver)")
    print(f"driver on the bundled data: observed {eo:.3e}, nulls {en:.3e}")
    n_vars = [sum(1 for lab in ma.values() if lab == m) for m in MODULES]
    assert r["totalSize"] == 150 and list(r["nVarsPresent"].values()) == n_vars
    exp_p = permutationTest(r["nulls"], r["observed"], n_vars, 150, "greater")
    np.testing.assert_array_equal(_bits(r["p.values"]), _bits(exp_p))
    assert _pooled() >= 1                                     # its datasets were closed


# 6 -------------------------------------------------------------------------

def test_constant_column_returns_the_context(bundled):
    disc, _test, ma = _bundled(bundled)
    x = bundled["discovery_data"].copy()
    x[:, 37] = 2.5
    bad = RMatrix(x, None, list(disc.colnames))
    N.ReleaseResident()
    assert _pooled() == 0
    calls = (lambda: N.FromDataDataset(bad, 5.0),
             lambda: N.IntermediatePropertiesFromData(bad, 5.0, list(disc.colnames), ma, MODULES, scaleData=True),
             lambda: N.NetPropsFromData(bad, 5.0, ma, MODULES))
    for call in calls:
        with pytest.raises(N.NetRepError) as ei:
            call()
        assert ei.value.code == L.NR_ERR_NONFINITE
        assert "non-finite" in str(ei.value)
        assert _pooled() == 1


def test_missing_discovery_node_and_use_after_close(bundled):
    disc, test, ma = _bundled(bundled)
    ma2 = dict(ma)
    ma2["not_a_node"] = "1"
    ds = N.FromDataDataset(disc, 5.0)
    with pytest.raises(N.NetRepError) as ei:
        ds.intermediate_properties(list(test.colnames) + ["not_a_node"], ma2, MODULES)
    assert ei.value.code == L.NR_ERR_INVALID
    assert str(ei.value) == "node 'not_a_node' of moduleAssignments is not in the discovery dataset"
    good = ds.intermediate_properties(list(test.colnames), ma, MODULES)    # the handle survived the error
    assert list(good["degree"]) == MODULES
    ds.close()
    ds.close()
    for call in (lambda: ds.matrices(), lambda: ds.net_props(ma, MODULES),
                 lambda: ds.intermediate_properties(list(test.colnames), ma, MODULES),
                 lambda: ds.permutation_procedure(good, ma, MODULES, 0)):
        with pytest.raises(N.NetRepError) as ei:
            call()
        assert ei.value.code == L.NR_ERR_INVALID


def test_release_resident_leaves_live_handles(bundled, bundled_expected):
    disc, test, ma = _bundled(bundled)
    e = bundled_expected
    with N.FromDataDataset(disc, 5.0) as a, N.FromDataDataset(test, 5.0) as b:
        before = a.intermediate_properties(list(test.colnames), ma, MODULES)
        N.ReleaseResident()
        assert _pooled() == 0
        after = a.intermediate_properties(list(test.colnames), ma, MODULES)
        _assert_disc_bitwise(after, before, "after ReleaseResident")
        r = b.permutation_procedure(after, ma, MODULES, e["pis"].shape[0], pi=e["pis"])
        assert_stats_close(r["nulls"], e["nulls_data"], what="nulls after ReleaseResident")
    assert _pooled() >= 1
