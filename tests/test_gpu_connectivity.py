"""Connectivity by module on a resident from-data dataset
(nr_module_connectivity and the netrep_Dataset* entries behind
FromDataDataset.module_connectivity, intramodular_connectivity, hub_nodes,
node_order and sample_order): the table bit for bit against the numpy
restatement of the stated summation order run on the dataset's own exported
network, against the exactly rounded sum, against net_props' degree,
independence of the module tile, the module count and the pair layout, that
nothing resident changes, the orders end to end, and the edge cases."""
import ctypes as C

import numpy as np
import pytest

import netrep_amd as N
from netrep_amd import _lib as L
from netrep_amd.api import RMatrix

import connectivity_ref as K
import hclust_ref as H
import modmerge_ref as R
from conftest import assert_stats_close
from test_gpu_dual import _case
from test_gpu_netbuild import _set_modules
from test_modmerge_host import LARGE, planted_case

pytestmark = pytest.mark.gpu

BETA = 5.0
S = 23
KINDS = {"unsigned": dict(net_type="unsigned", tom=False), "signed": dict(net_type="signed", tom=False),
         "tom": dict(net_type="unsigned", tom=True)}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _names(n):
    return [f"g{i}" for i in range(n)]


def _bar(n):
    """Both orders sum at most n non-negative terms: (n + 16) 2^-52 relative."""
    return (n + 16) * 2.0 ** -52


def _scratch_bytes(eng):
    b = C.c_int64()
    assert L.load().nr_scratch_bytes(eng._h, C.byref(b)) == L.NR_OK
    return b.value


_DATA = {}


def data_of(n):
    """Planted data of n nodes, made once."""
    if n not in _DATA:
        k = max(n // 8, 1)
        x, _labels = R.planted(n, S, [k] * 5, {}, seed=300 + n)
        x.setflags(write=False)
        _DATA[n] = x
    return _DATA[n]


def slots(n, m, seed=0):
    """m modules of equal size over three quarters of the nodes (one node each
    where n is small), scattered over the node order so that every lane meets
    every module; the rest unassigned."""
    rng = np.random.default_rng([n, m, seed])
    k = max((3 * n // 4) // m, 1)
    slot = np.full(n, -1, dtype=np.int32)
    slot[rng.permutation(n)[:k * m]] = np.repeat(np.arange(m, dtype=np.int32), k)
    return slot


def _assert_table_equal(got, exp, what):
    np.testing.assert_array_equal(_bits(got[0]), _bits(exp[0]), err_msg=f"{what}: k_mod")
    np.testing.assert_array_equal(_bits(got[1]), _bits(exp[1]), err_msg=f"{what}: k_total")


# 1 -------------------------------------------------------------------------

# 63: a lane with no row; 64: exactly one row per lane; 65: one lane with two rows; 97: not a multiple of
# 64; 600: the unrolled walk (8 x 64 rows) and its remainder. M = 70: more than any default tile (two passes).
@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("n", [63, 64, 65, 97, 600])
def test_table_bitwise_against_the_restatement_and_the_exact_sum(n, kind):
    x = data_of(n)
    with N.Engine(0) as eng:
        eng.set_dataset_from_data(x, BETA, **KINDS[kind])
        _corr, net = eng.matrices()
        got = {m: eng.module_connectivity(m, slots(n, m)) for m in ((1, 3, 37, 70) if n == 600 else (1, 3, 37))}
        assert eng.connectivity_ms() > 0.0
    assert (net >= 0.0).all()
    np.testing.assert_array_equal(net, net.T)
    for m, (k_mod, k_total) in got.items():
        slot = slots(n, m)
        _assert_table_equal((k_mod, k_total), K.module_connectivity(net, slot, m), f"n={n} M={m} {kind}")
        f_mod, f_total = K.fsum_table(net, slot, m)
        worst = 0.0
        for a, b in ((k_mod, f_mod), (k_total, f_total)):
            nz = b > 0
            assert (a[~nz] == 0.0).all()
            worst = max(worst, float((np.abs(a[nz] - b[nz]) / b[nz]).max()) if nz.any() else 0.0)
        print(f"n={n} M={m} {kind}: worst relative difference from the exactly rounded sum {worst:.3e} "
              f"(bar {_bar(n):.3e})")
        assert worst <= _bar(n)
        # what the table means: the module columns of an assigned-or-not node add up to less than kTotal
        assert (k_mod.sum(axis=1) <= k_total * (1 + 1e-12)).all()


# 2 -------------------------------------------------------------------------

def test_own_module_column_against_net_props_degree():
    x, labels = planted_case("large", 0.25)
    n = labels.size
    mods = R.modules_of(labels)
    ma = {f"g{i}": str(int(lab)) for i, lab in enumerate(labels)}
    with N.FromDataDataset(RMatrix(x, None, _names(n)), BETA, tom=True) as ds:
        table, k_total = ds.module_connectivity(labels)
        props = ds.net_props(ma, [str(int(m)) for m in mods])
    assert table.rownames == _names(n) and table.colnames == [f"k{int(m)}" for m in mods]
    assert k_total.shape == (n,)
    for j, m in enumerate(mods):
        worst = assert_stats_close(table.values[labels == m, j], props[str(int(m))]["degree"], what=f"module {m}")
        print(f"module {m}: worst scaled error of the own column against net_props' degree {worst:.3e}")


# 3 -------------------------------------------------------------------------

def test_cells_do_not_depend_on_the_tile_or_the_module_count():
    n, m = 600, 37
    slot = slots(n, m)
    with N.Engine(0) as eng:
        eng.set_dataset_from_data(data_of(n), BETA, tom=True)
        whole = eng.module_connectivity(m, slot)
        for tile in (1, 2, 5, 0):
            eng.set_connectivity_module_tile(tile)
            _assert_table_equal(eng.module_connectivity(m, slot), whole, f"tile {tile}")
        for j in range(m):                                            # every module alone
            k_mod, k_total = eng.module_connectivity(1, np.where(slot == j, 0, -1).astype(np.int32))
            np.testing.assert_array_equal(_bits(k_mod[:, 0]), _bits(whole[0][:, j]), err_msg=f"module {j} alone")
            np.testing.assert_array_equal(_bits(k_total), _bits(whole[1]), err_msg=f"k_total with module {j} alone")
        rev = eng.module_connectivity(m, np.where(slot >= 0, m - 1 - slot, -1).astype(np.int32))
        np.testing.assert_array_equal(_bits(rev[0][:, ::-1]), _bits(whole[0]), err_msg="modules renumbered in reverse")
        np.testing.assert_array_equal(_bits(rev[1]), _bits(whole[1]))
        for bad in (-1, 65):
            with pytest.raises(N.NetRepError) as ei:
                eng.set_connectivity_module_tile(bad)
            assert ei.value.code == L.NR_ERR_INVALID


# 4 -------------------------------------------------------------------------

def test_either_pair_layout_and_nothing_resident_changes():
    """Before and after a permutation run that leaves the Gram table in place
    of the pair array: the same bits, and the call changes nothing resident."""
    lay, mi, disc, txs, _tc, _tn = _case([130, 120], 140, 31, n_nodes=400)
    slot = slots(400, 37)
    with N.Engine(0) as eng:
        eng.set_dataset_from_data(txs, BETA, scale=False, tom=True)
        _set_modules(eng, mi, disc)
        assert not eng.gram_table()
        corr0, net0 = eng.matrices()
        before = eng.module_connectivity(37, slot)
        obs, nulls = eng.observed(), eng.run(0, 64, 77)
        assert eng.gram_table()
        held = _scratch_bytes(eng)
        after = eng.module_connectivity(37, slot)
        assert _scratch_bytes(eng) == held and eng.gram_table()
        _assert_table_equal(after, before, "Gram table vs pair array")
        _assert_table_equal(before, K.module_connectivity(net0, slot, 37), "pair array vs the restatement")
        np.testing.assert_array_equal(_bits(eng.observed()), _bits(obs))
        np.testing.assert_array_equal(_bits(eng.run(0, 64, 77)), _bits(nulls))
        corr1, net1 = eng.matrices()
        np.testing.assert_array_equal(_bits(corr1), _bits(corr0))
        np.testing.assert_array_equal(_bits(net1), _bits(net0))
    # on a handle: every other output is the same before and after the new calls
    names, ma, modules = list(lay.names), dict(zip(lay.names, lay.labels)), list(lay.modules)
    labels = (slot + 1).astype(np.int32)

    def snapshot(ds):
        corr, net = ds.matrices()
        props = ds.net_props(ma, modules)
        tree = ds.hclust()
        dp = ds.intermediate_properties(names, ma, modules)
        perm = ds.permutation_procedure(dp, ma, modules, 64, seed=5)
        flat = [corr.values, net.values, tree["height"], tree["merge"].astype(np.float64), perm["observed"],
                perm["nulls"]]
        for m in modules:
            flat += [props[m]["degree"], props[m]["summary"], props[m]["contribution"]]
        return [_bits(a).copy() for a in flat]

    with N.FromDataDataset(RMatrix(np.asfortranarray(txs), None, names), BETA, scaleData=False, tom=True) as ds:
        first = snapshot(ds)
        table, k_total = ds.module_connectivity(labels)               # on the Gram table the run left
        ds.intramodular_connectivity(labels)
        ds.hub_nodes(labels)
        ds.node_order(labels)
        ds.sample_order(labels)
        second = snapshot(ds)
    for a, b in zip(first, second):
        np.testing.assert_array_equal(a, b)
    _assert_table_equal((table.values, k_total), before, "the handle after a run vs the engine's pair array")


# 5 -------------------------------------------------------------------------

def test_intramodular_hubs_and_orders_on_the_planted_modules():
    x, labels = planted_case("large", 0.25)
    n, names = labels.size, _names(labels.size)
    slot, mods = K.slots_of(labels)
    assert mods.size == 7 and (labels == 0).any()
    with N.FromDataDataset(RMatrix(x, None, names), BETA, tom=True) as ds:
        _corr, net = ds.matrices()
        k = ds.intramodular_connectivity(labels)
        table, k_total = ds.module_connectivity(labels)
        hubs = ds.hub_nodes(labels)
        order = ds.node_order(labels)
        plain = ds.node_order(labels, orderModules=False)
        samples = ds.sample_order(labels)
        eig = ds.module_eigengenes(labels)["eigengenes"]
    e_mod, e_total = K.module_connectivity(net.values, slot, mods.size)
    _assert_table_equal((table.values, k_total), (e_mod, e_total), "handle table")
    within, out, diff = K.intramodular(slot, e_total, e_mod)
    np.testing.assert_array_equal(k["modules"], mods)
    for key, exp in (("kTotal", e_total), ("kWithin", within), ("kOut", out), ("kDiff", diff)):
        np.testing.assert_array_equal(_bits(k[key][labels > 0]), _bits(exp[labels > 0]), err_msg=key)
    # identities: kWithin + kOut == kTotal to one rounding; NaN exactly on label 0
    sel = labels > 0
    assert (np.abs(k["kWithin"][sel] + k["kOut"][sel] - k["kTotal"][sel]) <= 2.0 ** -52 * k["kTotal"][sel]).all()
    for key in ("kWithin", "kOut", "kDiff"):
        assert np.isnan(k[key][~sel]).all() and np.isfinite(k[key][sel]).all()
    assert np.isfinite(k["kTotal"]).all()
    # preconditions of the orders, on the restatement: no two kWithin of a module, and no two tree
    # heights, closer than 1,000 bars
    for m in mods:
        v = np.sort(within[labels == m])
        assert (np.diff(v) / v[1:]).min() > 1e3 * _bar(n), f"precondition: kWithin of module {m} apart"
    id_lo, id_hi, height, _sets = K.eigengene_tree(eig, "complete")
    hs = np.sort(height)
    assert (np.diff(hs) / hs[1:]).min() > 1e3 * H.height_bar(mods.size), "precondition: tree heights apart"
    assert hubs == {int(m): names[int(np.flatnonzero(labels == m)[np.argmax(within[labels == m])])] for m in mods}
    mod_order = K.module_order(eig, mods)
    assert sorted(mod_order) == mods.tolist() and mod_order != mods.tolist()
    flat, per = K.node_order(labels, within, names, mod_order)
    assert order["nodes"] == flat and order["modules"] == per and list(order["modules"]) == mod_order
    flat0, per0 = K.node_order(labels, within, names, mods.tolist())
    assert plain["nodes"] == flat0 and plain["modules"] == per0 and list(plain["modules"]) == mods.tolist()
    assert len(flat) == int(sel.sum()) and set(flat) == {names[i] for i in np.flatnonzero(sel)}
    e_samples = K.sample_order(eig, mods)
    assert list(samples) == mods.tolist()
    for m in mods:
        np.testing.assert_array_equal(samples[int(m)], e_samples[int(m)], err_msg=f"sample order of module {m}")
        assert sorted(samples[int(m)].tolist()) == list(range(LARGE["s"]))


# 6 -------------------------------------------------------------------------

def test_edge_cases():
    rng = np.random.default_rng(9)
    s, n = 23, 40
    x = np.asfortranarray(rng.standard_normal((s, n)))
    with N.FromDataDataset(RMatrix(x[:, :1], None, ["a"]), BETA) as ds:         # n = 1
        table, k_total = ds.module_connectivity(np.array([4], dtype=np.int32))
        assert table.values.tolist() == [[0.0]] and k_total.tolist() == [0.0] and table.colnames == ["k4"]
        assert ds.hub_nodes([4]) == {4: "a"} and ds.node_order([4])["nodes"] == ["a"]
    everyone = np.full(n, 6, dtype=np.int32)
    single = np.zeros(n, dtype=np.int32)
    single[30] = 2
    ds = N.FromDataDataset(RMatrix(x, None, _names(n)), BETA)
    try:
        _corr, net = ds.matrices()
        k = ds.intramodular_connectivity(everyone)                              # all nodes in one module
        np.testing.assert_array_equal(_bits(k["kWithin"]), _bits(k["kTotal"]))
        assert (k["kOut"] == 0.0).all()
        np.testing.assert_array_equal(_bits(k["kDiff"]), _bits(k["kTotal"]))
        np.testing.assert_array_equal(_bits(k["kTotal"]), _bits(K.module_connectivity(net.values, np.zeros(n), 1)[1]))
        assert ds.node_order(everyone)["modules"].keys() == {6}
        k = ds.intramodular_connectivity(single)                                # a one-node module
        assert k["kWithin"][30] == 0.0 and k["kOut"][30] == k["kTotal"][30] and k["kDiff"][30] == -k["kTotal"][30]
        assert np.isnan(np.delete(k["kWithin"], 30)).all()
        table, _k_total = ds.module_connectivity(single)
        np.testing.assert_array_equal(np.delete(table.values[:, 0], 30), np.delete(net.values[30], 30))
        assert ds.hub_nodes(single) == {2: "g30"}
        calls = (ds.module_connectivity, ds.intramodular_connectivity, ds.hub_nodes, ds.node_order, ds.sample_order)
        for bad, text in ((np.where(everyone > 0, -1, 0), "negative label"),
                          (np.zeros(n, dtype=np.int32), "no positive label")):
            for call in calls:
                with pytest.raises(N.NetRepError) as ei:
                    call(bad)
                assert ei.value.code == L.NR_ERR_INVALID and text in str(ei.value)
        with pytest.raises(N.NetRepError):
            ds.module_connectivity(everyone[:-1])
    finally:
        ds.close()
    for call in calls:
        with pytest.raises(N.NetRepError) as ei:
            call(everyone)
        assert ei.value.code == L.NR_ERR_INVALID
    # the engine entry's own checks
    with N.Engine(0) as eng:
        lib = eng._lib
        sl = np.zeros(n, dtype=np.int32)
        out = np.zeros((n, 2), order="F")
        ip, dp = sl.ctypes.data_as(L._i32p), out.ctypes.data_as(L._dp)
        assert lib.nr_module_connectivity(eng._h, 1, ip, None, dp) == L.NR_ERR_INVALID
        assert b"no dataset" in lib.nr_last_error(eng._h)
        eng.set_dataset_from_data(x, BETA)
        assert lib.nr_module_connectivity(eng._h, 0, ip, None, dp) == L.NR_ERR_INVALID
        assert lib.nr_module_connectivity(eng._h, 1, None, None, dp) == L.NR_ERR_INVALID
        assert lib.nr_module_connectivity(eng._h, 1, ip, None, None) == L.NR_ERR_INVALID
        for bad in (-2, 2):
            sl[17] = bad
            assert lib.nr_module_connectivity(eng._h, 2, ip, None, dp) == L.NR_ERR_INVALID
            assert b"slot[17]" in lib.nr_last_error(eng._h)
        sl[17] = 1
        assert lib.nr_module_connectivity(eng._h, 2, ip, None, dp) == L.NR_OK                # k_total is optional
        np.testing.assert_array_equal(_bits(out), _bits(eng.module_connectivity(2, sl)[0]))


def test_host_matrices_with_negative_weights_are_summed_by_magnitude():
    n = 70
    rng = np.random.default_rng(4)
    net = rng.uniform(-1.0, 1.0, (n, n))
    net = np.asfortranarray((net + net.T) / 2)
    corr = np.asfortranarray(np.clip(net, -1, 1))
    slot = slots(n, 3)
    with N.Engine(0) as eng:
        eng.set_dataset(corr, net)
        got = eng.module_connectivity(3, slot)
    assert (net < 0).any()
    _assert_table_equal(got, K.module_connectivity(net, slot, 3), "host matrices")
