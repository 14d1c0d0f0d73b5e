"""CPU tests of the host rules behind the connectivity-by-module entries: the
eigengene tree (netrep_EigengeneTree) against the restatement bit for bit for
both linkages and against scipy's complete linkage, its ties and its invalid
arguments, the intramodular rules (netrep_IntramodularConnectivity) against
the restatement, and the restated node order on a table with tied degrees."""
import numpy as np
import pytest

import netrep_amd as N
from netrep_amd import _lib as L

import connectivity_ref as K
import hclust_ref as H
import modmerge_ref as R

import scipy.cluster.hierarchy as scipy_hierarchy  # noqa: E402
from scipy.spatial.distance import squareform  # noqa: E402


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _eigengenes(s, m, seed):
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((s, max(m // 3, 1)))
    return np.asfortranarray(base[:, rng.integers(0, base.shape[1], m)] + 0.6 * rng.standard_normal((s, m)))


CASES = [(5, 2, 4), (23, 3, 1), (40, 7, 2), (130, 37, 3)]


# 1: the tree ------------------------------------------------------------------

@pytest.mark.parametrize("s,m,seed", CASES)
@pytest.mark.parametrize("linkage", ["average", "complete"])
def test_tree_against_the_restatement(s, m, seed, linkage):
    eig = _eigengenes(s, m, seed)
    id_lo, id_hi, height = N.eigengeneTree(eig, linkage)
    e_lo, e_hi, e_height, sets = K.eigengene_tree(eig, linkage)
    np.testing.assert_array_equal(id_lo, e_lo)
    np.testing.assert_array_equal(id_hi, e_hi)
    np.testing.assert_array_equal(_bits(height), _bits(e_height))
    # the groups: the ids name the column sets the restatement merged, step by step
    got = H.clusters(m, zip(id_lo, id_hi), height)
    assert list(got) == sets
    if linkage == "average":
        _group, g_heights = N.eigengeneGroups(eig, 0.25)
        np.testing.assert_array_equal(_bits(height), _bits(g_heights))
    # netrep_HclustFinish accepts the triples
    merge, h, order, _repairs = N.hclustFinish(m, id_lo, id_hi, height)
    e_merge, e_h, e_order, _r = H.finish(m, e_lo, e_hi, e_height)
    np.testing.assert_array_equal(merge, e_merge)
    np.testing.assert_array_equal(_bits(h), _bits(e_h))
    np.testing.assert_array_equal(order, e_order)
    assert sorted(order.tolist()) == list(range(1, m + 1))


@pytest.mark.parametrize("s,m,seed", CASES)
def test_complete_linkage_against_scipy(s, m, seed):
    eig = _eigengenes(s, m, seed)
    d = np.array(R.eigengene_dissimilarity(eig))
    Z = scipy_hierarchy.linkage(squareform(d, checks=False), "complete")
    zh = Z[:, 2]
    bar = H.height_bar(m)
    if zh.size > 1:
        gaps = np.diff(zh) / zh[1:]
        print(f"M = {m}: smallest relative height gap {gaps.min():.3e}, 1,000 bars = {1e3 * bar:.3e}")
        assert gaps.min() > 1e3 * bar, "precondition: scipy's heights are more than 1,000 bars apart"
    id_lo, id_hi, height = N.eigengeneTree(eig, "complete")
    got = H.clusters(m, zip(id_lo, id_hi), height)
    exp = H.clusters(m, Z[:, :2], Z[:, 2])
    assert set(got) == set(exp)
    worst = max(abs(got[k] - exp[k]) / exp[k] for k in exp)
    print(f"M = {m}: worst relative height error {worst:.3e} (bar {bar:.3e})")
    assert worst <= bar


def test_one_module():
    e = np.random.default_rng(5).standard_normal((12, 1))
    for linkage in ("average", "complete"):
        id_lo, id_hi, height = N.eigengeneTree(e, linkage)
        assert id_lo.size == id_hi.size == height.size == 0
    lib = L.load()
    assert lib.netrep_EigengeneTree(e.ctypes.data_as(L._dp), 12, 1, 1, None, None, None) == L.NR_OK
    assert K.module_order(e, [4]) == [4]


def test_exact_ties_go_to_the_lowest_pair():
    # orthogonal +-1 patterns: distinct columns have d = 1 exactly, copies d = 0 exactly:
    # columns (0, 3) and (1, 2) tie at 0, then everything ties at 1
    h = np.array([[1, 1, 1, 1, -1, -1, -1, -1], [1, 1, -1, -1, 1, 1, -1, -1], [1, -1, 1, -1, 1, -1, 1, -1]], float).T
    eig = np.column_stack([h[:, 0], h[:, 1], h[:, 1], h[:, 0], h[:, 2]])
    for linkage in ("average", "complete"):
        id_lo, id_hi, height = N.eigengeneTree(eig, linkage)
        assert height.tolist() == [0.0, 0.0, 1.0, 1.0]
        # (0, 3) before (1, 2); then clusters {0, 3} (id 5) and {1, 2} (id 6); then {0 .. 3} (id 7) and column 4
        assert id_lo.tolist() == [0, 1, 5, 7] and id_hi.tolist() == [3, 2, 6, 4]
        e_lo, e_hi, e_height, _sets = K.eigengene_tree(eig, linkage)
        assert (id_lo.tolist(), id_hi.tolist(), height.tolist()) == (e_lo.tolist(), e_hi.tolist(), e_height.tolist())
        _merge, _h, order, _r = N.hclustFinish(5, id_lo, id_hi, height)
        assert order.tolist() == [5, 1, 4, 2, 3]         # a row's singleton stands before its cluster, as in R


def test_invalid_arguments():
    lib = L.load()
    e = np.asfortranarray(np.random.default_rng(7).standard_normal((10, 3)))
    lo, hi, h = np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32), np.zeros(2)
    dp, ip = lambda a: a.ctypes.data_as(L._dp), lambda a: a.ctypes.data_as(L._i32p)  # noqa: E731
    assert lib.netrep_EigengeneTree(dp(e), 10, 3, 1, ip(lo), ip(hi), dp(h)) == L.NR_OK
    for linkage in (-1, 2):
        assert lib.netrep_EigengeneTree(dp(e), 10, 3, linkage, ip(lo), ip(hi), dp(h)) == L.NR_ERR_INVALID
        assert b"linkage" in lib.netrep_last_error()
    assert lib.netrep_EigengeneTree(None, 10, 3, 1, ip(lo), ip(hi), dp(h)) == L.NR_ERR_INVALID
    assert lib.netrep_EigengeneTree(dp(e), 10, 3, 1, None, ip(hi), dp(h)) == L.NR_ERR_INVALID
    assert lib.netrep_EigengeneTree(dp(e), 10, 0, 1, ip(lo), ip(hi), dp(h)) == L.NR_ERR_INVALID
    assert lib.netrep_EigengeneTree(dp(e), 1, 3, 1, ip(lo), ip(hi), dp(h)) == L.NR_ERR_INVALID
    const = e.copy(order="F")
    const[:, 1] = 3.0
    assert lib.netrep_EigengeneTree(dp(const), 10, 3, 1, ip(lo), ip(hi), dp(h)) == L.NR_ERR_INVALID
    with pytest.raises(N.NetRepError):
        N.eigengeneTree(e, "ward")
    # the handle entries check their arguments before they touch a device
    assert lib.netrep_DatasetModuleConnectivity(None, None, None, None) == L.NR_ERR_INVALID
    assert b"no dataset" in lib.netrep_last_error()
    assert lib.netrep_DatasetIntramodularConnectivity(None, None, None, None, None, None) == L.NR_ERR_INVALID
    assert b"no dataset" in lib.netrep_last_error()
    assert lib.nr_module_connectivity(None, 1, None, None, None) == L.NR_ERR_INVALID
    labels = np.array([1, 0, 2], dtype=np.int32)
    k = np.ones(3)
    table = np.ones((3, 2), order="F")
    for bad, text in ((np.array([1, -1, 2], dtype=np.int32), b"negative label"),
                      (np.zeros(3, dtype=np.int32), b"no positive label")):
        assert lib.netrep_IntramodularConnectivity(3, ip(bad), dp(k), dp(table), dp(k), dp(k), dp(k)) == L.NR_ERR_INVALID
        assert text in lib.netrep_last_error()
    assert lib.netrep_IntramodularConnectivity(3, ip(labels), None, dp(table), dp(k), dp(k), dp(k)) == L.NR_ERR_INVALID


# 2: the rules on a table ------------------------------------------------------

def test_intramodular_rules_and_node_order_with_tied_degrees():
    labels = np.array([5, 2, 0, 2, 5, 5, 2, 0, 9], dtype=np.int32)
    slot, mods = K.slots_of(labels)
    assert mods.tolist() == [2, 5, 9] and slot.tolist() == [1, 0, -1, 0, 1, 1, 0, -1, 2]
    n = labels.size
    rng = np.random.default_rng(3)
    k_mod = np.asfortranarray(rng.uniform(0.1, 2.0, (n, 3)))
    k_mod[[0, 5], 1] = 1.25                      # nodes 0 and 5 of module 5 tie; node 4 lies above both
    k_mod[4, 1] = 1.5
    k_mod[[1, 3, 6], 0] = 0.75                   # all of module 2 tie
    k_mod[8, 2] = 0.0                            # a one-node module
    k_total = k_mod.sum(axis=1) + rng.uniform(0.0, 1.0, n)
    got = N.intramodularConnectivity(labels, k_total, k_mod)
    within, out, diff = K.intramodular(slot, k_total, k_mod)
    for key, exp in (("kWithin", within), ("kOut", out), ("kDiff", diff)):
        np.testing.assert_array_equal(_bits(got[key]), _bits(exp), err_msg=key)
    assert np.isnan(got["kWithin"][[2, 7]]).all() and np.isnan(got["kOut"][[2, 7]]).all()
    assert np.isnan(got["kDiff"][[2, 7]]).all() and np.isfinite(got["kWithin"][labels > 0]).all()
    assert got["kWithin"][4] == 1.5 and got["kWithin"][8] == 0.0
    names = [f"g{i}" for i in range(n)]
    flat, per = K.node_order(labels, within, names, [5, 9, 2])
    assert per == {5: ["g4", "g0", "g5"], 9: ["g8"], 2: ["g1", "g3", "g6"]}
    assert flat == ["g4", "g0", "g5", "g8", "g1", "g3", "g6"]
    # the sample order keeps ties in sample order too
    eig = np.array([[0.5, -1.0], [0.7, 2.0], [0.5, 2.0], [-0.1, 0.0]])
    order = K.sample_order(eig, [3, 8])
    assert order[3].tolist() == [1, 0, 2, 3] and order[8].tolist() == [1, 2, 3, 0]
