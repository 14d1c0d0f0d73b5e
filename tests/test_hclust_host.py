"""CPU tests of the dendrogram's host side: the finishing step and the static
cut of the library (netrep_HclustFinish, netrep_CutreeStatic) against their
numpy restatement bit for bit, the restated chain against scipy's average
linkage, both against a committed scipy fixture, and the termination guard's
host-side arithmetic."""
import ctypes as C
import os

import numpy as np
import pytest

import netrep_amd as N
from netrep_amd import _lib as L

import hclust_ref as H
import tom_ref as T
from conftest import GOLDEN

import scipy.cluster.hierarchy as scipy_hierarchy  # noqa: E402
from scipy.spatial.distance import squareform  # noqa: E402


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _assert_finish_matches_ref(n, id_lo, id_hi, height, what):
    merge, h, order, repairs = N.hclustFinish(n, id_lo, id_hi, height)
    e_merge, e_h, e_order, e_repairs = H.finish(n, id_lo, id_hi, height)
    np.testing.assert_array_equal(merge, e_merge, err_msg=what)
    np.testing.assert_array_equal(_bits(h), _bits(e_h), err_msg=what)
    np.testing.assert_array_equal(order, e_order, err_msg=what)
    assert repairs == e_repairs, what
    assert sorted(order.tolist()) == list(range(1, n + 1)), what
    assert (np.diff(h) >= 0).all(), what
    return merge, h, order, repairs


# 1: the finishing function on hand-made discovery lists ---------------------

def test_finish_row_order_rules():
    """Two singletons in increasing node index whatever the slot order, a
    singleton before a cluster, two clusters in increasing sorted step."""
    n = 6
    # t0: nodes 4, 1 (given hi-first); t1: nodes 0, 5; t2: cluster 7 with node 2; t3: clusters 8, 6; t4: node 3
    id_lo = [4, 0, 7, 8, 10 - 1]
    id_hi = [1, 5, 2, 6, 3]
    height = [0.3, 0.1, 0.2, 0.5, 0.9]
    merge, h, order, repairs = _assert_finish_matches_ref(n, id_lo, id_hi, height, "row order")
    assert repairs == 0
    assert h.tolist() == [0.1, 0.2, 0.3, 0.5, 0.9]
    assert merge.tolist() == [[-1, -6], [-3, 1], [-2, -5], [2, 3], [-4, 4]]
    assert order.tolist() == [4, 3, 1, 6, 2, 5]


def test_finish_equal_heights_keep_discovery_order():
    n = 5
    id_lo, id_hi = [0, 2, 5, 7], [1, 3, 6, 4]
    height = [0.25, 0.25, 0.25, 0.25]
    merge, h, _order, repairs = _assert_finish_matches_ref(n, id_lo, id_hi, height, "equal heights")
    assert repairs == 0 and h.tolist() == height
    assert merge.tolist() == [[-1, -2], [-3, -4], [1, 2], [-5, 3]]      # the stable sort moved nothing


def test_finish_repairs_a_parent_one_ulp_below_its_child():
    n = 4
    child = 0.5
    parent = np.nextafter(child, 0.0)                                     # one ulp below
    id_lo, id_hi = [0, 4, 5], [1, 2, 3]
    height = [child, parent, 0.75]
    merge, h, _order, repairs = _assert_finish_matches_ref(n, id_lo, id_hi, height, "one ulp")
    assert repairs == 1
    assert h.tolist() == [child, child, 0.75]
    assert merge.tolist() == [[-1, -2], [-3, 1], [-4, 2]]                 # the child still precedes its parent
    # a repaired height propagates: the grandparent below both is raised too
    height = [child, parent, np.nextafter(parent, 0.0)]
    _m, h, _o, repairs = _assert_finish_matches_ref(n, id_lo, id_hi, height, "two repairs")
    assert repairs == 2 and h.tolist() == [child] * 3


def test_finish_one_and_two_nodes():
    merge, h, order, repairs = _assert_finish_matches_ref(1, [], [], [], "n = 1")
    assert merge.shape == (0, 2) and h.shape == (0,) and order.tolist() == [1] and repairs == 0
    merge, h, order, _r = _assert_finish_matches_ref(2, [1], [0], [0.125], "n = 2")
    assert merge.tolist() == [[-1, -2]] and h.tolist() == [0.125] and order.tolist() == [1, 2]
    np.testing.assert_array_equal(N.cutreeStatic({"merge": merge, "height": h}, 0.2, 1), [1, 1])
    np.testing.assert_array_equal(N.cutreeStatic({"merge": merge, "height": h}, 0.1, 1), [1, 2])
    np.testing.assert_array_equal(N.cutreeStatic({"merge": np.zeros((0, 2), np.int32), "height": []}, 0.1, 1), [1])


def test_finish_rejects_what_is_not_a_tree():
    for id_lo, id_hi, height in (([0, 0], [1, 2], [0.1, 0.2]),            # node 0 a child twice
                                 ([0, 4], [1, 2], [0.1, 0.2]),            # cluster 4 does not exist yet at step 1
                                 ([0, 3], [1, 2], [0.1, np.nan])):
        with pytest.raises(N.NetRepError) as ei:
            N.hclustFinish(3, id_lo, id_hi, height)
        assert ei.value.code == L.NR_ERR_INVALID


# 2: the restated chain against scipy ----------------------------------------

@pytest.fixture(scope="module", params=[97, 600])
def tom_case(request):
    n = request.param
    x, which = H.module_data(n, 40, 100 + n)
    d = 1.0 - T.tom(np.abs(np.corrcoef(x, rowvar=False)) ** 5)
    d = np.maximum(d, d.T)                                                # exactly symmetric
    np.fill_diagonal(d, 0.0)
    return n, d, which


def scipy_tree_with_gaps(n, d):
    """scipy's average linkage of d, after the precondition that makes its
    tree THE tree: consecutive heights differ by more than 1,000 bars, so no
    rounding-level tie can excuse another one."""
    Z = scipy_hierarchy.linkage(squareform(d, checks=False), "average")
    h = Z[:, 2]
    gaps = np.diff(h) / h[1:]
    print(f"n = {n}: smallest relative height gap {gaps.min():.3e}, 1,000 bars = {1e3 * H.height_bar(n):.3e}")
    assert gaps.min() > 1e3 * H.height_bar(n)
    return Z


def assert_same_tree(n, got, exp, what):
    """Same set of clusters, heights within the bar."""
    assert set(got) == set(exp), f"{what}: {len(set(got) ^ set(exp))} clusters differ"
    worst = max(abs(got[k] - exp[k]) / exp[k] for k in exp)
    print(f"{what}: worst relative height error {worst:.3e} (bar {H.height_bar(n):.3e})")
    assert worst <= H.height_bar(n), what
    return worst


def test_chain_against_scipy(tom_case):
    n, d, _which = tom_case
    Z = scipy_tree_with_gaps(n, d)
    id_lo, id_hi, height, size, searches = H.chain(d)
    print(f"n = {n}: {searches / n:.2f} searches per node")
    assert searches < 3 * n
    assert_same_tree(n, H.clusters(n, zip(id_lo, id_hi), height), H.clusters(n, Z[:, :2], Z[:, 2]), f"chain n={n}")
    np.testing.assert_array_equal(size, [len(c) for c in H.clusters(n, zip(id_lo, id_hi), height)])
    merge, h, order, repairs = _assert_finish_matches_ref(n, id_lo, id_hi, height, f"finish n={n}")
    assert repairs == 0
    assert_same_tree(n, H.clusters_of_merge(n, merge, h), H.clusters(n, Z[:, :2], Z[:, 2]), f"merge n={n}")
    # a leaf order consistent with the tree: every cluster is a contiguous run of it
    pos = np.empty(n, np.int64)
    pos[order - 1] = np.arange(n)
    for c in H.clusters_of_merge(n, merge, h):
        p = pos[list(c)]
        assert p.max() - p.min() == len(c) - 1
    # the static cut inside the largest gap, both ways
    at = int(np.argmax(np.diff(h)))
    cut = 0.5 * (h[at] + h[at + 1])
    got = N.cutreeStatic({"merge": merge, "height": h}, cut, 3)
    np.testing.assert_array_equal(got, H.cutree_static(n, merge, h, cut, 3))
    sp = scipy_hierarchy.cut_tree(Z, height=cut).ravel()
    big = got > 0
    assert big.any()
    pairs = set(zip(got[big].tolist(), sp[big].tolist()))                 # the same partition of those nodes
    assert len(pairs) == len(set(got[big].tolist())) == len(set(sp[big].tolist()))


# 3: the committed scipy fixture ---------------------------------------------

@pytest.fixture(scope="module")
def small():
    with np.load(os.path.join(GOLDEN, "hclust_small.npz"), allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def test_against_the_committed_scipy_tree(small):
    d, Z, cut = small["d"], small["Z"], float(small["cut_height"])
    n = d.shape[0]
    assert n == 12
    id_lo, id_hi, height, _size, _searches = H.chain(d)
    exp = H.clusters(n, Z[:, :2], Z[:, 2])
    assert_same_tree(n, H.clusters(n, zip(id_lo, id_hi), height), exp, "ref chain vs fixture")
    merge, h, _order, _r = _assert_finish_matches_ref(n, id_lo, id_hi, height, "fixture")
    assert_same_tree(n, H.clusters_of_merge(n, merge, h), exp, "library finish vs fixture")
    # scipy numbers its clusters by first appearance too (from 0)
    for labels in (N.cutreeStatic({"merge": merge, "height": h}, cut, 1), H.cutree_static(n, merge, h, cut, 1)):
        part = set(zip(labels.tolist(), small["cut_labels"].tolist()))
        assert len(part) == len(set(labels.tolist())) == len(set(small["cut_labels"].tolist())) == 3
    # the library's finishing of scipy's own tree gives scipy's clusters back
    m2, h2, _o2, r2 = N.hclustFinish(n, Z[:, 0].astype(np.int32), Z[:, 1].astype(np.int32), Z[:, 2])
    assert r2 == 0
    assert H.clusters_of_merge(n, m2, h2) == exp


# 4: the static cut -----------------------------------------------------------

def test_static_cut_small_clusters_and_relabelling():
    # nodes 0..9: {0, 1}, {2, 3, 4}, {5, 6, 7}, {8}, {9} below the cut
    n = 10
    id_lo = [0, 2, 10 + 1, 5, 10 + 3, 10 + 0, 10 + 5, 10 + 6, 10 + 7]
    id_hi = [1, 3, 4, 6, 7, 10 + 2, 10 + 4, 8, 9]
    height = [0.1, 0.1, 0.2, 0.15, 0.25, 0.6, 0.7, 0.8, 0.9]
    merge, h, _order, _r = _assert_finish_matches_ref(n, id_lo, id_hi, height, "cut")
    tree = {"merge": merge, "height": h}
    for cut, min_size, exp in ((0.5, 1, [3, 3, 1, 1, 1, 2, 2, 2, 4, 5]),      # by size; {2,3,4} before {5,6,7} (tie)
                               (0.5, 3, [0, 0, 1, 1, 1, 2, 2, 2, 0, 0]),      # small clusters become 0
                               (0.5, 4, [0] * 10),
                               (0.2, 1, [2, 2, 1, 1, 1, 3, 3, 4, 5, 6]),       # exactly at a height: that merge is applied
                               (0.05, 1, list(range(1, 11))),
                               (0.65, 1, [1, 1, 1, 1, 1, 2, 2, 2, 3, 4]),
                               (1.0, 1, [1] * 10)):
        got = N.cutreeStatic(tree, cut, min_size)
        np.testing.assert_array_equal(got, H.cutree_static(n, merge, h, cut, min_size), err_msg=f"{cut} {min_size}")
        np.testing.assert_array_equal(got, exp, err_msg=f"{cut} {min_size}")
    bad = merge.copy()
    bad[0, 0] = 5                                                            # a row that refers to a later row
    with pytest.raises(N.NetRepError) as ei:
        N.cutreeStatic({"merge": bad, "height": h}, 0.5, 1)
    assert ei.value.code == L.NR_ERR_INVALID


# 5: the termination guard's host-side arithmetic ------------------------------

def test_guard_arithmetic_and_error_words():
    lib = L.load()
    cap = C.c_int64()
    for n in (1, 2, 97, 20000, 2 ** 30):
        assert lib.nr_hclust_search_cap(n, C.byref(cap)) == L.NR_OK
        assert cap.value == 4 * n + 16 == H.search_cap(n)
    assert lib.nr_hclust_search_cap(0, C.byref(cap)) == L.NR_ERR_INVALID
    buf = C.create_string_buffer(256)
    texts = {}
    for word in (1, 2, 3):
        assert lib.nr_hclust_error_message(word, buf, 256) == L.NR_OK
        texts[word] = buf.value.decode()
    assert "search cap" in texts[1] and "4 n + 16" in texts[1]
    assert "no finite" in texts[2]
    assert "chain" in texts[3]
    assert len(set(texts.values())) == 3
    for word in (0, 4, -1):
        assert lib.nr_hclust_error_message(word, buf, 256) == L.NR_ERR_INVALID
    assert lib.nr_hclust_error_message(1, buf, 8) == L.NR_ERR_INVALID      # too small: refused, not truncated
