"""CPU tests of the host rules that follow the eigengenes: the eigengene tree
and its cut (netrep_EigengeneGroups) against the restatement bit for bit and
against scipy's average linkage, the label rules (netrep_MergeLabels,
netrep_TrimModulesKME) against the restatement, the restated
mergeCloseModules loop on planted data, and the invalid arguments."""
import ctypes as C

import numpy as np
import pytest

import netrep_amd as N
from netrep_amd import _lib as L

import hclust_ref as H
import modmerge_ref as R

import scipy.cluster.hierarchy as scipy_hierarchy  # noqa: E402
from scipy.spatial.distance import squareform  # noqa: E402

# R.find_seed(n, s, sizes, R.SEVEN_LINKS, cut, rounds=2, grouping=R.SEVEN_GROUPING)
# picked these; every test that uses one asserts the preconditions itself.
SMALL = dict(n=97, s=23, sizes=[13, 12, 10, 9, 7, 6, 4])
LARGE = dict(n=600, s=40, sizes=[30, 26, 22, 18, 15, 12, 9])
TWO_ROUND_SEEDS = {("small", 0.25): 48, ("small", 0.30): 16, ("large", 0.25): 75, ("large", 0.30): 4}
MARGIN = 0.01


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def planted_case(which, cut):
    shape = SMALL if which == "small" else LARGE
    return R.planted(shape["n"], shape["s"], shape["sizes"], R.SEVEN_LINKS, TWO_ROUND_SEEDS[(which, cut)])


def _partition(group):
    out = {}
    for m, g in enumerate(group):
        out.setdefault(int(g), set()).add(m)
    return sorted(map(frozenset, out.values()), key=min)


def _check_groups(eig, cut, what):
    group, heights = N.eigengeneGroups(eig, cut)
    e_group, e_heights = R.eigengene_groups(eig, cut)
    np.testing.assert_array_equal(group, e_group, err_msg=what)
    np.testing.assert_array_equal(_bits(heights), _bits(e_heights), err_msg=what)
    return group, heights


# 1: groups and heights -------------------------------------------------------

@pytest.mark.parametrize("s,m,seed", [(23, 3, 1), (40, 7, 2), (130, 37, 3), (5, 2, 4)])
def test_groups_against_the_restatement_and_scipy(s, m, seed):
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((s, max(m // 3, 1)))
    eig = np.asfortranarray(base[:, rng.integers(0, base.shape[1], m)] + 0.6 * rng.standard_normal((s, m)))
    # scipy links the dissimilarities of the stated definition, so the comparison is of the linkage alone
    d = np.array(R.eigengene_dissimilarity(eig))
    Z = scipy_hierarchy.linkage(squareform(d, checks=False), "average")
    zh = Z[:, 2]
    between = float(zh[zh.size // 2 - 1] + zh[zh.size // 2]) / 2 if zh.size > 1 else float(zh[0]) / 2
    for cut in (0.25, between, 1.5):
        # precondition: no scipy height within 1e-9 of the cut, so rounding cannot move a merge across it
        assert np.abs(Z[:, 2] - cut).min() > 1e-9
        group, heights = _check_groups(eig, cut, f"S={s} M={m} cut={cut}")
        flat = scipy_hierarchy.fcluster(Z, cut, "distance")
        assert _partition(group) == _partition(flat), (s, m, cut)
        worst = (np.abs(np.sort(heights) - Z[:, 2]) / Z[:, 2]).max()
        print(f"S={s} M={m}: worst relative height error {worst:.3e} (bar {H.height_bar(m):.3e})")
        assert worst <= H.height_bar(m)


def test_one_module_two_modules_identical_and_opposite():
    rng = np.random.default_rng(5)
    e = rng.standard_normal((12, 1))
    group, heights = _check_groups(e, 0.25, "M=1")
    assert group.tolist() == [0] and heights.size == 0
    a = rng.standard_normal(12)
    b = rng.standard_normal(12)
    group, heights = _check_groups(np.column_stack([a, b]), 0.25, "M=2")
    assert heights.size == 1 and group.tolist() == ([0, 0] if heights[0] <= 0.25 else [0, 1])
    group, heights = _check_groups(np.column_stack([a, a, b]), 0.0, "identical pair")
    assert heights[0] == 0.0 and group.tolist() == [0, 0, 2]      # d = 0 merges at cut 0 (<=)
    group, heights = _check_groups(np.column_stack([a, -a]), 1.0, "opposite pair")
    assert heights[0] == 2.0 and group.tolist() == [0, 1]
    group, _ = _check_groups(np.column_stack([a, -a]), 2.0, "opposite pair at cut 2")
    assert group.tolist() == [0, 0]


def test_cut_exactly_at_a_height_merges():
    rng = np.random.default_rng(6)
    eig = np.asfortranarray(rng.standard_normal((30, 5)))
    _g, heights = R.eigengene_groups(eig, 0.0)
    for t in (0, 2):
        group, _h = _check_groups(eig, float(heights[t]), f"cut at height {t}")
        assert len(_partition(group)) == 5 - (t + 1)
        group, _h = _check_groups(eig, float(np.nextafter(heights[t], -np.inf)), f"cut below height {t}")
        assert len(_partition(group)) == 5 - t


def test_ties_go_to_the_lowest_pair():
    # orthogonal +-1 patterns: every pair of distinct columns has d = 1 exactly,
    # copies have d = 0 exactly: columns (0, 3) and (1, 2) tie at 0, then all tie at 1
    h = np.array([[1, 1, 1, 1, -1, -1, -1, -1], [1, 1, -1, -1, 1, 1, -1, -1], [1, -1, 1, -1, 1, -1, 1, -1]], float).T
    eig = np.column_stack([h[:, 0], h[:, 1], h[:, 1], h[:, 0], h[:, 2]])
    group, heights = _check_groups(eig, 0.5, "ties")
    assert heights.tolist() == [0.0, 0.0, 1.0, 1.0]
    assert group.tolist() == [0, 1, 1, 0, 4]
    # at cut 1 everything joins the cluster of column 0
    group, _ = _check_groups(eig, 1.0, "ties at cut 1")
    assert group.tolist() == [0, 0, 0, 0, 0]


# 2: label rules ----------------------------------------------------------------

def test_merge_labels_against_the_restatement():
    labels = np.array([0, 1, 1, 1, 2, 2, 3, 3, 3, 3, 0, 4, 5, 5, 5, 5], dtype=np.int32)
    mods = R.modules_of(labels)
    for group in ([0, 1, 2, 3, 4], [0, 0, 2, 3, 4], [0, 1, 1, 3, 1], [0, 0, 0, 0, 0], [0, 1, 2, 2, 4]):
        for relabel in (False, True):
            got = N.mergeLabels(labels, mods, group, relabel)
            np.testing.assert_array_equal(got, R.merge_labels(labels, mods, group, relabel), err_msg=str(group))
            assert (got[labels == 0] == 0).all() and (got[labels > 0] > 0).all()
    # the label of a group is its first module's
    assert N.mergeLabels(labels, mods, [0, 1, 1, 3, 1]).tolist() == [0, 1, 1, 1, 2, 2, 2, 2, 2, 2, 0, 4, 2, 2, 2, 2]
    # relabelling: sizes 3 (label 1), 2 + 4 = 6 (label 2), 1 (label 4), 4 (label 5) -> 2 -> 1, 5 -> 2, 1 -> 3, 4 -> 4
    assert N.mergeLabels(labels, mods, [0, 1, 1, 3, 4], True).tolist() == [0, 3, 3, 3, 1, 1, 1, 1, 1, 1, 0, 4, 2, 2, 2, 2]
    # ties in size go to the lower old label: 3 and 7 both have two nodes
    tied = np.array([7, 7, 3, 3, 9, 9, 9], dtype=np.int32)
    assert N.mergeLabels(tied, [3, 7, 9], [0, 1, 2], True).tolist() == [3, 3, 2, 2, 1, 1, 1]


def test_trim_modules_against_the_restatement():
    labels = np.array([1] * 6 + [2] * 6 + [3] * 6 + [0] * 3 + [4] * 4, dtype=np.int32)
    kme = np.array([0.9, 0.8, 0.7, 0.6, 0.55, 0.2,        # 1: one node dropped, five stay
                    0.45, 0.4, 0.4, 0.35, 0.6, 0.31,      # 2: one core node only: dissolved at core size 2
                    0.9, 0.8, 0.1, 0.2, 0.25, 0.7,        # 3: three dropped, three left: under min_size 4
                    0.99, 0.99, 0.99,                     # 0: never touched
                    0.9, 0.9, -0.9, 0.9])                 # 4: a negative kME goes
    for kw in (dict(min_size=4), dict(min_size=4, min_core_kme_size=1), dict(min_size=3, min_kme_to_stay=0.5),
               dict(min_size=6, min_core_kme=0.85), dict(min_size=7), dict(min_size=2, min_core_kme_size=0)):
        got = N.trimModulesKME(labels, kme, kw["min_size"], kw.get("min_kme_to_stay", 0.3), kw.get("min_core_kme", 0.5),
                               kw.get("min_core_kme_size"))
        np.testing.assert_array_equal(got, R.trim_modules(labels, kme, **kw), err_msg=str(kw))
    got = N.trimModulesKME(labels, kme, 4)          # default core size: ceil(4 / 3) = 2
    assert got[:6].tolist() == [1, 1, 1, 1, 1, 0]
    assert (got[6:12] == 0).all()                    # one node above 0.5 < 2
    assert (got[12:18] == 0).all()                   # fell under min_size after the drops
    assert (got[18:21] == 0).all()
    assert (got[21:] == 0).all()                     # the negative kME goes, three left < min_size 4
    assert N.trimModulesKME(labels, kme, 3)[21:].tolist() == [4, 4, 0, 4]
    assert N.trimModulesKME(labels, kme, 4, minCoreKMESize=1)[6:12].tolist() == [2] * 6
    # the default is min_size / 3 as a count: 7 / 3 -> 3 core nodes needed; module 3 has exactly 3
    assert (N.trimModulesKME(labels, kme, 7, minKMEtoStay=-1.0)[12:18] == 0).all()       # 6 nodes < min_size 7
    seven = np.array([3] * 7, dtype=np.int32)
    k7 = np.array([0.9, 0.8, 0.7, 0.4, 0.4, 0.4, 0.4])
    assert N.trimModulesKME(seven, k7, 7).tolist() == [3] * 7
    k7[2] = 0.5                                      # not above 0.5: two core nodes < 3
    assert N.trimModulesKME(seven, k7, 7).tolist() == [0] * 7


# 3: the restated loop on planted data ------------------------------------------

@pytest.mark.parametrize("which,cut", sorted(TWO_ROUND_SEEDS))
def test_restated_loop_returns_the_planted_grouping_in_two_rounds(which, cut):
    x, labels = planted_case(which, cut)
    r = R.merge_close_modules(R.scale(x), labels, cut, relabel=False)
    heights = [np.round(h, 3).tolist() for h in r["all_heights"]]
    print(f"{which} cut {cut}: heights per round {heights}")
    assert R.margin(r["all_heights"], cut) >= MARGIN
    assert r["rounds"] == 2
    assert R.grouping_of(labels, r["labels"]) == sorted(R.SEVEN_GROUPING, key=min)
    assert (r["labels"][labels == 0] == 0).all()
    # the host entries walk the same rounds on the restated eigengenes
    cur = labels.copy()
    for _round in range(3):
        e = R.module_eigengenes(R.scale(x), cur)
        group, _h = N.eigengeneGroups(e["eigengenes"], cut)
        cur = N.mergeLabels(cur, e["modules"], group)
    np.testing.assert_array_equal(cur, r["labels"])
    # a cut under every height merges nothing
    r0 = R.merge_close_modules(R.scale(x), labels, 0.02, relabel=False)
    assert r0["rounds"] == 0 and R.margin(r0["all_heights"], 0.02) >= MARGIN
    np.testing.assert_array_equal(r0["labels"], labels)


# 4: invalid arguments ------------------------------------------------------------

def test_invalid_arguments():
    lib = L.load()
    e = np.asfortranarray(np.random.default_rng(7).standard_normal((10, 3)))
    g = np.zeros(3, dtype=np.int32)
    h = np.zeros(2)
    dp, ip = lambda a: a.ctypes.data_as(L._dp), lambda a: a.ctypes.data_as(L._i32p)  # noqa: E731
    for cut in (-0.1, 2.1, float("nan")):
        assert lib.netrep_EigengeneGroups(dp(e), 10, 3, cut, ip(g), dp(h)) == L.NR_ERR_INVALID
        assert b"cut_height" in lib.netrep_last_error()
    assert lib.netrep_EigengeneGroups(None, 10, 3, 0.25, ip(g), dp(h)) == L.NR_ERR_INVALID
    assert lib.netrep_EigengeneGroups(dp(e), 10, 0, 0.25, ip(g), dp(h)) == L.NR_ERR_INVALID
    const = e.copy(order="F")
    const[:, 1] = 3.0
    assert lib.netrep_EigengeneGroups(dp(const), 10, 3, 0.25, ip(g), dp(h)) == L.NR_ERR_INVALID
    labels = np.array([1, 2, 0, 2], dtype=np.int32)
    out = np.zeros(4, dtype=np.int32)
    mods = np.array([1, 2], dtype=np.int32)
    grp = np.array([0, 0], dtype=np.int32)
    assert lib.netrep_MergeLabels(4, ip(labels), 2, ip(mods), ip(grp), 0, ip(out)) == L.NR_OK
    neg = np.array([1, -2, 0, 2], dtype=np.int32)
    assert lib.netrep_MergeLabels(4, ip(neg), 2, ip(mods), ip(grp), 0, ip(out)) == L.NR_ERR_INVALID
    assert b"negative label" in lib.netrep_last_error()
    one = np.array([1], dtype=np.int32)
    assert lib.netrep_MergeLabels(4, ip(labels), 1, ip(one), ip(grp), 0, ip(out)) == L.NR_ERR_INVALID   # label 2 unknown
    fwd = np.array([1, 0], dtype=np.int32)
    assert lib.netrep_MergeLabels(4, ip(labels), 2, ip(mods), ip(fwd), 0, ip(out)) == L.NR_ERR_INVALID  # group[0] > 0
    kme = np.ones(4)
    assert lib.netrep_TrimModulesKME(4, ip(labels), dp(kme), 0.3, 0.5, -1, 1, ip(out)) == L.NR_OK
    assert lib.netrep_TrimModulesKME(4, ip(neg), dp(kme), 0.3, 0.5, -1, 1, ip(out)) == L.NR_ERR_INVALID
    assert lib.netrep_TrimModulesKME(4, ip(labels), dp(kme), float("nan"), 0.5, -1, 1, ip(out)) == L.NR_ERR_INVALID
    assert lib.netrep_TrimModulesKME(4, ip(labels), None, 0.3, 0.5, -1, 1, ip(out)) == L.NR_ERR_INVALID
    # the handle entries check their arguments before they touch a device
    for fn, args in (("netrep_DatasetModuleMembership", (None, None)),
                     ("netrep_DatasetTrimModules", (None, 0.3, 0.5, -1, 1, None))):
        assert getattr(lib, fn)(None, *args) == L.NR_ERR_INVALID
        assert b"no dataset" in lib.netrep_last_error()
    assert lib.netrep_DatasetMergeCloseModules(None, None, 0.25, 1, None, None, None, None, None) == L.NR_ERR_INVALID
    assert lib.netrep_DatasetModuleEigengenes(None, None, None, None, None, None, None) == L.NR_ERR_INVALID
    assert C.sizeof(C.c_int32) == 4
