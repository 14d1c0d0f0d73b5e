"""Eigengenes, module membership, close-module merging and kME trimming on a
resident from-data dataset (nr_module_eigengenes, nr_module_membership, the
netrep_Dataset* entries behind FromDataDataset): against the numpy
restatement, bit for bit against net_props where the kernels are the same,
independence of the kME cells from the tiling, the merge loop and the
trimming end to end, and that nothing resident changes."""
import numpy as np
import pytest

import netrep_amd as N
from netrep_amd import _lib as L
from netrep_amd.api import RMatrix

import modmerge_ref as R
from conftest import assert_stats_close
from test_modmerge_host import LARGE, MARGIN, SMALL, planted_case

pytestmark = pytest.mark.gpu

BETA = 5.0
KME_ATOL = 1e-12          # the project's absolute floor, 1e-10 x 1e-2


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _names(n):
    return [f"g{i}" for i in range(n)]


def _sizes37():
    return [int(v) for v in np.linspace(26, 5, 37)]


# (n, S, module sizes, links): S below a wave and odd; S over two waves' worth and no multiple of 64 with
# M = 37 over any eigengene tile; a 400-node module for the dual-Gram profile path; n never a multiple of 16.
SHAPES = {
    "97x23x3": (97, 23, [13, 12, 10], {}),
    "600x40x7": (LARGE["n"], LARGE["s"], LARGE["sizes"], R.SEVEN_LINKS),
    "600x130x37": (600, 130, _sizes37(), {}),
    "600x40+400": (600, 40, [400, 30, 26, 22], {}),
}
_CACHE = {}


def case(key):
    """Data, labels and the restatement of a shape, computed once and shared."""
    if key not in _CACHE:
        n, s, sizes, links = SHAPES[key]
        x, labels = R.planted(n, s, sizes, links, seed=11)
        ref = R.module_eigengenes(R.scale(x), labels)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _CACHE[key] = (x, labels, ref)
    return _CACHE[key]


def _csr(labels):
    mods = R.modules_of(labels)
    idx = [np.flatnonzero(labels == m) for m in mods]
    return np.cumsum([0] + [i.size for i in idx]).astype(np.int64), np.concatenate(idx).astype(np.int32)


def _assignments(labels):
    return {f"g{i}": str(int(lab)) for i, lab in enumerate(labels)}


# 1 -------------------------------------------------------------------------

@pytest.mark.parametrize("key", sorted(SHAPES))
def test_eigengenes_against_the_restatement_and_net_props(key):
    x, labels, ref = case(key)
    n = labels.size
    assert ref["gap"] > 0.05, "precondition: every module's top two singular values differ by more than 5 %"
    sel = labels > 0
    with N.FromDataDataset(RMatrix(x, None, _names(n)), BETA) as ds:
        got = ds.module_eigengenes(labels)
        mods = [str(int(m)) for m in ref["modules"]]
        props = ds.net_props(_assignments(labels), mods)
    np.testing.assert_array_equal(got["modules"], ref["modules"])
    worst = max(assert_stats_close(got["eigengenes"], ref["eigengenes"], what="eigengenes"),
                assert_stats_close(got["varExplained"], ref["varExplained"], what="varExplained"),
                assert_stats_close(got["kME"][sel], ref["kME"][sel], what="own kME"))
    print(f"{key}: worst scaled error against the restatement {worst:.3e}")
    assert np.isnan(got["kME"][~sel]).all()
    # the same kernels as net_props on the same handle: the same bits
    for j, m in enumerate(mods):
        np.testing.assert_array_equal(_bits(got["eigengenes"][:, j]), _bits(props[m]["summary"]), err_msg=m)
        np.testing.assert_array_equal(_bits(got["kME"][labels == int(m)]), _bits(props[m]["contribution"]), err_msg=m)
        assert _bits(got["varExplained"][j:j + 1])[0] == _bits(np.array([props[m]["coherence"]]))[0], m


# 2 -------------------------------------------------------------------------

def _check_table(kme, data, eig, labels, own, what):
    """kme against the restatement from the GPU's own eigengenes and the
    dataset's own data, and each module's own column against its own kME."""
    exp = R.cor_columns(data, eig)
    err = float(np.abs(kme - exp).max())
    mods = R.modules_of(labels)
    own_err = max(float(np.abs(kme[labels == m, j] - own[labels == m]).max()) for j, m in enumerate(mods))
    print(f"{what}: worst absolute kME error {err:.3e}, own column against own kME {own_err:.3e} (bar {KME_ATOL:.0e})")
    assert err <= KME_ATOL and own_err <= KME_ATOL, what


@pytest.mark.parametrize("key", sorted(SHAPES))
def test_membership_table(key):
    x, labels, _ref = case(key)
    n = labels.size
    with N.FromDataDataset(RMatrix(x, None, _names(n)), BETA) as ds:
        e = ds.module_eigengenes(labels)
        table = ds.module_membership(labels)
    assert table.rownames == _names(n) and table.colnames == [f"kME{int(m)}" for m in e["modules"]]
    _check_table(table.values, R.scale(x), e["eigengenes"], labels, e["kME"], key)


@pytest.mark.parametrize("kw", [dict(scaleData=False), dict(corType="spearman")], ids=["unscaled", "spearman"])
def test_membership_table_reads_the_data_as_stored(kw):
    x, labels, _ref = case("97x23x3")
    x = np.asfortranarray(x * np.linspace(0.5, 3.0, x.shape[1]) + 2.0)      # neither centred nor unit variance
    with N.FromDataDataset(RMatrix(x, None, _names(labels.size)), BETA, **kw) as ds:
        e = ds.module_eigengenes(labels)
        table = ds.module_membership(labels)
    stored = x if kw.get("scaleData") is False else R.scale(x)
    _check_table(table.values, stored, e["eigengenes"], labels, e["kME"], str(kw))


# every path of membership_tile: 4, 2 and 1 eigengenes per thread with the columns resident (S <= 229, 383,
# 575), their last sizes, and the chunked walk beyond (one chunk and a remainder; two chunks and a remainder)
@pytest.mark.parametrize("s", [3, 229, 230, 383, 384, 575, 576, 1100])
def test_membership_at_every_tile_rule(s):
    n, m = 35, 19                                    # three workgroups, the last with 3 nodes; M over a 16-tile
    rng = np.random.default_rng(s)
    x = np.asfortranarray(rng.standard_normal((s, n)) + rng.standard_normal(n))
    eig = np.asfortranarray(rng.standard_normal((s, m)) + 0.5)
    with N.Engine(0) as eng:
        eng.set_dataset_from_data(x, BETA, scale=False)
        kme = eng.module_membership(m, eig)
        one = eng.module_membership(1, eig[:, 7:8])
    err = float(np.abs(kme - R.cor_columns(x, eig)).max())
    print(f"S={s}: worst absolute kME error {err:.3e}")
    assert err <= KME_ATOL
    np.testing.assert_array_equal(_bits(one[:, 0]), _bits(kme[:, 7]))


# 3 -------------------------------------------------------------------------

def test_cells_do_not_depend_on_the_tiling():
    x, labels, _ref = case("600x130x37")
    s, m = x.shape[0], 37
    node_off, idx = _csr(labels)
    with N.Engine(0) as eng:
        eng.set_dataset_from_data(x, BETA)
        e = eng.module_eigengenes(node_off, idx)
        whole = eng.module_membership(m)
        assert eng.membership_ms() > 0.0
        eig = e["eigengenes"]
        for j in range(m):
            alone = eng.module_membership(1, eig[:, j:j + 1])
            np.testing.assert_array_equal(_bits(alone[:, 0]), _bits(whole[:, j]), err_msg=f"column {j} alone")
        rev = eng.module_membership(m, eig[:, ::-1])
        np.testing.assert_array_equal(_bits(rev[:, ::-1]), _bits(whole), err_msg="reversed order")
        before = N.h2d_bytes()
        host = eng.module_membership(m, eig)
        assert N.h2d_bytes() - before == 8 * s * m
        np.testing.assert_array_equal(_bits(host), _bits(whole), err_msg="host-supplied eigengenes")
        np.testing.assert_array_equal(_bits(eng.module_membership(m)), _bits(whole), err_msg="kept eigengenes again")
        # the kept eigengenes belong to a dataset and a module count
        with pytest.raises(N.NetRepError) as ei:
            eng.module_membership(m - 1)
        assert ei.value.code == L.NR_ERR_INVALID
        eng.set_dataset_from_data(x, BETA)
        with pytest.raises(N.NetRepError) as ei:
            eng.module_membership(m)
        assert ei.value.code == L.NR_ERR_INVALID


# 4 -------------------------------------------------------------------------

@pytest.mark.parametrize("which,cut,relabel", [("small", 0.25, True), ("large", 0.30, False), ("large", 0.25, True)])
def test_merge_close_modules_against_the_restated_loop(which, cut, relabel):
    x, labels = planted_case(which, cut)
    shape = SMALL if which == "small" else LARGE
    assert (labels == 0).sum() == shape["n"] - sum(shape["sizes"]) > 0
    for cut_height, rounds in ((cut, 2), (0.02, 0)):
        exp = R.merge_close_modules(R.scale(x), labels, cut_height, relabel=relabel)
        # preconditions, on the restatement alone
        assert R.margin(exp["all_heights"], cut_height) >= MARGIN and exp["rounds"] == rounds
        with N.FromDataDataset(RMatrix(x, None, _names(labels.size)), BETA) as ds:
            got = ds.merge_close_modules(labels, cut_height, relabel=relabel)
        np.testing.assert_array_equal(got["labels"], exp["labels"])
        assert got["rounds"] == exp["rounds"]
        assert R.grouping_of(labels, got["labels"]) == R.grouping_of(labels, exp["labels"])
        assert (got["labels"][labels == 0] == 0).all()
        err = float(np.abs(got["heights"] - exp["heights"]).max())
        print(f"{which} cut {cut_height} relabel {relabel}: worst last-round height error {err:.3e}")
        assert got["heights"].shape == exp["heights"].shape and err <= 1e-9
        assert_stats_close(got["eigengenes"], exp["eigengenes"], what="last round's eigengenes")
        if rounds == 0 and not relabel:
            np.testing.assert_array_equal(got["labels"], labels)


# 5 -------------------------------------------------------------------------

def test_trim_modules_against_the_restatement():
    n, s, sizes = 300, 40, [40, 34, 28, 22, 9]
    x, labels = R.planted(n, s, sizes, {}, seed=21, n_noise_inside=3)
    ref = R.module_eigengenes(R.scale(x), labels)
    own = ref["kME"][labels > 0]
    for kw in (dict(min_size=8), dict(min_size=8, min_kme_to_stay=0.5, min_core_kme=0.8),
               dict(min_size=30), dict(min_size=8, min_core_kme=0.9, min_core_kme_size=25)):
        stay, core = kw.get("min_kme_to_stay", 0.3), kw.get("min_core_kme", 0.5)
        assert min(np.abs(own - stay).min(), np.abs(own - core).min()) > 1e-6, "precondition: no kME at a threshold"
        exp = R.trim_modules(labels, ref["kME"], **kw)
        with N.FromDataDataset(RMatrix(x, None, _names(n)), BETA) as ds:
            got = ds.trim_modules(labels, kw["min_size"], stay, core, kw.get("min_core_kme_size"))
        np.testing.assert_array_equal(got, exp, err_msg=str(kw))
    base = R.trim_modules(labels, ref["kME"], min_size=8)
    assert 0 < (base != labels).sum() < (labels > 0).sum()         # the noise genes go, the modules stay
    assert (R.trim_modules(labels, ref["kME"], min_size=30)[labels == 5] == 0).all()


# 6 -------------------------------------------------------------------------

def test_nothing_resident_changes():
    x, labels = planted_case("small", 0.25)
    names = _names(labels.size)
    ma = _assignments(labels)
    mods = [str(int(m)) for m in R.modules_of(labels)]

    def snapshot(ds):
        corr, net = ds.matrices()
        props = ds.net_props(ma, mods)
        tree = ds.hclust()
        disc = ds.intermediate_properties(names, ma, mods)
        perm = ds.permutation_procedure(disc, ma, mods, 64, seed=5)
        flat = [corr.values, net.values, tree["height"], tree["merge"].astype(np.float64), perm["observed"],
                perm["nulls"]]
        for m in mods:
            flat += [props[m]["degree"], props[m]["summary"], props[m]["contribution"]]
        return [_bits(a).copy() for a in flat]

    with N.FromDataDataset(RMatrix(x, None, names), BETA) as ds:
        before = snapshot(ds)
        ds.module_eigengenes(labels)
        ds.module_membership(labels)
        ds.merge_close_modules(labels, 0.25)
        ds.trim_modules(labels, 4)
        after = snapshot(ds)
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a, b)
    node_off, idx = _csr(labels)
    with N.Engine(0) as eng:
        eng.set_dataset_from_data(x, BETA)
        eng.release_scratch()
        held = eng.scratch_bytes()
        eng.module_eigengenes(node_off, idx)
        assert eng.scratch_bytes() >= held + 8 * x.shape[0] * (node_off.size - 1)     # the kept eigengenes count
        eng.module_membership(node_off.size - 1)
        eng.release_scratch()
        assert eng.scratch_bytes() == held
        with pytest.raises(N.NetRepError):
            eng.module_membership(node_off.size - 1)                                  # released with the scratch


# 7 -------------------------------------------------------------------------

def test_detect_modules_defaults_are_unchanged():
    x, labels = planted_case("small", 0.25)
    data = RMatrix(x, None, _names(labels.size))
    res = N.DetectModulesFromData(data, BETA, 0.9, minSize=4)
    with N.FromDataDataset(data, BETA, tom=True) as ds:
        tree = ds.hclust()
    exp = N.cutreeStatic(tree, 0.9, 4)
    assert set(res) == {"moduleAssignments", "tree"}
    assert res["moduleAssignments"] == {nm: str(int(lab)) for nm, lab in zip(tree["labels"], exp)}
    assert set(res["tree"]) == set(tree)
    for k in ("merge", "height", "order"):
        np.testing.assert_array_equal(res["tree"][k], tree[k])
    assert res["tree"]["labels"] == tree["labels"] and res["tree"]["n_repairs"] == tree["n_repairs"]


def test_detect_trim_merge_then_preservation():
    n, s, sizes = LARGE["n"], LARGE["s"], LARGE["sizes"]
    # tight modules (noise 0.2): the adjacency tree tells the planted pair 1, 2 (factors correlated at 0.95) apart
    x, planted = R.planted(n, s, sizes, R.SEVEN_LINKS, seed=75, noise=0.2)
    x2, _ = R.planted(n, s, sizes, R.SEVEN_LINKS, seed=1234, noise=0.2)     # the same modules in a second dataset
    names = _names(n)
    disc, test = RMatrix(x, None, names), RMatrix(x2, None, names)
    tree = N.DetectModulesFromData(disc, BETA, 0.5, minSize=6, tom=False)["tree"]

    def module_of(labels, m):
        """The detected label that holds at least 80 % of planted module m, or None."""
        vals, counts = np.unique(labels[planted == m], return_counts=True)
        top = int(np.argmax(counts))
        return int(vals[top]) if vals[top] > 0 and counts[top] >= 0.8 * (planted == m).sum() else None

    # precondition: the highest cut of a fixed grid at which the static cut holds planted 1 and 2 as two modules
    cut = None
    for c in np.linspace(0.999, 0.2, 400):
        static = N.cutreeStatic(tree, float(c), 6)
        if None not in (module_of(static, 1), module_of(static, 2)) and module_of(static, 1) != module_of(static, 2):
            cut = float(c)
            break
    assert cut is not None, "precondition: a static cut that splits the planted pair"
    res = N.DetectModulesFromData(disc, BETA, cut, minSize=6, tom=False, mergeCutHeight=0.25, minKMEtoStay=0.3)
    assert set(res) == {"moduleAssignments", "tree", "unmergedAssignments", "eigengenes", "rounds"}
    unmerged = np.array([int(res["unmergedAssignments"][nm]) for nm in names])
    merged = np.array([int(res["moduleAssignments"][nm]) for nm in names])
    n_before, n_after = R.modules_of(unmerged).size, R.modules_of(merged).size
    print(f"cut {cut:.4f}: {n_before} modules before the merge, {n_after} after, {res['rounds']} rounds")
    assert module_of(unmerged, 1) != module_of(unmerged, 2)
    assert res["rounds"] >= 1 and n_after < n_before
    assert module_of(merged, 1) == module_of(merged, 2) is not None
    assert res["eigengenes"].shape == (s, n_after)
    assert ((merged == 0) == (unmerged == 0)).all()                         # the merge assigns and drops nobody
    assert R.modules_of(merged).tolist() == list(range(1, n_after + 1))      # relabelled by size
    out = N.modulePreservationFromData({"d": disc, "t": test}, BETA, {"d": res["moduleAssignments"]}, nPerm=64)
    r = out["d"]["t"]
    assert r["modules"] == [str(k) for k in range(1, n_after + 1)]
    assert r["nulls"].shape == (n_after, 7, 64)
    assert np.isfinite(r["observed"]).all() and np.isfinite(r["nulls"]).all() and np.isfinite(r["p.values"]).all()
    N.ReleaseResident()


# 8 -------------------------------------------------------------------------

def test_edge_cases():
    rng = np.random.default_rng(9)
    s, n = 23, 40
    f = rng.standard_normal(s)
    x = rng.standard_normal((s, n))
    x[:, :12] = f[:, None] + 0.3 * rng.standard_normal((s, 12))
    x[:, 12:24] = f[:, None] + 0.3 * rng.standard_normal((s, 12))       # the same factor: they merge into one
    x = np.asfortranarray(x)
    one = np.zeros(n, dtype=np.int32)
    one[:12] = 3
    two = one.copy()
    two[12:24] = 8
    single = np.zeros(n, dtype=np.int32)
    single[30] = 2
    ds = N.FromDataDataset(RMatrix(x, None, _names(n)), BETA)
    try:
        r = ds.merge_close_modules(one, 0.25, relabel=False)
        np.testing.assert_array_equal(r["labels"], one)
        assert r["rounds"] == 0 and r["eigengenes"].shape == (s, 1) and r["heights"].size == 0
        exp = R.merge_close_modules(R.scale(x), two, 0.25, relabel=False)
        assert exp["rounds"] == 1 and R.margin(exp["all_heights"], 0.25) >= MARGIN
        r = ds.merge_close_modules(two, 0.25, relabel=False)
        np.testing.assert_array_equal(r["labels"], exp["labels"])
        assert r["rounds"] == 1 and R.modules_of(r["labels"]).tolist() == [3] and r["eigengenes"].shape == (s, 1)
        assert ds.merge_close_modules(two, 0.25, relabel=True)["labels"].max() == 1
        # a module of one node: its eigengene is the column normalised
        e = ds.module_eigengenes(single)
        col = R.scale(x)[:, 30]
        assert_stats_close(e["eigengenes"][:, 0], col / np.linalg.norm(col), what="one-node eigengene")
        assert abs(e["kME"][30] - 1.0) <= 1e-12 and abs(e["varExplained"][0] - 1.0) <= 1e-12
        assert abs(ds.module_membership(single).values[30, 0] - 1.0) <= KME_ATOL
        for bad, text in ((np.where(one > 0, -1, 0), "negative label"), (np.zeros(n, dtype=np.int32), "no positive label")):
            for call in (ds.module_eigengenes, ds.module_membership, ds.merge_close_modules,
                         lambda lab: ds.trim_modules(lab, 4)):
                with pytest.raises(N.NetRepError) as ei:
                    call(bad)
                assert ei.value.code == L.NR_ERR_INVALID and text in str(ei.value)
        for cut in (-0.01, 2.5, float("nan")):
            with pytest.raises(N.NetRepError) as ei:
                ds.merge_close_modules(one, cut)
            assert ei.value.code == L.NR_ERR_INVALID and "cut_height" in str(ei.value)
    finally:
        ds.close()
    for call in (ds.module_eigengenes, ds.module_membership, ds.merge_close_modules, lambda lab: ds.trim_modules(lab, 4)):
        with pytest.raises(N.NetRepError) as ei:
            call(one)
        assert ei.value.code == L.NR_ERR_INVALID
