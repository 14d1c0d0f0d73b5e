"""CPU tests of the resident from-data dataset's interface (netrep_Dataset*,
the two from-data one-shots, FromDataDataset, modulePreservationFromData): the
symbols through the header, the library and the bindings; the argument checks
that run before any context is opened (so they need no GPU); the Python
signatures; and the driver's loop with FromDataDataset replaced by a numpy
stand-in built from tests/netbuild_ref.py and oracle/netrep_oracle.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import netrep_amd as N
from netrep_amd import _lib as L
from netrep_amd import api as A
from netrep_amd.api import RMatrix
from netrep_amd.contingency import order_as_numeric
from netrep_amd.pvalues import permutationTest
from oracle import netrep_oracle as O

import netbuild_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HANDLE_ENTRIES = ["netrep_DatasetFromData", "netrep_DatasetRelease", "netrep_DatasetShape", "netrep_DatasetMatrices",
                  "netrep_DatasetIntermediateProperties", "netrep_DatasetNetProps",
                  "netrep_DatasetPermutationProcedure"]
ONE_SHOTS = ["netrep_IntermediatePropertiesFromData", "netrep_NetPropsFromData"]


def _header():
    hdr = open(os.path.join(ROOT, "include", "netrep_gpu.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


@pytest.mark.parametrize("name", HANDLE_ENTRIES + ONE_SHOTS)
def test_entry_in_header_library_and_signatures(name):
    m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, _header())
    assert m, name
    assert hasattr(L.load(), name)
    assert name in L.SIGNATURES
    declared = [a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"]
    res, args = L.SIGNATURES[name]
    assert len(declared) == len(args), (name, declared)
    assert (res is None) == bool(re.search(r"\bvoid\s+%s\s*\(" % name, _header()))


def test_the_handle_is_opaque_in_the_header():
    hdr = _header()
    assert re.search(r"typedef\s+struct\s+netrep_dataset\s+netrep_dataset\s*;", hdr)
    assert not re.search(r"struct\s+netrep_dataset\s*\{", hdr)
    full = open(os.path.join(ROOT, "include", "netrep_gpu.h")).read()
    assert re.search(r"netrep_ReleaseResident[\s*]+does[\s*]+NOT[\s*]+free[\s*]+live[\s*]+handles", full)


def test_integration_glue_for_the_handle():
    """INTEGRATION.md's Rcpp glue for the new entries: the handle is an external
    pointer whose finalizer releases it, every routine is exported, and the
    glue calls only functions the header declares."""
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    code = "\n".join(re.findall(r"```cpp\n(.*?)```", doc, flags=re.S))
    m = re.search(r"static\s+void\s+(\w+)\s*\(\s*netrep_dataset\s*\*\s*(\w+)\s*\)\s*\{\s*netrep_DatasetRelease\s*\(\s*\2\s*\)\s*;\s*\}", code)
    assert m, "no finalizer that calls netrep_DatasetRelease"
    assert re.search(r"Rcpp::XPtr<\s*netrep_dataset\s*,\s*Rcpp::PreserveStorage\s*,\s*%s\b" % m.group(1), code)
    exported = set(re.findall(r"//\s*\[\[Rcpp::export\]\]\s*\n\s*[\w:<>]+\s+(\w+)\s*\(", code))
    assert {"DatasetFromData", "DatasetRelease", "DatasetIntermediateProperties"} <= exported
    for name in ("netrep_DatasetFromData", "netrep_DatasetIntermediateProperties"):
        assert re.search(r"\b%s\s*\(" % name, code), name
    for name in HANDLE_ENTRIES + ONE_SHOTS:
        assert name in doc, name
    declared = set(re.findall(r"\b((?:nr|netrep)_[A-Za-z0-9_]+)\s*\(", _header()))
    used = set(re.findall(r"\b((?:nr|netrep)_[A-Za-z0-9_]+)\s*\(", code))
    assert used <= declared, used - declared


# -- argument checks, before any context is opened ---------------------------

_X = np.asfortranarray(np.random.default_rng(0).normal(size=(5, 3)))
_XP = _X.ctypes.data_as(L._dp)
_NAMES = (C.c_char_p * 3)(b"a", b"b", b"c")
_D = np.empty(16)
_DP = _D.ctypes.data_as(L._dp)
_I = np.zeros(4, dtype=np.int64)
_IP = _I.ctypes.data_as(L._i64p)


def _from_data(data=_XP, net_type=0, beta=5.0, s=5, names=_NAMES, out=True):
    h = C.c_void_p()
    rc = L.load().netrep_DatasetFromData(data, 1, net_type, beta, s, 3, names, 0, C.byref(h) if out else None)
    assert not h.value
    return rc


def _ip_from_data(data=_XP, net_type=0, beta=5.0, s=5, names=_NAMES, out=True):
    return L.load().netrep_IntermediatePropertiesFromData(
        data, 1, net_type, beta, s, 3, names, _NAMES, 3, _NAMES, _NAMES, 3, _NAMES, 1, _DP, _IP, _DP, _IP,
        _DP if out else None, _IP)


def _np_from_data(data=_XP, net_type=0, beta=5.0, s=5, names=_NAMES, out=True):
    return L.load().netrep_NetPropsFromData(
        data, 1, net_type, beta, s, 3, names, _NAMES, _NAMES, 3, _NAMES, 1, _DP, _DP, _DP, _DP, _DP,
        _IP if out else None)


FROM_DATA = [_from_data, _ip_from_data, _np_from_data]


@pytest.mark.parametrize("entry", FROM_DATA)
@pytest.mark.parametrize("kw,message", [
    (dict(data=None), "data missing"),
    (dict(s=1), "data needs n_samples >= 2 and n_nodes >= 1"),
    (dict(net_type=0x300), "unknown correlation type"),
    (dict(net_type=0x103), "unknown network type"),
    (dict(beta=0.0), "beta must be finite and > 0"),
    (dict(beta=-2.0), "beta must be finite and > 0"),
    (dict(beta=float("nan")), "beta must be finite and > 0"),
    (dict(out=False), "invalid arguments to "),
    (dict(names=None), "invalid arguments to "),
])
def test_from_data_entries_reject_before_a_context_opens(entry, kw, message):
    """The existing messages of check_from_data_args; a context that failed to
    open (there is no GPU here) would report the device instead."""
    rc = entry(**kw)
    msg = L.load().netrep_last_error().decode()
    assert rc == L.NR_ERR_INVALID and message in msg, (entry.__name__, kw, rc, msg)


def test_the_data_checks_come_first():
    assert _from_data(data=None, out=False) == L.NR_ERR_INVALID
    assert L.load().netrep_last_error().decode() == "data missing"


def test_release_of_null_is_safe():
    L.load().netrep_DatasetRelease(None)
    L.load().netrep_DatasetRelease(None)


def test_handle_entries_reject_a_null_handle():
    lib = L.load()
    dp = L.DiscProps()
    n, s = C.c_int64(), C.c_int64()
    calls = {
        "DatasetShape": lambda: lib.netrep_DatasetShape(None, C.byref(n), C.byref(s)),
        "DatasetMatrices": lambda: lib.netrep_DatasetMatrices(None, _DP, _DP),
        "DatasetIntermediateProperties": lambda: lib.netrep_DatasetIntermediateProperties(
            None, _NAMES, 3, _NAMES, _NAMES, 3, _NAMES, 1, _DP, _IP, _DP, _IP, _DP, _IP),
        "DatasetNetProps": lambda: lib.netrep_DatasetNetProps(None, _NAMES, _NAMES, 3, _NAMES, 1, _DP, _DP, _DP, _DP,
                                                              _DP, _IP),
        "DatasetPermutationProcedure": lambda: lib.netrep_DatasetPermutationProcedure(
            C.byref(dp), None, _NAMES, _NAMES, 3, _NAMES, 1, 0, 1, b"overlap", 0, 0, None, None, _DP),
    }
    assert sorted("netrep_" + k for k in calls) == sorted(set(HANDLE_ENTRIES) - {"netrep_DatasetFromData",
                                                                                 "netrep_DatasetRelease"})
    for name, call in calls.items():
        assert call() == L.NR_ERR_INVALID, name
        assert name in lib.netrep_last_error().decode()


# -- Python signatures --------------------------------------------------------

def _defaults(fn):
    return {k: p.default for k, p in inspect.signature(fn).parameters.items() if p.default is not inspect.Parameter.empty}


def _positional(fn):
    return [k for k, p in inspect.signature(fn).parameters.items() if p.default is inspect.Parameter.empty
            and k != "self"]


def test_python_signatures_and_defaults():
    assert _positional(N.FromDataDataset.__init__) == ["data", "beta"]
    assert _defaults(N.FromDataDataset.__init__) == dict(networkType="unsigned", scaleData=True, tom=False,
                                                         corType="pearson", nCores=0)
    D = N.FromDataDataset
    assert _positional(D.intermediate_properties) == ["tNodeNames", "moduleAssignments", "modules"]
    assert _positional(D.net_props) == ["moduleAssignments", "modules"]
    assert _positional(D.permutation_procedure) == ["discProps", "moduleAssignments", "modules", "nPermutations"]
    assert _defaults(D.permutation_procedure) == dict(nCores=1, nullHypothesis="overlap", verbose=False,
                                                      seed=A.DEFAULT_SEED, pi=None)
    assert _positional(D.matrices) == []
    for name in ("close", "__enter__", "__exit__"):
        assert callable(getattr(D, name))

    assert _positional(N.IntermediatePropertiesFromData) == ["dData", "beta", "tNodeNames", "moduleAssignments",
                                                             "modules"]
    assert _defaults(N.IntermediatePropertiesFromData) == dict(networkType="unsigned", scaleData=False, tom=False,
                                                               corType="pearson")
    assert _positional(N.NetPropsFromData) == ["data", "beta", "moduleAssignments", "modules"]
    assert _defaults(N.NetPropsFromData) == dict(networkType="unsigned", scaleData=True, tom=False,
                                                 corType="pearson")
    assert _positional(N.modulePreservationFromData) == ["datasets", "beta", "moduleAssignments"]
    d = _defaults(N.modulePreservationFromData)
    assert list(d)[:3] == ["modules", "discovery", "test"]
    assert (d["modules"], d["discovery"], d["test"], d["pi"]) == (None, None, None, None)
    assert (d["nullHypothesis"], d["alternative"], d["networkType"], d["scaleData"], d["tom"], d["corType"]) == \
        ("overlap", "greater", "unsigned", True, False, "pearson")
    assert d["seed"] == A.DEFAULT_SEED and d["nPerm"] > 0
    for name in ("FromDataDataset", "IntermediatePropertiesFromData", "NetPropsFromData",
                 "modulePreservationFromData"):
        assert name in N.__all__


def test_colnames_are_required():
    for call in (lambda: N.FromDataDataset(RMatrix(_X), 5.0),
                 lambda: N.IntermediatePropertiesFromData(RMatrix(_X), 5.0, ["a"], {"a": "1"}, ["1"]),
                 lambda: N.NetPropsFromData(RMatrix(_X, None, ["a", "b"]), 5.0, {"a": "1"}, ["1"])):
        with pytest.raises(N.NetRepError) as ei:
            call()
        assert ei.value.code == L.NR_ERR_INVALID and "colname" in str(ei.value)


# -- the driver, on a numpy stand-in ------------------------------------------

class NumpyDataset:
    """FromDataDataset's interface restated with the numpy oracles."""
    built, closed = [], []

    def __init__(self, data, beta, networkType="unsigned", scaleData=True, tom=False, corType="pearson", nCores=0):
        assert not tom and corType == "pearson"
        self.names = [str(n) for n in data.colnames]
        self.xs = R.scale(data.values) if scaleData else np.asarray(data.values, dtype=np.float64)
        self.corr, self.net = R.build(self.xs, beta, networkType, do_scale=False)
        self.beta = beta
        self.open = True
        NumpyDataset.built.append((self.names[0], beta))

    def close(self):
        if self.open:
            NumpyDataset.closed.append(self.names[0])
        self.open = False

    def _index(self, t_names, assignments, modules):
        names, labels = zip(*assignments.items())
        return O.ModuleIndex(names, labels, t_names, modules)

    def intermediate_properties(self, tNodeNames, moduleAssignments, modules):
        assert self.open
        mi = self._index(tNodeNames, moduleAssignments, modules)
        return O.intermediate_properties(self.xs, self.corr, self.net, mi.disc_idx(self.names))

    def permutation_procedure(self, discProps, moduleAssignments, modules, nPermutations, nCores=1,
                              nullHypothesis="overlap", verbose=False, seed=0, pi=None):
        assert self.open
        mi = self._index(self.names, moduleAssignments, modules)
        if pi is None:
            rng = np.random.default_rng(seed % 2**32)
            pi = np.array([rng.permutation(mi.null_idx.size) for _ in range(nPermutations)]).reshape(
                nPermutations, mi.null_idx.size)
        nulls, obs = O.permutation_procedure(discProps, self.xs, self.corr, self.net, mi, pi)
        res = {"observed": obs, "observed_dimnames": (list(modules), O.STATNAMES)}
        if nPermutations > 0:
            res["nulls"] = nulls
        return res


@pytest.fixture
def stand_in(monkeypatch):
    NumpyDataset.built, NumpyDataset.closed = [], []
    monkeypatch.setattr(A, "FromDataDataset", NumpyDataset)
    return NumpyDataset


def _three_datasets():
    """24 nodes in modules "2" (7 nodes), "10" (6) and the background "0";
    dataset B lacks the last three nodes, C has its columns reversed."""
    rng = np.random.default_rng(11)
    names = [f"n{i}" for i in range(24)]
    labels = ["2"] * 7 + ["10"] * 6 + ["0"] * 11
    ma = dict(zip(names, labels))

    def one(cols, seed):
        base = np.random.default_rng(seed).normal(size=(12, 3))
        x = rng.normal(size=(12, len(cols)))
        for j, nm in enumerate(cols):
            lab = ma[nm]
            if lab != "0":
                x[:, j] += 1.5 * base[:, 0 if lab == "2" else 1]
        return RMatrix(x, None, list(cols))
    return {"A": one(names, 1), "B": one(names[:-3], 2), "C": one(names[::-1], 3)}, ma


def test_driver_pair_enumeration(stand_in):
    ds, ma = _three_datasets()
    res = N.modulePreservationFromData(ds, 4.0, {"A": ma}, nPerm=3)
    assert {d: list(v) for d, v in res.items()} == {"A": ["B", "C"]}
    assert sorted(stand_in.built) == [("n0", 4.0), ("n0", 4.0), ("n23", 4.0)]     # one per dataset name
    assert len(stand_in.closed) == 3
    res = N.modulePreservationFromData(ds, 4.0, {"A": ma, "B": ma}, discovery=["A", "B"],
                                       test={"A": "C", "B": ["A", "B"]}, nPerm=2)
    assert {d: list(v) for d, v in res.items()} == {"A": ["C"], "B": ["A"]}      # B within B is skipped
    res = N.modulePreservationFromData(ds, 4.0, {"C": ma}, discovery="C", test="A", nPerm=0)
    r = res["C"]["A"]
    assert "nulls" not in r and "p.values" not in r and r["observed"].shape == (2, 7)


def test_driver_closes_its_datasets_when_it_raises(stand_in):
    ds, ma = _three_datasets()
    bad = dict(ma)
    bad["ghost"] = "2"          # in the test data (as a column name) but not in the discovery data
    ds["B"] = RMatrix(np.random.default_rng(2).normal(size=(12, 4)), None, ["n0", "n1", "n2", "ghost"])
    with pytest.raises(KeyError):
        N.modulePreservationFromData(ds, 4.0, {"A": bad}, test="B", nPerm=2)
    assert len(stand_in.built) == 1 and len(stand_in.closed) == 1
    with pytest.raises(N.NetRepError):
        N.modulePreservationFromData(ds, 4.0, {"A": ma}, test="Z", nPerm=2)
    with pytest.raises(N.NetRepError):
        N.modulePreservationFromData(ds, 4.0, {"B": ma}, discovery="A", nPerm=2)


def test_driver_modules_none_and_beta_dict(stand_in):
    ds, ma = _three_datasets()
    res = N.modulePreservationFromData(ds, {"A": 3.0, "B": 5.0, "C": 6.0}, {"A": ma}, test="B", nPerm=2)
    r = res["A"]["B"]
    assert r["modules"] == ["2", "10"] == order_as_numeric(["10", "2"])       # not "0", numeric order
    assert r["observed"].shape == (2, 7) and r["nulls"].shape == (2, 7, 2)
    assert sorted(stand_in.built) == [("n0", 3.0), ("n0", 5.0)]
    only = N.modulePreservationFromData(ds, 4.0, {"A": ma}, modules=["10"], test="B", nPerm=2)["A"]["B"]
    assert only["modules"] == ["10"] and only["observed"].shape == (1, 7)
    per = N.modulePreservationFromData(ds, 4.0, {"A": ma}, modules={"A": ["10", "2"]}, test="B", nPerm=2)["A"]["B"]
    assert per["modules"] == ["2", "10"]


def test_driver_p_values_are_permutation_test_by_hand(stand_in):
    ds, ma = _three_datasets()
    pi = np.array([np.random.default_rng(s).permutation(21) for s in range(6)], dtype=np.uint32)
    res = N.modulePreservationFromData(ds, 4.0, {"A": ma, "B": {k: v for k, v in ma.items() if k in ds["B"].colnames}},
                                       test="B", nPerm=6, pi=pi, alternative="less")
    r = res["A"]["B"]
    # 21 of A's 24 assigned nodes are in B (the null pool): all 7 of module "2", all 6 of "10"
    assert r["totalSize"] == 21 and dict(r["nVarsPresent"]) == {"2": 7, "10": 6}
    assert dict(r["propVarsPresent"]) == {"2": 1.0, "10": 1.0}
    assert r["alternative"] == "less" and r["contingency"] is not None
    exp = permutationTest(r["nulls"], r["observed"], [7, 6], 21, "less")
    np.testing.assert_array_equal(r["p.values"].view(np.uint64), exp.view(np.uint64))
    assert np.isfinite(r["p.values"]).all() and ((r["p.values"] > 0) & (r["p.values"] <= 1)).all()
    # the result is what combineAnalyses takes
    from netrep_amd.combine import combineAnalyses
    both = combineAnalyses(res, res)
    assert both["A"]["B"]["nulls"].shape == (2, 7, 12)
