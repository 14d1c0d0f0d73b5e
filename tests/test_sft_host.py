"""CPU tests of the soft-threshold pick (no GPU needed): the numpy oracles
(tests/sft_ref.py) against the definitions written out as loops, the
library's pure host functions (netrep_ScaleFreeFit, netrep_ScaleFreeBins,
netrep_SftPowerEstimate) against the oracles, and the new entries through the
header, the library's argument checks -- which run before any context is
opened -- and the Python signatures."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest

import netrep_amd as N
from netrep_amd import _lib as L
from netrep_amd.engine import Engine

import netbuild_ref as R
import sft_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["nr_soft_connectivity", "nr_sft_ms", "nr_sft_finite", "nr_set_sft_row_groups", "netrep_ScaleFreeFit",
               "netrep_ScaleFreeBins", "netrep_SftPowerEstimate", "netrep_PickSoftThreshold"]


# ---- the oracle against the definition as loops ------------------------------

def _connectivity_loops(c, powers, net_type):
    n = c.shape[0]
    out = np.zeros((n, len(powers)))
    for m, p in enumerate(powers):
        for i in range(n):
            t = 0.0
            for u in range(n):
                if u == i:
                    continue
                cc = c[i, u]
                b = abs(cc) if net_type == "unsigned" else ((1.0 + cc) / 2.0 if net_type == "signed"
                                                            else (cc if cc > 0.0 else 0.0))
                t += b ** p
            out[i, m] = t
    return out


@pytest.mark.parametrize("net_type", SR.NET_TYPES)
def test_connectivity_oracle_matches_the_loops(net_type):
    c = R.correlation(R.scale(np.random.default_rng(3).normal(size=(9, 6))))
    powers = [1, 2, 6, 0.5, 2]
    SR.assert_connectivity_close(SR.connectivity(c, powers, net_type), _connectivity_loops(c, powers, net_type), 6,
                                 powers, net_type)


def test_connectivity_oracle_edge_cases():
    np.testing.assert_array_equal(SR.connectivity(np.array([[1.0]]), [1, 2]), [[0.0, 0.0]])   # n = 1: k = 0
    c = R.correlation(R.scale(np.random.default_rng(4).normal(size=(7, 5))))
    c[2, :] = c[:, 2] = np.nan                                                                # a NaN column
    for net_type in SR.NET_TYPES:
        assert np.isnan(SR.connectivity(c, [1, 3], net_type)).all()
    assert (SR.base(np.array([-0.5, 0.0, 0.25]), "signed_hybrid") == [0.0, 0.0, 0.25]).all()


# ---- the fit ------------------------------------------------------------------

def _heavy(n=500, seed=1):
    return np.random.default_rng(seed).pareto(1.5, n) * 3.0 + 0.5


def _empty_bin():
    """B = 10 over [0, 10]: nothing in (4, 5], bin 5."""
    v = np.random.default_rng(2).uniform(0.0, 10.0, 400)
    v = v[(v <= 4.0) | (v > 5.0)]
    return np.concatenate([[0.0, 10.0], v])


def _zero_mean_bin():
    """A hybrid network's k: isolated nodes with k = 0 fill bin 1 alone."""
    return np.concatenate([np.zeros(30), np.random.default_rng(5).uniform(2.0, 10.0, 100), [10.0]])


# name -> (k, n_breaks, remove_first); tools and docs quote the bar measured over these
FIT_CASES = {
    "heavy": (_heavy(), 10, False),
    "heavy_remove_first": (_heavy(), 10, True),
    "heavy_20": (_heavy(), 20, False),
    "empty_bin": (_empty_bin(), 10, False),
    "zero_mean_bin": (_zero_mean_bin(), 10, False),
    "zero_mean_bin_remove_first": (_zero_mean_bin(), 10, True),
    "three_bins": (_heavy(60, 7), 3, False),
    "three_bins_remove_first": (_heavy(60, 7), 3, True),
    "five_bins": (_heavy(200, 8), 5, False),
}


def _lib_fit(k, n_breaks, remove_first):
    k = np.ascontiguousarray(k, dtype=np.float64)
    out = np.empty(3)
    rc = L.load().netrep_ScaleFreeFit(k.ctypes.data_as(L._dp), k.size, n_breaks, int(remove_first),
                                      out.ctypes.data_as(L._dp))
    assert rc == L.NR_OK, L.load().netrep_last_error().decode()
    bins = np.empty(k.size, dtype=np.int32)
    assert L.load().netrep_ScaleFreeBins(k.ctypes.data_as(L._dp), k.size, n_breaks,
                                         bins.ctypes.data_as(L._i32p)) == L.NR_OK
    return out, bins


def _bins_loops(k, n_breaks):
    mn, dx = min(k), max(k) - min(k)
    return [1 + sum(1 for m in range(1, n_breaks) if ki > mn + m * (dx / n_breaks)) for ki in k]


@pytest.mark.parametrize("case", sorted(FIT_CASES))
def test_fit_matches_the_oracle(case):
    k, n_breaks, remove_first = FIT_CASES[case]
    exp = SR.scale_free_fit(k, n_breaks, remove_first)
    got, bins = _lib_fit(k, n_breaks, remove_first)
    np.testing.assert_array_equal(bins, exp["bins"])                       # every node's bin, exactly
    np.testing.assert_array_equal(bins, _bins_loops(k.tolist(), n_breaks))
    np.testing.assert_array_equal(np.bincount(bins, minlength=n_breaks + 1)[1:], exp["counts"])
    n_used = n_breaks - int(remove_first)
    for name, g, e in zip(("rsq", "slope", "trunc"), got, (exp["rsq"], exp["slope"], exp["trunc"])):
        print(f"{case} {name}: library {g!r} oracle {e!r}")
        if name == "trunc" and n_used <= 3:
            assert math.isnan(g) and math.isnan(e)
        else:
            assert math.isfinite(e) and abs(g - e) <= SR.FIT_BAR, (case, name, g, e)
    assert N.ScaleFreeFit(k, n_breaks, remove_first) == {
        "Rsquared.SFT": got[0], "slope.SFT": got[1], "truncatedExponentialAdjRsquared": pytest.approx(got[2], nan_ok=True)}


def test_cases_are_what_they_say():
    assert 0 in SR.scale_free_fit(*FIT_CASES["empty_bin"])["counts"][1:-1]
    f = SR.scale_free_fit(*FIT_CASES["zero_mean_bin"])
    k = FIT_CASES["zero_mean_bin"][0]
    assert f["counts"][0] == 30 and (k[f["bins"] == 1] == 0.0).all()
    # a heavy tail: fewer nodes at higher k
    assert SR.scale_free_fit(*FIT_CASES["heavy"])["slope"] < 0


def test_the_extremes_land_in_the_end_bins():
    for k, n_breaks, _rf in FIT_CASES.values():
        _out, bins = _lib_fit(k, n_breaks, False)
        assert (bins[k == k.max()] == n_breaks).all() and (bins[k == k.min()] == 1).all()
        assert bins.min() >= 1 and bins.max() <= n_breaks
    # values exactly on an inner edge belong to the bin below (right-closed)
    k = np.array([0.0, 2.0, 4.0, 6.0, 8.0, 6.5])
    _out, bins = _lib_fit(k, 4, False)
    np.testing.assert_array_equal(bins, [1, 1, 2, 3, 4, 4])


@pytest.mark.parametrize("k", [np.full(20, 3.5), np.array([1.0, 2.0, np.nan, 4.0]), np.array([1.0, np.inf, 3.0]),
                               np.array([2.0])])
def test_constant_or_non_finite_k_gives_nans(k):
    got, bins = _lib_fit(k, 10, False)
    assert np.isnan(got).all() and (bins == 0).all()
    exp = SR.scale_free_fit(k, 10, False)
    assert math.isnan(exp["rsq"]) and math.isnan(exp["slope"]) and math.isnan(exp["trunc"])


def test_fit_rejects_bad_arguments():
    lib = L.load()
    k = np.arange(5.0)
    out = np.empty(3)
    kp, op = k.ctypes.data_as(L._dp), out.ctypes.data_as(L._dp)
    for args in ((None, 5, 10, 0, op), (kp, 5, 10, 0, None), (kp, 0, 10, 0, op), (kp, 5, 2, 0, op)):
        assert lib.netrep_ScaleFreeFit(*args) == L.NR_ERR_INVALID
        assert lib.netrep_last_error().decode()
    assert lib.netrep_ScaleFreeBins(kp, 5, 2, np.empty(5, np.int32).ctypes.data_as(L._i32p)) == L.NR_ERR_INVALID


# ---- powerEstimate -------------------------------------------------------------

def _estimate(powers, rsq, slope, cut=0.85):
    table = np.zeros((len(powers), 7), order="F")
    table[:, 0], table[:, 1], table[:, 2] = powers, rsq, slope
    est = C.c_double()
    assert L.load().netrep_SftPowerEstimate(table.ctypes.data_as(L._dp), len(powers), cut,
                                            C.cast(C.byref(est), L._dp)) == L.NR_OK
    got = None if math.isnan(est.value) else est.value
    assert got == SR.power_estimate(powers, rsq, slope, cut)
    return got


def test_power_estimate_on_hand_made_tables():
    powers = [1, 2, 3, 4, 6]
    # the first power that passes, in the given order (4 would pass too)
    assert _estimate(powers, [0.2, 0.7, 0.9, 0.95, 0.99], [-0.5, -1.0, -1.5, -1.7, -2.0]) == 3.0
    assert _estimate([6, 4, 3], [0.99, 0.95, 0.9], [-2.0, -1.7, -1.5]) == 6.0
    # none passes
    assert _estimate(powers, [0.2, 0.7, 0.8, 0.84, 0.85], [-1.0] * 5) is None
    # a positive slope does not pass, however good the line
    assert _estimate(powers, [0.99, 0.99, 0.99, 0.99, 0.9], [2.0, 1.0, 0.5, 0.0, -1.0]) == 6.0
    assert _estimate([1, 2], [0.99, 0.99], [1.0, 1.0]) is None
    # NaN rows do not pass; another cut
    assert _estimate([1, 2], [np.nan, 0.9], [np.nan, -1.0]) == 2.0
    assert _estimate(powers, [0.2, 0.7, 0.9, 0.95, 0.99], [-1.0] * 5, cut=0.6) == 2.0


# ---- header, bindings, argument checks -----------------------------------------

def _header():
    hdr = open(os.path.join(ROOT, "include", "netrep_gpu.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_new_entries_in_header_library_and_signatures():
    hdr, lib = _header(), L.load()
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES, name
    src = open(os.path.join(ROOT, "netrep_amd", "csrc", "kernels.h")).read()
    m = re.search(r"constexpr\s+int\s+kSftMaxPowers\s*=\s*(\d+)\s*;", src)
    assert m and int(m.group(1)) == Engine.SFT_MAX_POWERS == 32


def test_context_entries_reject_null():
    lib = L.load()
    assert lib.nr_sft_ms(None, None) == L.NR_ERR_INVALID
    assert lib.nr_sft_finite(None, None) == L.NR_ERR_INVALID
    assert lib.nr_set_sft_row_groups(None, 1) == L.NR_ERR_INVALID
    assert lib.nr_soft_connectivity(None, None, 1, 2, 1, 0, None, 1, None) == L.NR_ERR_INVALID


_X = np.asfortranarray(np.random.default_rng(0).normal(size=(5, 3)))
_XP = _X.ctypes.data_as(L._dp)


def _pick(powers, net_type=0, data=_XP, table=True, est=True, n_powers=None, n_breaks=10, s=5, n=3):
    lib = L.load()
    p = None if powers is None else np.ascontiguousarray(powers, dtype=np.float64)
    n_p = (0 if p is None else p.size) if n_powers is None else n_powers
    tab = np.empty((max(n_p, 1), 7), order="F")
    e = C.c_double()
    rc = lib.netrep_PickSoftThreshold(data, 1, net_type, s, n, None if p is None else p.ctypes.data_as(L._dp), n_p,
                                      0.85, n_breaks, 0, tab.ctypes.data_as(L._dp) if table else None,
                                      C.cast(C.byref(e), L._dp) if est else None, None)
    return rc, lib.netrep_last_error().decode()


@pytest.mark.parametrize("kwargs,message", [
    (dict(powers=[1, 2], data=None), "missing"),
    (dict(powers=None, n_powers=2), "missing"),
    (dict(powers=[1, 2], table=False), "missing"),
    (dict(powers=[1, 2], est=False), "missing"),
    (dict(powers=[], n_powers=0), "n_powers"),
    (dict(powers=list(range(1, 34))), "n_powers"),
    (dict(powers=[1, 0]), "powers must be finite and > 0"),
    (dict(powers=[1, -2.5]), "powers must be finite and > 0"),
    (dict(powers=[1, np.nan]), "powers must be finite and > 0"),
    (dict(powers=[np.inf]), "powers must be finite and > 0"),
    (dict(powers=[1, 2], net_type=L.NR_NET_TOM), "NR_NET_TOM"),
    (dict(powers=[1, 2], net_type=L.NR_NET_TOM | L.NR_NET_SIGNED), "NR_NET_TOM"),
    (dict(powers=[1, 2], net_type=3), "unknown network type"),
    (dict(powers=[1, 2], net_type=0x300), "unknown correlation type"),
    (dict(powers=[1, 2], n_breaks=2), "n_breaks"),
    (dict(powers=[1, 2], s=1), "n_samples"),
])
def test_pick_rejects_before_a_context_is_opened(kwargs, message):
    rc, msg = _pick(**kwargs)
    assert rc == L.NR_ERR_INVALID and message in msg, (rc, msg)


def test_valid_pick_fails_only_where_build_network_does():
    """Past the argument checks: without a GPU both fail when they open a
    context, with the same code; with one, both succeed."""
    lib = L.load()
    out = np.empty((3, 3), order="F")
    rc_build = lib.netrep_BuildNetwork(_XP, 1, 0, 5.0, 5, 3, out.ctypes.data_as(L._dp), None)
    msg_build = lib.netrep_last_error().decode()
    for powers, net_type in (([1, 2, 6], 0), (list(range(1, 33)), L.NR_NET_SIGNED | L.NR_COR_SPEARMAN),
                             ([0.5], L.NR_NET_SIGNED_HYBRID | L.NR_COR_BICOR)):
        rc, msg = _pick(powers, net_type)
        assert rc == rc_build, (rc, msg)
        if rc != L.NR_OK:
            assert msg == msg_build


def test_python_signatures_and_defaults():
    p = inspect.signature(N.PickSoftThreshold).parameters
    assert list(p) == ["data", "powerVector", "networkType", "corType", "scaleData", "RsquaredCut", "nBreaks",
                       "removeFirst", "returnConnectivity"]
    assert tuple(p["powerVector"].default) == tuple(range(1, 11)) + (12, 14, 16, 18, 20) == SR.DEFAULT_POWERS
    assert (p["networkType"].default, p["corType"].default) == ("unsigned", "pearson")
    assert p["scaleData"].default is True and p["RsquaredCut"].default == 0.85 and p["nBreaks"].default == 10
    assert p["removeFirst"].default is False and p["returnConnectivity"].default is False
    p = inspect.signature(N.ScaleFreeFit).parameters
    assert list(p) == ["k", "nBreaks", "removeFirst"] and p["nBreaks"].default == 10 and p["removeFirst"].default is False
    p = inspect.signature(Engine.soft_connectivity).parameters
    assert list(p) == ["self", "data", "powers", "net_type", "scale", "cor_type"]
    assert (p["net_type"].default, p["scale"].default, p["cor_type"].default) == ("unsigned", True, "pearson")
    assert callable(Engine.sft_ms) and Engine.SFT_MAX_POWERS == 32
    from netrep_amd.api import SFT_COLUMNS
    assert SFT_COLUMNS == SR.COLUMNS


def test_python_rejects_tom_and_unknown_names():
    x = np.random.default_rng(0).normal(size=(5, 3))
    with pytest.raises(N.NetRepError) as ei:
        N.PickSoftThreshold(x, networkType="tom")
    assert ei.value.code == L.NR_ERR_INVALID
    with pytest.raises(N.NetRepError) as ei:
        N.PickSoftThreshold(x, corType="kendall")
    assert ei.value.code == L.NR_ERR_INVALID
