"""CPU tests of the correlation types of the from-data path (NR_COR_SPEARMAN,
NR_COR_BICOR): the numpy oracle (tests/cor_ref.py) against hand-worked columns
and a scipy fixture, and the flags through the header, the library's argument
checks and the Python signatures (no GPU needed: the checks run before any
context is opened).

tests/golden/cor_small.npz was written once with scipy 1.15: x, a 9 x 6 matrix
with ties; rankdata = scipy.stats.rankdata(x, axis=0); spearmanr =
scipy.stats.spearmanr(x).statistic. It holds only those three arrays."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import netrep_amd as N
from netrep_amd import _lib as L
from netrep_amd.engine import Engine

import cor_ref as CR
import netbuild_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ranks_by_hand():
    x = np.array([[3.0], [1.0], [3.0], [2.0], [3.0]])
    np.testing.assert_array_equal(CR.ranks(x)[:, 0], [4.0, 1.0, 4.0, 2.0, 4.0])
    # +-Inf are ranked like any value; -0.0 ties with 0.0; a NaN takes the column
    x = np.array([[np.inf, 0.0, 1.0], [-np.inf, -0.0, np.nan], [0.5, 2.0, 3.0]])
    r = CR.ranks(x)
    np.testing.assert_array_equal(r[:, 0], [3.0, 1.0, 2.0])
    np.testing.assert_array_equal(r[:, 1], [1.5, 1.5, 3.0])
    assert np.isnan(r[:, 2]).all()


def test_ranks_are_less_plus_half_of_equal_plus_one():
    x = np.round(np.random.default_rng(3).normal(size=(41, 5)) * 2) / 2
    less = (x[None, :, :] < x[:, None, :]).sum(axis=1)
    equal = (x[None, :, :] == x[:, None, :]).sum(axis=1)
    np.testing.assert_array_equal(CR.ranks(x), less + (equal + 1) / 2.0)


def test_bicor_by_hand():
    col = np.array([1.0, 2.0, 3.0, 4.0, 100.0])
    med, mad, a = CR.bicor_column(col)
    assert med == 3.0 and mad == 1.0
    # u = (x - 3) / 9: the outlier's |u| = 97 / 9 > 1, weight 0
    u = np.array([-2.0, -1.0, 0.0, 1.0]) / 9.0
    np.testing.assert_array_equal(a[4], 0.0)
    np.testing.assert_allclose(a[:4], np.array([-2.0, -1.0, 0.0, 1.0]) * (1 - u * u) ** 2, rtol=4e-16)
    z = CR.bicor_z(col[:, None])[:, 0]
    np.testing.assert_allclose((z * z).sum(), 4.0, rtol=1e-15)
    assert z[4] == 0.0


def test_bicor_even_median():
    col = np.array([4.0, 1.0, 3.0, 2.0, 10.0, 0.0])    # sorted 0 1 2 3 4 10: lo 2, hi 3
    med, mad, _a = CR.bicor_column(col)
    assert med == 2.5
    # d = 1.5 1.5 0.5 0.5 7.5 2.5 -> sorted 0.5 0.5 1.5 1.5 2.5 7.5: lo 1.5, hi 1.5
    assert mad == 1.5
    assert CR.median(np.array([1.0, 2.0])) == 1.5
    assert CR.median(np.array([-0.0, 0.0, 0.0])).tobytes() == np.float64(0.0).tobytes()


def test_bicor_mad_zero_takes_the_pearson_fallback():
    col = np.array([2.0, 2.0, 2.0, 5.0, -1.0])     # med 2, d = 0 0 0 3 3: mad 0
    med, mad, a = CR.bicor_column(col)
    assert med == 2.0 and mad == 0.0
    np.testing.assert_array_equal(a, col - col.mean())
    z = CR.bicor_z(col[:, None])
    np.testing.assert_allclose(z, R.scale(col[:, None]), rtol=4e-16)
    # against a second column: the correlation is Pearson's for this column
    # a constant column: a is all zero, z = 0 / 0
    assert np.isnan(CR.bicor_z(np.full((4, 1), 2.5))).all()
    # any non-finite entry takes the column
    assert np.isnan(CR.bicor_z(np.array([[1.0], [np.inf], [2.0]]))).all()


def test_transforms_are_affine_invariant():
    x = np.random.default_rng(8).standard_t(1.5, size=(31, 4))
    y = 4.0 * x + 8.0                        # exact in binary: no new ties, no rounding of the order
    np.testing.assert_array_equal(CR.ranks(x), CR.ranks(y))
    np.testing.assert_allclose(CR.bicor_z(x), CR.bicor_z(y), rtol=0, atol=1e-13)


def test_scipy_fixture():
    with np.load(os.path.join(ROOT, "tests", "golden", "cor_small.npz")) as f:
        assert sorted(f.files) == ["rankdata", "spearmanr", "x"]
        x, rd, sp = f["x"], f["rankdata"], f["spearmanr"]
    assert x.shape == (9, 6)
    assert any(np.unique(x[:, j]).size < 9 for j in range(6))     # it has ties
    np.testing.assert_array_equal(CR.ranks(x), rd)
    c, _w = CR.build(x, 5.0, "unsigned", "spearman")
    assert np.abs(c - sp).max() <= CR.corr_bar(9, "spearman")


def _header():
    hdr = open(os.path.join(ROOT, "include", "netrep_gpu.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_flags_in_header_and_python():
    for name, value in (("NR_COR_SPEARMAN", 0x100), ("NR_COR_BICOR", 0x200)):
        m = re.search(rf"#define\s+{name}\s+(\S+)", _header())
        assert m and int(m.group(1), 0) == value == getattr(L, name)


def test_net_type_code_all_combinations():
    bases = {"unsigned": 0, "signed": 1, "signed_hybrid": 2}
    cors = {"pearson": 0, "spearman": 0x100, "bicor": 0x200}
    seen = set()
    for nt, b in bases.items():
        for tom in (False, True):
            for ct, c in cors.items():
                code = L.net_type_code(nt, tom, ct)
                assert code == b | (0x10 if tom else 0) | c
                assert code == L.net_type_code(nt, tom=tom, cor_type=ct)
                seen.add(code)
    assert len(seen) == 18
    assert L.net_type_code("signed") == L.net_type_code("signed", False, "pearson") == 1


def test_unknown_cor_type_raises():
    with pytest.raises(N.NetRepError) as ei:
        L.net_type_code("unsigned", False, "kendall")
    assert ei.value.code == L.NR_ERR_INVALID
    for name in ("pearson", "spearman", "bicor"):
        assert name in str(ei.value)
    with pytest.raises(N.NetRepError):      # a correlation type is no network type
        L.net_type_code("bicor")


_X = np.asfortranarray(np.random.default_rng(0).normal(size=(5, 3)))
_XP = _X.ctypes.data_as(L._dp)


def _build_network(net_type):
    lib = L.load()
    out = np.empty((3, 3), order="F")
    rc = lib.netrep_BuildNetwork(_XP, 1, net_type, 5.0, 5, 3, out.ctypes.data_as(L._dp), None)
    return rc, lib.netrep_last_error().decode()


def _permutation_procedure(net_type):
    lib = L.load()
    dp = L.DiscProps()
    names = (C.c_char_p * 3)(b"a", b"b", b"c")
    obs = np.empty((1, 7), order="F")
    rc = lib.netrep_PermutationProcedureFromData(
        C.byref(dp), _XP, 1, net_type, 5.0, 5, 3, names, names, names, 3, names, 1, 0, 1, b"overlap", 0, 0,
        None, None, obs.ctypes.data_as(L._dp))
    return rc, lib.netrep_last_error().decode()


@pytest.mark.parametrize("net_type", [0x100, 0x111, 0x212])
def test_entries_accept_the_flags(net_type):
    """Past the argument check: without a GPU the call fails only when it
    opens a context, with a GPU it succeeds."""
    rc, msg = _build_network(net_type)
    assert rc != L.NR_ERR_INVALID, msg
    if rc != L.NR_OK:
        assert "unknown" not in msg
        # the same failure as the plain type's: the device, not the flag
        assert rc == _build_network(net_type & 0xF)[0]


@pytest.mark.parametrize("net_type,message", [(0x300, "unknown correlation type"), (0x312, "unknown correlation type"),
                                              (0x400, "unknown network type"), (0x103, "unknown network type"),
                                              (0x303, "unknown network type")])
def test_entries_reject_other_values(net_type, message):
    for entry in (_build_network, _permutation_procedure):
        rc, msg = entry(net_type)
        assert rc == L.NR_ERR_INVALID and message in msg, (entry.__name__, rc, msg)


def test_getter_in_header_library_and_signatures():
    assert re.search(r"\bnr_cor_ms\s*\(", _header())
    assert hasattr(L.load(), "nr_cor_ms")
    assert "nr_cor_ms" in L.SIGNATURES
    assert L.load().nr_cor_ms(None, None) == L.NR_ERR_INVALID


def test_lds_row_budget_is_the_kernels():
    src = open(os.path.join(ROOT, "netrep_amd", "csrc", "kernels.h")).read()
    m = re.search(r"constexpr\s+int\s+kCorLdsRows\s*=\s*(\d+)\s*;", src)
    assert m and int(m.group(1)) == Engine.COR_LDS_ROWS
    # the columns-per-workgroup rule: a wave owns a column up to a quarter of it
    assert re.search(r"constexpr\s+int\s+kCorWaveRows\s*=\s*kCorLdsRows\s*/\s*4\s*;", src)
    assert Engine.COR_WAVE_ROWS == Engine.COR_LDS_ROWS // 4


@pytest.mark.parametrize("fn,name", [(N.BuildNetwork, "corType"), (N.PermutationProcedureFromData, "corType"),
                                     (Engine.set_dataset_from_data, "cor_type")])
def test_python_entries_take_the_correlation_type(fn, name):
    p = inspect.signature(fn).parameters
    assert name in p and p[name].default == "pearson"
