"""CPU tests of the topological-overlap option of the from-data path
(NR_NET_TOM): the numpy oracle (tests/tom_ref.py) against the definition
written out as loops, and the flag through the header, the library's argument
checks and the Python signatures (no GPU needed: the checks run before any
context is opened)."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import netrep_amd as N
from netrep_amd import _lib as L
from netrep_amd.engine import Engine

import netbuild_ref as R
import tom_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _adjacency(n, net_type, beta, seed):
    x = np.random.default_rng(seed).normal(size=(max(n, 4) + 3, n))
    return R.build(x, beta, net_type)[1]


def _tom_loops(a):
    n = a.shape[0]
    a = a.copy()
    for i in range(n):
        a[i, i] = 0.0
    t = np.empty((n, n))
    for i in range(n):
        for j in range(n):
            if i == j:
                t[i, j] = 1.0
                continue
            ki = sum(a[u, i] for u in range(n))
            kj = sum(a[u, j] for u in range(n))
            lij = sum(a[i, u] * a[u, j] for u in range(n))
            t[i, j] = (lij + a[i, j]) / (min(ki, kj) + 1.0 - a[i, j])
    return t


@pytest.mark.parametrize("net_type", R.NET_TYPES)
def test_oracle_matches_the_triple_loop(net_type):
    a = _adjacency(6, net_type, 2.0, 11)
    got, exp = TR.tom(a), _tom_loops(a)
    assert np.abs(got - exp).max() <= TR.tom_bar(6) * np.abs(exp).max()
    TR.assert_tom_close(got, exp, 6, net_type)


def test_oracle_smallest_cases():
    np.testing.assert_array_equal(TR.tom(np.array([[0.7]])), [[1.0]])
    # n = 2: L_01 = 0 and k_0 = k_1 = a_01, so t_01 = a_01 / (a_01 + 1 - a_01)
    a = np.array([[1.0, 0.375], [0.375, 1.0]])
    np.testing.assert_array_equal(TR.tom(a), [[1.0, 0.375], [0.375, 1.0]])


@pytest.mark.parametrize("net_type", R.NET_TYPES)
def test_oracle_symmetric_unit_diagonal_in_unit_interval(net_type):
    a = _adjacency(41, net_type, 3.0, 5)
    assert a.min() >= 0.0 and a.max() <= 1.0
    t = TR.tom(a)
    np.testing.assert_array_equal(np.diag(t), np.ones(41))
    assert np.abs(t - t.T).max() <= TR.tom_bar(41)
    assert t.min() >= 0.0 and t.max() <= 1.0


def test_oracle_propagates_nan_and_keeps_the_diagonal():
    a = _adjacency(7, "unsigned", 2.0, 3)
    a[2, :] = a[:, 2] = np.nan
    t = TR.tom(a)
    np.testing.assert_array_equal(np.isnan(t), ~np.eye(7, dtype=bool))
    np.testing.assert_array_equal(np.diag(t), np.ones(7))
    # one NaN degree alone is kept by the minimum
    with pytest.raises(AssertionError):
        TR.assert_tom_close(np.ones((7, 7)), t, 7)


def _header():
    hdr = open(os.path.join(ROOT, "include", "netrep_gpu.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_flag_in_header_and_python():
    m = re.search(r"#define\s+NR_NET_TOM\s+(\S+)", _header())
    assert m and int(m.group(1), 0) == 0x10 == L.NR_NET_TOM


def test_getter_in_header_library_and_signatures():
    assert re.search(r"\bnr_tom_ms\s*\(", _header())
    assert hasattr(L.load(), "nr_tom_ms")
    assert "nr_tom_ms" in L.SIGNATURES


def test_getter_rejects_null():
    assert L.load().nr_tom_ms(None, None) == L.NR_ERR_INVALID


def test_tom_tile_is_the_netbuild_tile():
    """The TOM kernel runs the from-data kernel's main loop on its tile: the
    GPU cases sized by Engine.NETBUILD_TILE reach its tile edges too."""
    src = open(os.path.join(ROOT, "netrep_amd", "csrc", "netbuild.hip")).read()
    assert re.search(r"kNbTile\s*=\s*kNetbuildTile\b", src)
    body = src[src.index("tom_kernel("):]
    assert "nb_syrk_tile(A, n, n," in body[:body.index("deinterleave_kernel")]


_X = np.asfortranarray(np.random.default_rng(0).normal(size=(5, 3)))
_XP = _X.ctypes.data_as(L._dp)


def _build_network(net_type):
    lib = L.load()
    out = np.empty((3, 3), order="F")
    rc = lib.netrep_BuildNetwork(_XP, 1, net_type, 5.0, 5, 3, out.ctypes.data_as(L._dp), None)
    return rc, lib.netrep_last_error().decode()


@pytest.mark.parametrize("net_type", [0x10, 0x11, 0x12])
def test_build_network_accepts_the_flag(net_type):
    """Past the argument check: without a GPU the call fails only when it
    opens a context, with a GPU it succeeds."""
    rc, msg = _build_network(net_type)
    assert rc != L.NR_ERR_INVALID, msg
    if rc != L.NR_OK:
        assert "unknown network type" not in msg
        # the same failure as the plain type's: the device, not the flag
        assert rc == _build_network(net_type & 0xF)[0]


@pytest.mark.parametrize("net_type", [0x13, 0x20, 0x10 | 8])
def test_entries_reject_other_values(net_type):
    rc, msg = _build_network(net_type)
    assert rc == L.NR_ERR_INVALID and "unknown network type" in msg
    lib = L.load()
    dp = L.DiscProps()
    names = (C.c_char_p * 3)(b"a", b"b", b"c")
    obs = np.empty((1, 7), order="F")
    rc = lib.netrep_PermutationProcedureFromData(
        C.byref(dp), _XP, 1, net_type, 5.0, 5, 3, names, names, names, 3, names, 1, 0, 1, b"overlap", 0, 0,
        None, None, obs.ctypes.data_as(L._dp))
    assert rc == L.NR_ERR_INVALID and "unknown network type" in lib.netrep_last_error().decode()


def test_net_type_code_takes_tom():
    assert L.net_type_code("signed", tom=True) == 0x11
    assert L.net_type_code("unsigned", tom=True) == 0x10
    assert L.net_type_code("signed hybrid", tom=True) == 0x12
    assert L.net_type_code("signed", tom=False) == L.net_type_code("signed") == 1


@pytest.mark.parametrize("fn", [N.BuildNetwork, N.PermutationProcedureFromData, Engine.set_dataset_from_data])
def test_python_entries_take_tom(fn):
    p = inspect.signature(fn).parameters
    assert "tom" in p and p["tom"].default is False
