"""CPU tests of the from-data path: the numpy restatement (tests/netbuild_ref.py)
pinned to the reference's recorded matrices, and the new entry points' ABI and
argument checks (no GPU needed: the checks run before any context is opened)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from netrep_amd import _lib as L
from netrep_amd.engine import Engine

import netbuild_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ["nr_set_dataset_from_data", "nr_get_dataset_matrices", "nr_netbuild_ms",
               "netrep_PermutationProcedureFromData", "netrep_BuildNetwork"]


@pytest.mark.parametrize("which", ["discovery", "test"])
def test_restatement_matches_reference_fixture(bundled, which):
    """The reference's example data: correlation = cor(data), network =
    abs(correlation)^5 (R/example-data.R:111-116). Bars from the dot product's
    length, S = 30: corr 4 S 2^-53 = 1.3e-14, net beta times that = 6.7e-14
    (measured 6.7e-16 and 3.3e-15)."""
    data = bundled[f"{which}_data"]
    s, beta = data.shape[0], 5.0
    assert s == 30
    c, w = R.build(data, beta, "unsigned")
    ce = np.abs(c - bundled[f"{which}_correlation"]).max()
    we = np.abs(w - bundled[f"{which}_network"]).max()
    print(f"{which}: corr error {ce:.3e}, net error {we:.3e}")
    assert ce <= 4 * s * 2.0 ** -53
    assert we <= beta * 4 * s * 2.0 ** -53


def test_restatement_transforms_and_nan():
    c = np.array([-1.0, -0.5, 0.0, 0.25, 1.0, np.nan])
    np.testing.assert_array_equal(R.network(c, 2.0, "unsigned")[:5], [1.0, 0.25, 0.0, 0.0625, 1.0])
    np.testing.assert_array_equal(R.network(c, 2.0, "signed")[:5], [0.0, 0.0625, 0.25, 0.390625, 1.0])
    np.testing.assert_array_equal(R.network(c, 2.0, "signed_hybrid")[:5], [0.0, 0.0, 0.0, 0.0625, 1.0])
    for t in R.NET_TYPES:
        assert np.isnan(R.network(c, 2.0, t)[5])
    x = np.random.default_rng(3).normal(size=(9, 4))
    x[:, 2] = 1.5                                    # constant column: NaN row and column
    cc, ww = R.build(x, 3.0)
    bad = np.zeros((4, 4), bool)
    bad[2, :] = bad[:, 2] = True
    np.testing.assert_array_equal(np.isnan(cc), bad)
    np.testing.assert_array_equal(np.isnan(ww), bad)


def test_header_and_library_have_the_new_entries():
    hdr = open(os.path.join(ROOT, "include", "netrep_gpu.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = L.load()
    for name in NEW_ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert hasattr(lib, name), name
        assert name in L.SIGNATURES
    for macro, val in (("NR_NET_UNSIGNED", 0), ("NR_NET_SIGNED", 1), ("NR_NET_SIGNED_HYBRID", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, val), hdr)
        assert getattr(L, macro) == val


def test_python_tile_constant_matches_the_kernel():
    src = open(os.path.join(ROOT, "netrep_amd", "csrc", "kernels.h")).read()
    assert int(re.search(r"kNetbuildTile\s*=\s*(\d+)", src).group(1)) == Engine.NETBUILD_TILE >= 64


_X = np.asfortranarray(np.random.default_rng(0).normal(size=(5, 3)))
_XP = _X.ctypes.data_as(L._dp)
# (data, net_type, beta, n_samples, n_nodes), one invalid argument each
INVALID = {
    "data NULL": (None, 0, 5.0, 5, 3),
    "n_samples 1": (_XP, 0, 5.0, 1, 3),
    "n_nodes 0": (_XP, 0, 5.0, 5, 0),
    "net_type 3": (_XP, 3, 5.0, 5, 3),
    "net_type -1": (_XP, -1, 5.0, 5, 3),
    "beta 0": (_XP, 0, 0.0, 5, 3),
    "beta negative": (_XP, 0, -2.0, 5, 3),
    "beta nan": (_XP, 0, math.nan, 5, 3),
    "beta inf": (_XP, 0, math.inf, 5, 3),
}
# what the entry's own check says (not a context or device failure)
MESSAGE = {"data": "data missing", "n_": "n_samples >= 2 and n_nodes >= 1", "net": "unknown network type",
           "beta": "beta must be finite"}


def _expected_message(case):
    return next(v for k, v in MESSAGE.items() if case.startswith(k))


@pytest.mark.parametrize("case", sorted(INVALID))
def test_build_network_rejects_invalid_arguments(case):
    data, net_type, beta, s, n = INVALID[case]
    lib = L.load()
    out = np.empty((3, 3), order="F")
    rc = lib.netrep_BuildNetwork(data, 1, net_type, beta, s, n, out.ctypes.data_as(L._dp), None)
    assert rc == L.NR_ERR_INVALID
    assert _expected_message(case) in lib.netrep_last_error().decode()


@pytest.mark.parametrize("case", sorted(INVALID))
def test_permutation_from_data_rejects_invalid_arguments(case):
    data, net_type, beta, s, n = INVALID[case]
    lib = L.load()
    dp = L.DiscProps()
    names = (C.c_char_p * 3)(b"a", b"b", b"c")
    obs = np.empty((1, 7), order="F")
    rc = lib.netrep_PermutationProcedureFromData(
        C.byref(dp), data, 1, net_type, beta, s, n, names, names, names, 3, names, 1, 0, 1, b"overlap", 0, 0,
        None, None, obs.ctypes.data_as(L._dp))
    assert rc == L.NR_ERR_INVALID
    assert _expected_message(case) in lib.netrep_last_error().decode()


def test_engine_entries_reject_a_null_context():
    lib = L.load()
    assert lib.nr_set_dataset_from_data(None, _XP, 3, 5, L.NR_HOST, 0, 0, 5.0) == L.NR_ERR_INVALID
    assert lib.nr_get_dataset_matrices(None, None, None) == L.NR_ERR_INVALID
    assert lib.nr_netbuild_ms(None, None) == L.NR_ERR_INVALID


def test_python_rejects_unknown_network_type():
    with pytest.raises(L.NetRepError) as ei:
        L.net_type_code("bicor")
    assert ei.value.code == L.NR_ERR_INVALID
    assert L.net_type_code("signed hybrid") == L.NR_NET_SIGNED_HYBRID
