"""The soft-threshold pick on the GPU (nr_soft_connectivity: netbuild.hip's
soft_connectivity_kernel and its reduction; netrep_PickSoftThreshold): the
connectivities of every candidate power from the data matrix alone, against
the numpy oracle (tests/sft_ref.py) started from the engine's own correlation
bits -- the corr that set_dataset_from_data exports for the same data, type
and cor_type.

Bar (sft_ref): (n + 2 p_max + 16) 2^-52 relative per entry, exact where the
expected value is 0; the fit columns at sft_ref.FIT_BAR."""
import ctypes as C

import numpy as np
import pytest

import netrep_amd as N
from netrep_amd import _lib as L

import netbuild_ref as R
import sft_ref as SR
from test_gpu_dual import _case
from test_gpu_netbuild import _bits, _set_modules

pytestmark = pytest.mark.gpu

T = N.Engine.NETBUILD_TILE   # the kernel's tile (it runs the from-data kernel's main loop)
DEFAULT = list(SR.DEFAULT_POWERS)


def _corr(eng, x, net_type="unsigned", scale=True, cor_type="pearson"):
    """The engine's own correlation bits for this data (beta does not enter corr)."""
    eng.set_dataset_from_data(x, 2.0, net_type, scale=scale, cor_type=cor_type)
    return eng.matrices()[0]


def _check(x, powers, net_type, what, scale=True, cor_type="pearson"):
    n = x.shape[1]
    with N.Engine(0) as eng:
        c = _corr(eng, x, net_type, scale, cor_type)
        k = eng.soft_connectivity(x, powers, net_type, scale=scale, cor_type=cor_type)
        assert eng.sft_ms() > 0.0
    assert k.shape == (n, len(powers)) and k.flags.f_contiguous
    SR.assert_connectivity_close(k, SR.connectivity(c, powers, net_type), n, powers, what)
    return c, k


# n carries the tile edges (below one MFMA tile, just past one, around the
# 64-column workgroup tile, three tile rows with a ragged edge, four tile rows
# and columns: interior tiles on both sides of the diagonal); S the chunk
# edges (a partial chunk only, exactly one whole chunk, whole + partial).
EDGE_CASES = [
    (1, 5, "unsigned"), (2, 5, "signed"), (15, 3, "signed_hybrid"), (17, 5, "unsigned"), (63, 17, "signed"),
    (64, 32, "signed_hybrid"), (65, 61, "unsigned"), (129, 33, "signed"), (3 * T + 1, 61, "unsigned"),
    (3 * T + 1, 8, "signed_hybrid"),
]


@pytest.mark.parametrize("n,s,net_type", EDGE_CASES)
def test_tile_and_chunk_edges(n, s, net_type):
    x = np.random.default_rng(1000 * n + s).normal(size=(s, n))
    c, k = _check(x, DEFAULT, net_type, f"n={n} S={s} {net_type}")
    if n == 1:
        np.testing.assert_array_equal(k, np.zeros((1, len(DEFAULT))))
    if (n, s) == (3 * T + 1, 8):
        assert (SR.base(c, net_type) == 0.0).mean() > 0.25   # the case is what it says


POWER_SETS = {
    "chain_default": DEFAULT,
    "chain_64": [64],
    "pow": [0.5, 2.5, 6.0],
    "mixed_order_duplicates": [6, 1, 6],
    "one_power": [3],
    "pow_one_power": [1.5],
    "thirty_two": list(range(1, 33)),
    "pow_thirty_two": [0.25 * m for m in range(1, 33)],
}


@pytest.mark.parametrize("n,s", [(65, 61), (3 * T + 1, 61)])
@pytest.mark.parametrize("name", sorted(POWER_SETS))
def test_both_arithmetic_paths(name, n, s):
    powers = POWER_SETS[name]
    x = np.random.default_rng(31 * n + s).normal(size=(s, n))
    net_type = SR.NET_TYPES[(len(name) + n) % 3]
    _c, k = _check(x, powers, net_type, f"{name} n={n} {net_type}")
    if name == "mixed_order_duplicates":
        np.testing.assert_array_equal(_bits(k[:, 0]), _bits(k[:, 2]))
        assert not np.array_equal(k[:, 0], k[:, 1])


def test_row_groups():
    """The test override regroups the partial sums: every R within the bar;
    the same R twice, and the default twice, bitwise equal. 7 is more than
    the four row tiles: three groups are empty."""
    n, s = 3 * T + 1, 61
    x = np.random.default_rng(77).normal(size=(s, n))
    with N.Engine(0) as eng:
        exp = SR.connectivity(_corr(eng, x), DEFAULT, "unsigned")
        d0 = eng.soft_connectivity(x, DEFAULT)
        np.testing.assert_array_equal(_bits(d0), _bits(eng.soft_connectivity(x, DEFAULT)))
        for r in (1, 2, 3, 4, 7):
            eng.set_sft_row_groups(r)
            k = eng.soft_connectivity(x, DEFAULT)
            SR.assert_connectivity_close(k, exp, n, DEFAULT, f"R={r}")
            np.testing.assert_array_equal(_bits(k), _bits(eng.soft_connectivity(x, DEFAULT)))
        eng.set_sft_row_groups(0)
        np.testing.assert_array_equal(_bits(d0), _bits(eng.soft_connectivity(x, DEFAULT)))
        with pytest.raises(N.NetRepError) as ei:
            eng.set_sft_row_groups(-1)
        assert ei.value.code == L.NR_ERR_INVALID


@pytest.mark.parametrize("cor_type,net_type", [("spearman", "signed"), ("bicor", "unsigned")])
def test_cor_types(cor_type, net_type):
    x = np.random.default_rng(13).normal(size=(61, 65))
    _check(x, DEFAULT, net_type, f"{cor_type} {net_type}", cor_type=cor_type)


def test_prescaled_data():
    x = np.random.default_rng(21).normal(size=(61, 65))
    with N.Engine(0) as eng:
        xs = eng.scale(x)
        a = eng.soft_connectivity(x, DEFAULT, "signed", scale=True)
        b = eng.soft_connectivity(xs, DEFAULT, "signed", scale=False)
    np.testing.assert_array_equal(_bits(a), _bits(b))
    _check(R.scale(x), [2, 7], "signed_hybrid", "pre-scaled", scale=False)


def _scratch_bytes(eng):
    b = C.c_int64()
    assert L.load().nr_scratch_bytes(eng._h, C.byref(b)) == L.NR_OK
    return b.value


def test_resident_state_untouched():
    _lay, mi, disc, txs, _tc, _tn = _case([40, 20, 7], 30, 31, n_nodes=150)
    other = np.random.default_rng(3).normal(size=(19, 3 * T + 1))
    with N.Engine(0) as eng:
        assert eng.sft_ms() == 0.0
        eng.set_dataset_from_data(txs, 5.0, "unsigned", scale=False)
        _set_modules(eng, mi, disc)
        obs, nulls = eng.observed(), eng.run(0, 8, 77)
        held, shape = _scratch_bytes(eng), eng.shape()
        k = eng.soft_connectivity(other, DEFAULT, "signed")
        assert np.isfinite(k).all() and eng.sft_ms() > 0.0
        assert _scratch_bytes(eng) == held and eng.shape() == shape
        np.testing.assert_array_equal(_bits(eng.observed()), _bits(obs))
        np.testing.assert_array_equal(_bits(eng.run(0, 8, 77)), _bits(nulls))


def test_constant_column(bundled):
    x = bundled["test_data"].copy()
    x[:, 37] = 2.5
    with N.Engine(0) as eng:
        k = eng.soft_connectivity(x, DEFAULT)
    assert np.isnan(k).all()
    with pytest.raises(N.NetRepError) as ei:
        N.PickSoftThreshold(x)
    assert ei.value.code == L.NR_ERR_NONFINITE


def test_engine_rejects_invalid_arguments():
    x = np.random.default_rng(2).normal(size=(6, 4))
    with N.Engine(0) as eng:
        for powers in ([], list(range(1, 34)), [1, 0], [np.nan], [np.inf]):
            with pytest.raises(N.NetRepError) as ei:
                eng.soft_connectivity(x, powers)
            assert ei.value.code == L.NR_ERR_INVALID
        assert eng.sft_ms() == 0.0


@pytest.mark.parametrize("net_type", SR.NET_TYPES)
def test_end_to_end_on_bundled_data(bundled, net_type):
    x = bundled["test_data"]
    n = x.shape[1]
    assert n == 150
    got = N.PickSoftThreshold(x, networkType=net_type, returnConnectivity=True)
    with N.Engine(0) as eng:
        c = _corr(eng, x, net_type)
        np.testing.assert_array_equal(_bits(got["connectivity"]), _bits(eng.soft_connectivity(x, DEFAULT, net_type)))
    exp = SR.pick(c, DEFAULT, net_type)
    SR.assert_connectivity_close(got["connectivity"], exp["connectivity"], n, DEFAULT, f"bundled {net_type}")
    g, e = got["fitIndices"], exp["fitIndices"]
    assert list(g) == SR.COLUMNS
    np.testing.assert_array_equal(g["Power"], e["Power"])
    for col in ("SFT.R.sq", "slope", "truncated.R.sq"):
        err = np.abs(g[col] - e[col]).max()
        print(f"bundled {net_type} {col}: max error {err:.3e} (bar {SR.FIT_BAR:.1e})")
        assert np.isfinite(e[col]).all() and err <= SR.FIT_BAR, (col, g[col], e[col])
    for col in ("mean.k.", "median.k.", "max.k."):
        # the oracle's own k differs from the engine's at the connectivity bar
        bar = SR.connectivity_bar(n, DEFAULT) + (n + 16) * 2.0 ** -52
        assert (np.abs(g[col] - e[col]) <= bar * np.abs(e[col])).all(), col
    # and on the engine's own connectivities: exact order statistics, the mean at its bar
    k = got["connectivity"]
    np.testing.assert_array_equal(g["max.k."], k.max(axis=0))
    np.testing.assert_array_equal(g["median.k."], np.median(k, axis=0))
    assert (np.abs(g["mean.k."] - k.mean(axis=0)) <= (n + 16) * 2.0 ** -52 * k.mean(axis=0)).all()
    for m in range(len(DEFAULT)):
        f = SR.scale_free_fit(k[:, m])
        assert abs(g["SFT.R.sq"][m] - f["rsq"]) <= SR.FIT_BAR and abs(g["slope"][m] - f["slope"]) <= SR.FIT_BAR
        assert abs(g["truncated.R.sq"][m] - f["trunc"]) <= SR.FIT_BAR
    assert got["powerEstimate"] == exp["powerEstimate"]
    assert got["powerEstimate"] == SR.power_estimate(DEFAULT, g["SFT.R.sq"], g["slope"])
    print(f"bundled {net_type}: powerEstimate {got['powerEstimate']}")
