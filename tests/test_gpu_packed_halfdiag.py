"""The Gram-table kernel's packed Gram stores its diagonal halved (kernels.hip
packed_gram_doubles), so that the packed matvec's lower and mirrored parts
both run over every stored element and the diagonal term is the sum of their
two halves. The table fill halves the diagonal at the store; whoever needs
G_cc doubles what it reads (the Lanczos start column, the node contributions,
the squared pass's column norms). The kernels that take their Gram from the
matrix cores keep the plain diagonal.

Module sizes sit where a diagonal block meets the layout's edges: a 16-column
group edge (15, 16, 17, 47, 48, 63..65, 79..81, 112, 127, 128), a 64-row chunk
edge (63, 64, 65, 127, 128), the ones column in a group of its own (16, 48, 64,
80, 112, 128) and items with fewer matvec units than waves (1, 2, 15). S = 128
puts the launch above the wave class (Lanczos dimension 111), on the packed
kernels. Null "overlap" (ModuleIndex's default), against the C++ LAPACK
restatement on identical shuffles at conftest's bar.

The two-node module's cor.degree, cor.contrib and avg.contrib are rounding
noise in the reference itself (tests/test_gpu_edge.py) and are masked as
there."""
import numpy as np
import pytest

import netrep_amd as N
from oracle import netrep_oracle as O

from conftest import assert_stats_close
from test_gpu_dual import _case, _cpp
from test_gpu_edge import _mask_two_node_noise
from test_gpu_parity import _engine_from

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 15, 16, 17, 47, 48, 63, 64, 65, 79, 80, 81, 112, 127, 128]
N_PERM = 32
SEED = 19


@pytest.fixture(scope="module")
def table_case():
    """The table-path dataset with its oracle cube, computed once."""
    lay, mi, disc, txs, tc, tn = _case(SIZES, 128, 51, n_nodes=1500)
    pis = N.prp_table(SEED, 0, N_PERM, mi.null_idx.size)
    exp, obs = _cpp(mi, disc, txs, tc, tn, pis)
    for a in (exp, obs, txs, tc, tn):
        a.setflags(write=False)
    return mi, disc, txs, tc, tn, exp, obs


def _engine_subset(mi, disc, txs, tc, tn, mods):
    eng = N.Engine(0)
    eng.set_dataset(tc, tn, txs)
    node_off = np.concatenate([[0], np.cumsum([mi.test_idx[m].size for m in mods])])
    eng.set_modules(len(mi.modules), [mi.modules.index(m) for m in mods], node_off,
                    np.concatenate([mi.test_idx[m] for m in mods]),
                    np.concatenate([mi.null_pos[m] for m in mods]),
                    np.concatenate([disc["corr"][m] for m in mods]),
                    np.concatenate([disc["degree"][m] for m in mods]),
                    np.concatenate([disc["contribution"][m] for m in mods]))
    eng.set_null_pool(mi.null_idx)
    return eng


def test_table_fill_halved_diagonal_vs_cpp_oracle(table_case):
    """Every module on the Gram-table path: the table fill stores G_cc / 2."""
    mi, disc, txs, tc, tn, exp, obs = table_case
    eng = _engine_from(mi, disc, txs, tc, tn)
    nulls = eng.run(0, N_PERM, SEED)
    assert eng.gram_table()
    e_obs = assert_stats_close(_mask_two_node_noise(eng.observed(), mi), _mask_two_node_noise(obs, mi),
                               what="observed (table, halved diagonal)")
    e_null = assert_stats_close(_mask_two_node_noise(nulls, mi), _mask_two_node_noise(exp, mi),
                                what="nulls (table, halved diagonal)")
    print(f"table path: max scaled error observed {e_obs:.3e}, nulls {e_null:.3e}")


def test_table_larger_modules_run_both_precisions(table_case):
    """The larger modules' items take more than 16 Lanczos steps on average, so
    the fp64 passes and the relaxed fp32 passes over the halved diagonal both
    ran. (The engine's diagnostics count steps over a whole run, so the
    assertion is on the mean over these six modules' items, not per module.
    What no end-to-end test here can see is the squared pass's correction for
    the halved diagonal: it only decides which column starts the Lanczos run,
    and any start column converges to the same pair.)"""
    mi, disc, txs, tc, tn, exp, obs = table_case
    big = [m for m in mi.mods_present if mi.test_idx[m].size >= 79]
    assert len(big) == 6
    eng = _engine_subset(mi, disc, txs, tc, tn, big)
    nulls = eng.run(0, N_PERM, SEED)
    assert eng.gram_table()
    d = eng.diagnostics()
    print(f"larger modules: {d}")
    assert d["eig_items"] >= len(big) * N_PERM
    assert d["eig_steps"] > 16 * d["eig_items"]
    assert d["eig_cap_hits"] == 0
    rows = [mi.modules.index(m) for m in big]
    assert_stats_close(nulls[rows], exp[rows], what="nulls (larger modules alone)")


@pytest.mark.parametrize("n_samples", [128, 64])
def test_matrix_core_producers_vs_cpp_oracle(n_samples):
    """No Gram table, so the packed Grams come from the matrix-core epilogues,
    which keep the plain diagonal, and the matvec keeps its test for it (the
    same packed_matvec with the halved diagonal compiled out): the two forms
    must not mix. The engine builds no table when the packed class (modules of up to 320
    nodes) holds a dual item (k > S): the 300-node module is one at either S.
    A 400-node module alone does not do it -- it runs in the large-module
    launch (dual there: the 64 x 64 super-tile epilogue) and leaves the packed
    class on the table. At S = 64 every module above 64 nodes goes dual."""
    lay, mi, disc, txs, tc, tn = _case(SIZES + [300, 400], n_samples, 53, n_nodes=2200)
    eng = _engine_from(mi, disc, txs, tc, tn)
    nulls = eng.run(0, 8, SEED)
    assert not eng.gram_table()
    pis = N.prp_table(SEED, 0, 8, mi.null_idx.size)
    exp, obs = _cpp(mi, disc, txs, tc, tn, pis)
    e_obs = assert_stats_close(_mask_two_node_noise(eng.observed(), mi), _mask_two_node_noise(obs, mi),
                               what=f"observed (matrix cores, S={n_samples})")
    e_null = assert_stats_close(_mask_two_node_noise(nulls, mi), _mask_two_node_noise(exp, mi),
                                what=f"nulls (matrix cores, S={n_samples})")
    print(f"matrix-core producers S={n_samples}: max scaled error observed {e_obs:.3e}, nulls {e_null:.3e}")


def test_table_nonfinite_column_gives_na(table_case):
    """A NaN data column in one member node of the 80-node module: that
    module's summary-profile statistics are NA (src/netStats.cpp:229-235), the
    other modules' observed statistics still match the oracle (the Python
    restatement, which carries the reference's NA rules, as the other
    non-finite tests use). Observed items only: null items with a non-finite
    member take the same fill and the same flag, and are not run here."""
    mi, disc, txs, tc, tn, _, _ = table_case
    txs = txs.copy()
    m0 = next(m for m in mi.mods_present if mi.test_idx[m].size == 80)
    txs[:, mi.test_idx[m0][5]] = np.nan
    eng = _engine_from(mi, disc, txs, tc, tn)
    obs = eng.observed()
    assert eng.gram_table()
    _, exp = O.permutation_procedure(disc, txs, tc, tn, mi, np.zeros((0, mi.null_idx.size), int))
    assert_stats_close(_mask_two_node_noise(obs, mi), _mask_two_node_noise(exp, mi),
                       what="observed with NaN column (table, halved diagonal)")
    row = mi.modules.index(m0)
    assert not np.isfinite(obs[row, [1, 4, 6]]).any()
    assert np.isfinite(obs[row, [0, 2, 3, 5]]).all()
