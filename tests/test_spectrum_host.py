"""CPU: certifies the case table of the designed-spectrum GPU tests
(tests/spectrum_ref.py CASES, run by tests/test_gpu_spectra.py). Every block
is the one the GPU test runs (one fixed seed per case).

Columns: the block is scaled data. Spectrum: its top gap and rank are the
designed ones. Reference conditioning: the oracle's statistics of the block
with LAPACK's two SVD drivers agree within a tenth of the parity bar -- a
condition on the inputs, not a measurement: a block that breaks it leaves the
table (spectrum_ref.REDRAW), it never gets a wider bar. Emulated steps: a numpy
restatement of the kernels' stop rule keeps the slow cases 20 steps under the
step cap, and the cap case half a cap beyond it. Planner: every case reaches
the class and kernel it is meant for (host code, no GPU)."""
import numpy as np
import pytest

from oracle import netrep_oracle as O

import spectrum_ref as R
from conftest import FLOOR

CASES = R.all_cases()
CAP = [(cls, i) for cls in R.CAP_CASES for i in range(R.CAP_REPLICAS)]


def check_columns(x):
    assert np.abs(x.mean(axis=0)).max() <= 1e-14
    assert np.abs(x.std(axis=0, ddof=1) - 1.0).max() <= 1e-13


def check_spectrum(x, spec):
    s, k = x.shape
    ev = np.linalg.eigvalsh(x.T @ x)[::-1]
    target = R.top_gap(spec, k, s)
    gap = (ev[0] - ev[1]) / ev[0]
    assert abs(gap - target) <= 0.01 * target, (gap, target)
    assert int((ev > 1e-12 * ev[0]).sum()) == int(np.count_nonzero(R.spectrum(spec, k, s)))


def driver_disagreement(x):
    """The oracle's data statistics of the block (coherence; cor.contrib and
    avg.contrib against a fixed discovery vector) with dgesvd and with dgesdd:
    their largest difference under conftest's scaling, and the largest
    absolute difference of the per-node vectors (contributions, summary
    profile)."""
    idx = np.arange(x.shape[1])
    d_nc = np.random.default_rng(0).uniform(-1.0, 1.0, x.shape[1])
    stats, vecs = [], []
    keep = O.SVD_DRIVER
    try:
        for drv in ("gesvd", "gesdd"):
            O.SVD_DRIVER = drv
            sp = O.summary_profile(x, idx)
            nc = O.node_contribution(x, idx, sp)
            stats.append(np.array([O.module_coherence(nc), O.correlation(d_nc, nc), O.sign_aware_mean(d_nc, nc)]))
            vecs.append(np.concatenate([nc, sp]))
    finally:
        O.SVD_DRIVER = keep
    a, b = stats
    return float((np.abs(a - b) / np.maximum(np.abs(a), FLOOR)).max()), float(np.abs(vecs[0] - vecs[1]).max())


def check_conditioning(x):
    stat, vec = driver_disagreement(x)
    print(f"LAPACK drivers apart: statistics {stat:.2e} (scaled), per-node vectors {vec:.2e} (absolute)")
    assert stat <= 1e-11      # a tenth of the parity bar (conftest.RTOL)
    assert vec <= 1e-11       # a tenth of the per-node bar of test_gpu_spectra.VEC_FLOOR


def lanczos_gram(x):
    s, k = x.shape
    return x.T @ x if k <= s else x @ x.T     # the kernels' Lanczos dimension is min(k, S)


@pytest.mark.parametrize("case", CASES, ids=R.case_id)
def test_columns_and_spectrum(case):
    cls, s, k, spec = case
    x = R.case_block(cls, s, k, spec)
    assert x.shape == (s, k)
    check_columns(x)
    check_spectrum(x, spec)


@pytest.mark.parametrize("case", CASES, ids=R.case_id)
def test_reference_conditioning(case):
    cls, s, k, spec = case
    check_conditioning(R.case_block(cls, s, k, spec))


@pytest.mark.parametrize("case", [c for c in CASES if min(c[1], c[2]) > 160], ids=R.case_id)
def test_emulated_steps_stay_under_the_cap(case):
    """Where the step cap is below the Lanczos dimension (min(k, S) > 160),
    the emulated run converges at least 20 steps under it: the kernels stop
    at a check only, checks come at most 8 steps apart, and the emulator's
    full reorthogonalisation is the best case of the kernels' partial one."""
    cls, s, k, spec = case
    g = lanczos_gram(R.case_block(cls, s, k, spec))
    cap = R.step_cap(g.shape[0])
    steps, capped = R.lanczos_steps(g, cap, start="constant" if cls == "full_gram" else "column")
    print(f"{R.case_id(case)}: {steps} emulated steps, cap {cap}")
    assert not capped and steps <= cap - 20
    if spec in R.SLOW:
        assert steps > 4 * R.FIRST_CHECK   # slow indeed: far beyond the first check


def test_slow_cases_are_in_the_table():
    slow = [c for c in CASES if c[3] in R.SLOW and min(c[1], c[2]) > 160]
    assert {c[0] for c in slow} == {"table", "packed_runtime"} and len(slow) == 6


@pytest.mark.parametrize("cls,replica", CAP)
def test_cap_case(cls, replica):
    """The cap spectrum: scaled data of the designed spectrum, a
    well-conditioned reference, and an emulated run that is cut at the cap
    and would need at least 1.5 times the cap without one."""
    x = R.cap_block(cls, replica)
    check_columns(x)
    check_spectrum(x, R.CAP_SPECTRUM)
    check_conditioning(x)
    g = lanczos_gram(x)
    cap = R.step_cap(g.shape[0])
    assert cap == 160
    assert R.lanczos_steps(g, cap) == (cap, True)
    steps, _ = R.lanczos_steps(g, None)
    print(f"cap case {cls}/{replica}: {steps} emulated steps without a cap")
    assert steps >= 1.5 * cap


@pytest.mark.parametrize("cls", list(R.CASES))
def test_cases_reach_their_class(cls):
    s, sizes, p_cls, p_kernel, table = R.CASES[cls]
    n_nodes = sum(k * len(specs) for k, specs in sizes.items()) + 64
    R.assert_planned(list(sizes), s, n_nodes, p_cls, p_kernel, table, n_perm=4)
    for k in sizes:   # primal designed blocks need k <= S - 1
        assert k <= s - 1 or k > s


@pytest.mark.parametrize("cls", list(R.CAP_CASES))
def test_cap_cases_reach_their_class(cls):
    s, k, p_kernel, table = R.CAP_CASES[cls]
    R.assert_planned([k], s, k * R.CAP_REPLICAS + 64, "packed", p_kernel, table)
    (plan,) = R.launch_plans([k], s, k * R.CAP_REPLICAS + 64)
    assert int(plan["m"]) == 160 == R.step_cap(min(k, s))


def test_step_cap_is_the_planner_s():
    for k, s in ((96, 320), (161, 320), (300, 150), (320, 400), (520, 400), (350, 400), (905, 600), (1744, 1800)):
        (plan,) = R.launch_plans([k], s, 4000)
        if plan["class"] in ("packed", "full_partials_in_scratch"):
            assert int(plan["m"]) == R.step_cap(min(k, s)), (k, s)


def test_rotation_tables_send_null_items_onto_the_replicas():
    names = [f"G{i}" for i in range(40)]
    labels = ["0"] * 40
    for i in range(5):
        labels[i] = "1"
    for i in range(15, 18):
        labels[i] = "2"
    mi = O.ModuleIndex(names, labels, names, ["1", "2"])
    reps = {"1": [np.arange(0, 5), np.arange(5, 10), np.arange(10, 15)], "2": [np.arange(15, 18), np.arange(18, 21)]}
    pis = R.rotation_tables(mi, reps, 6, np.random.default_rng(3))
    orders = set()
    for p in range(6):
        assert np.array_equal(np.sort(pis[p]), np.arange(40))
        ridx = mi.random_idx(pis[p].astype(np.int64))
        for m in ("1", "2"):
            want = reps[m][p % len(reps[m])]
            assert np.array_equal(np.sort(ridx[m]), want)
        orders.add(tuple(ridx["1"]))
    assert len(orders) == 6     # shuffled within the block: each visit in another node order


def test_block_dataset_layout():
    rng = np.random.default_rng(5)
    blocks = [R.case_block("wave", 104, 33, ("rank3",)), R.case_block("wave", 104, 96, ("pair", 1e-2))]
    x, corr, net, pos = R.block_dataset(blocks, 104, 7, rng)
    assert x.shape == (104, 33 + 96 + 7) and [p.tolist() for p in pos] == [list(range(33)), list(range(33, 129))]
    assert np.array_equal(corr, corr.T) and (np.diag(corr) == 1.0).all()
    assert np.array_equal(net, np.abs(corr) ** 5)
    np.testing.assert_allclose(corr, np.corrcoef(x, rowvar=False), atol=1e-13)
    np.testing.assert_allclose(x[:, 129:], O.scale(x[:, 129:]), atol=1e-13)
