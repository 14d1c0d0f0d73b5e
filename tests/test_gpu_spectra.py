"""The summary-profile kernels on designed spectra and on uncentred data.

Designed spectra (tests/spectrum_ref.py; tests/test_spectrum_host.py certifies
every block on the CPU): each class of the launch planner gets modules whose
observed AND null items are scaled blocks with a prescribed correlation
spectrum -- top gaps from 1e-1 down to 3e-4, forty eigenvalues within 5% of the
top, a flat top, half rank (duplicated probes), rank 3 (an early Lanczos
breakdown). For each module size there is one replica of the module per
spectrum; explicit permutation tables send the module's null items onto the
replicas (spectrum_ref.rotation_tables), every replica at least twice, in two
node orders. Against the C++ LAPACK restatement on the same tables at
conftest's bar; the per-node vectors of every block (module_vectors) against
the oracle too. Every case first asks the planner for the class and kernel it
is meant to reach. One spectrum reaches the step cap: its error is recorded,
not held to a bar.

Uncentred data: the kernels' data statistics carry mean terms (cov = (Gv)_j /
sigma - S m_j u_bar, var_x = G_jj - S m_j^2, var_u = 1 - S u_bar^2) that scaled
columns multiply by zero, and every class's Gram has a ones row of its own
producer behind them. y_j = a_j x_j + b_j of the scaled synthetic data keeps
corr and net as they are and makes all of them count; the oracle runs on the
same y. The offsets stay small enough that no statistic loses digits to
cancellation (asserted from the oracle's side), so the bar stays conftest's."""
import functools
import zlib

import numpy as np
import pytest

import netrep_amd as N
from netrep_amd import synthetic as SYN
from oracle import netrep_oracle as O

import spectrum_ref as R
from conftest import assert_stats_close, record
from test_gpu_dual import _case, _cpp
from test_gpu_parity import _engine_from

pytestmark = pytest.mark.gpu

N_BACKGROUND = 64

# Bar of the per-node vectors (contributions, summary profile) of the designed
# blocks: |gpu - oracle| <= 1e-10 absolute (floor 1). They are first order in
# the top eigenvector's rotation towards the second one, which any backward
# stable solver leaves at eps / gap: LAPACK's own two SVD drivers differ per
# node by up to 4.6e-12 absolute on these blocks, which is up to 2.8e-10 under
# the statistics' floor of 1e-2 (measured on the CPU; the host test holds the
# absolute figure to 1e-11, a tenth of this bar). The statistics average over
# the nodes and keep conftest's bar.
VEC_FLOOR = 1.0


def _rng(*key):
    return np.random.default_rng(zlib.crc32("/".join(str(k) for k in key).encode()))


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


class Designed:
    """One dataset of designed blocks: per module size one replica per block,
    module labels on the first replica, the rest and the background "0"."""

    def __init__(self, key, n_samples, blocks_of_size, n_perm):
        self.n_samples = n_samples
        blocks, owner = [], []
        for i, (k, bl) in enumerate(blocks_of_size.items()):
            assert all(b.shape == (n_samples, k) for b in bl)
            blocks += bl
            owner += [str(i + 1)] * len(bl)
        rng = _rng(key, "dataset")
        self.x, self.corr, self.net, self.pos = R.block_dataset(blocks, n_samples, N_BACKGROUND, rng)
        n = self.x.shape[1]
        self.sizes = list(blocks_of_size)
        modules = [str(i + 1) for i in range(len(self.sizes))]
        self.replicas = {m: [p for p, o in zip(self.pos, owner) if o == m] for m in modules}
        names = [f"G{i + 1}" for i in range(n)]
        labels = ["0"] * n
        members = {}
        for m in modules:
            members[m] = self.replicas[m][0]
            for c in members[m]:
                labels[c] = m
        self.mi = O.ModuleIndex(names, labels, names, modules)
        # discovery properties from an independent synthetic dataset of the same layout
        lay = SYN.Layout(n, np.array(self.sizes), names, labels, modules, members)
        dx, dc, dn = SYN.numpy_dataset(lay, n_samples, zlib.crc32(key.encode()) & 0xFFFF)
        self.disc = O.intermediate_properties(O.scale(dx), dc, dn, self.mi.disc_idx(names))
        self.pis = R.rotation_tables(self.mi, self.replicas, n_perm, rng)
        self.exp, self.obs = _cpp(self.mi, self.disc, self.x, self.corr, self.net, self.pis)
        _freeze(self.x, self.corr, self.net, self.pis, self.exp, self.obs)

    def engine(self):
        return _engine_from(self.mi, self.disc, self.x, self.corr, self.net)


def _vectors_vs_oracle(eng, x, index_sets, floor, what):
    """module_vectors on explicit index sets against the oracle: the summary
    profile (the sp_out path, with its orientation sign), the node
    contributions and the coherence. Returns the worst scaled error."""
    node_off = np.concatenate([[0], np.cumsum([i.size for i in index_sets])])
    got = eng.module_vectors(node_off, np.concatenate(index_sets), True)
    worst = 0.0
    for b, idx in enumerate(index_sets):
        srt, rank = O.sort_nodes(idx)
        sp = O.summary_profile(x, srt)
        nc = O.node_contribution(x, srt, sp)[rank]
        lo, hi = int(node_off[b]), int(node_off[b + 1])
        worst = max(worst,
                    assert_stats_close(got["summary"][b], sp, floor=floor, what=f"{what}: summary profile {b}"),
                    assert_stats_close(got["contribution"][lo:hi], nc, floor=floor, what=f"{what}: contributions {b}"),
                    assert_stats_close([got["coherence"][b]], [O.module_coherence(nc)], what=f"{what}: coherence {b}"))
    return worst


# ----------------------------------------------------------------------------
# designed spectra, class by class
# ----------------------------------------------------------------------------

def _scaled_error(got, exp, floor=1e-2):
    """The figure assert_stats_close asserts on, without the assertion (so a
    record can be made before a failure)."""
    got, exp = np.asarray(got, np.float64), np.asarray(exp, np.float64)
    fin = np.isfinite(got) & np.isfinite(exp)
    return float((np.abs(got[fin] - exp[fin]) / np.maximum(np.abs(exp[fin]), floor)).max()) if fin.any() else 0.0


WORST = {}


def _record_worst(name, err, **extra):
    """One parity_maxerr.json entry per class: the worst figure of its spectra so far."""
    w = WORST.setdefault(name, {"err": 0.0, "by_spectrum": {}})
    w["err"] = max(w["err"], err)
    w["by_spectrum"].update(extra.pop("by_spectrum", {}))
    record(name, w["err"], by_spectrum=dict(w["by_spectrum"]), **extra)


@functools.lru_cache(maxsize=None)
def designed(cls):
    """The class's dataset and oracle cube and one pass of the engine over
    it, made once per class and shared by the tests below (which compare
    spectrum by spectrum and leave it unchanged). The planned class and kernel
    are asserted before anything runs."""
    s, sizes, p_cls, p_kernel, table = R.CASES[cls]
    blocks = {k: [R.case_block(cls, s, k, spec) for spec in specs] for k, specs in sizes.items()}
    n_rep = max(len(b) for b in blocks.values())
    # every replica twice; the full Gram's single block: one permutation
    d = Designed(cls, s, blocks, 2 * n_rep if n_rep > 1 else 1)
    n_perm = d.pis.shape[0]
    R.assert_planned(d.sizes, s, d.x.shape[1], p_cls, p_kernel, table, n_perm)
    eng = d.engine()
    obs = eng.observed()
    nulls = eng.run(0, n_perm, 1, pi=d.pis)
    on_table = eng.gram_table()
    node_off = np.concatenate([[0], np.cumsum([p.size for p in d.pos])])
    vec = eng.module_vectors(node_off, np.concatenate(d.pos), True)
    eng.close()
    d.corr = d.net = None   # (the N x N matrices are not needed any more)
    return cls, d, obs, nulls, on_table, node_off, vec


def _specs_of(cls):
    out = []
    for specs in R.CASES[cls][1].values():
        out += [sp for sp in specs if sp not in out]
    return out


CLASS_SPECTRA = [(cls, spec) for cls in R.CASES for spec in _specs_of(cls)]
_ids = [f"{cls}-{R.spec_name(spec)}" for cls, spec in CLASS_SPECTRA]


@pytest.mark.parametrize("cls", list(R.CASES))
def test_designed_spectra_reach_their_kernel(cls):
    cls, d, obs, nulls, on_table, node_off, vec = designed(cls)
    assert on_table == R.CASES[cls][4]
    assert np.isfinite(obs).all() and np.isfinite(nulls).all()


@pytest.mark.parametrize("cls,spec", CLASS_SPECTRA, ids=_ids)
def test_designed_spectrum_vs_cpp_oracle(cls, spec):
    """The statistics of every item that carries this spectrum -- the null
    items the permutation tables send onto its replicas, and the observed row
    where it is the first replica -- at conftest's bar.

    Measured on the MI355X (worst scaled error per family over all classes):
    pair 1e-1 .. 3e-4, cluster(40, 0.05), half_rank: <= 3.3e-11; rank3:
    <= 3.1e-14 since the breakdown rule (up to 2.2 before it); flat(0.3):
    <= 1.1e-11 since long runs are run again with the tight reorthogonalisation
    bound (before: 3.0e-09 on the wave class, 8.3e-09 on the small class,
    2.3e-09 on the table at 200 nodes and 2.2 at 300 nodes, a wrong vector
    with no cap hit). DESIGN.md section 8 has both findings."""
    cls, d, obs, nulls, on_table, node_off, vec = designed(cls)
    sizes = R.CASES[cls][1]
    n_perm = nulls.shape[2]
    worst = 0.0
    checks = []
    for row, (k, specs) in enumerate(sizes.items()):
        if spec not in specs:
            continue
        i = specs.index(spec)
        perms = [p for p in range(n_perm) if p % len(specs) == i]
        assert len(perms) >= (2 if len(specs) > 1 else 1)
        checks.append((nulls[row][:, perms], d.exp[row][:, perms], f"nulls ({cls}, {k} nodes, {R.spec_name(spec)})"))
        if i == 0:
            checks.append((obs[row], d.obs[row], f"observed ({cls}, {k} nodes, {R.spec_name(spec)})"))
    assert checks
    for got, exp, what in checks:
        e = _scaled_error(got, exp)
        print(f"{what}: max scaled error {e:.3e}")
        worst = max(worst, e)
    _record_worst(f"designed spectra: {cls}", worst, by_spectrum={R.spec_name(spec): worst}, n_samples=R.CASES[cls][0],
                  sizes=list(sizes))
    for got, exp, what in checks:
        assert_stats_close(got, exp, what=what)


@pytest.mark.parametrize("cls,spec", CLASS_SPECTRA, ids=_ids)
def test_designed_spectrum_module_vectors(cls, spec):
    """module_vectors on every block of this spectrum: the summary profile
    (the sp_out path and its orientation sign) and the node contributions at
    VEC_FLOOR, the coherence at conftest's bar. Measured: <= 2.6e-12 for every
    spectrum (flat(0.3) before the tight bound on long runs: 6.7e-10 on the
    wave class, 9.0e-10 on the small class, 0.31 on the table)."""
    cls, d, obs, nulls, on_table, node_off, vec = designed(cls)
    sizes = R.CASES[cls][1]
    blocks = [(k, sp) for k, specs in sizes.items() for sp in specs]
    checks = []
    for b, (k, sp) in enumerate(blocks):
        if sp != spec:
            continue
        idx = d.pos[b]
        u = O.summary_profile(d.x, idx)
        nc = O.node_contribution(d.x, idx, u)
        lo, hi = int(node_off[b]), int(node_off[b + 1])
        what = f"{cls}, {k} nodes, {R.spec_name(spec)}"
        checks += [(vec["summary"][b], u, VEC_FLOOR, f"summary profile ({what})"),
                   (vec["contribution"][lo:hi], nc, VEC_FLOOR, f"contributions ({what})"),
                   ([vec["coherence"][b]], [O.module_coherence(nc)], 1e-2, f"coherence ({what})")]
    assert checks
    worst = 0.0
    for got, exp, floor, what in checks:
        e = _scaled_error(got, exp, floor)
        print(f"{what}: max scaled error {e:.3e} (floor {floor:g})")
        worst = max(worst, e)
    _record_worst(f"designed spectra, per-node vectors: {cls}", worst, by_spectrum={R.spec_name(spec): worst})
    for got, exp, floor, what in checks:
        assert_stats_close(got, exp, floor=floor, what=what)


SLOW_CASES = [("table", R.CLUSTER40), ("table", R.FLAT), ("packed_runtime", R.CLUSTER40)]


@pytest.mark.parametrize("cls,spec", SLOW_CASES, ids=[f"{c}-{R.spec_name(sp)}" for c, sp in SLOW_CASES])
def test_slow_spectra_stay_under_the_step_cap(cls, spec):
    """A spectrum that crowds the top (forty eigenvalues within 5%; a flat
    top), alone in a run: many steps, none at the cap. Measured mean steps
    per item (of the final run: a run of more than 64 steps is run again with
    the tight bound): cluster 133.5 (table) and 136.5
    (runtime layout), errors 3.1e-12 and 1.2e-11; flat 118.5, error 7.9e-12
    (the emulator: 131 - 136 and 106 - 131 steps)."""
    s, sizes, p_cls, p_kernel, table = R.CASES[cls]
    blocks = {k: [R.case_block(cls, s, k, spec)] for k, specs in sizes.items() if spec in specs and min(k, s) > 160}
    assert len(blocks) == 2
    d = Designed(f"{cls}/slow/{R.spec_name(spec)}", s, blocks, 2)
    n_perm = d.pis.shape[0]
    R.assert_planned(d.sizes, s, d.x.shape[1], p_cls, p_kernel, table, n_perm)
    eng = d.engine()
    eng.reset_timing()
    nulls = eng.run(0, n_perm, 1, pi=d.pis)
    assert eng.gram_table() == table
    g = eng.diagnostics()
    eng.close()
    err = _scaled_error(nulls, d.exp)
    print(f"slow spectrum {R.spec_name(spec)}, {cls}: {g}, mean steps {g['eig_steps'] / max(g['eig_items'], 1):.1f}, "
          f"max scaled error {err:.3e}")
    record(f"designed spectra, slow case alone: {cls}, {R.spec_name(spec)}", err,
           mean_steps=g["eig_steps"] / max(g["eig_items"], 1), eig_reorths=g["eig_reorths"], eig_cap_hits=g["eig_cap_hits"])
    assert g["eig_items"] >= n_perm * len(d.sizes)
    assert g["eig_cap_hits"] == 0
    assert g["eig_steps"] > 16 * g["eig_items"]
    assert_stats_close(nulls, d.exp, what=f"nulls (slow spectrum {R.spec_name(spec)}, {cls})")


@pytest.mark.parametrize("cls", list(R.CAP_CASES))
def test_step_cap_is_reported(cls):
    """The cap, recorded and not repaired: one 320-node module whose replicas
    all carry the cap spectrum (140 eigenvalues within 5% of the top; the
    emulated run needs some 250 steps, the basis holds 160). Every item reports
    the cap through diagnostics()["eig_cap_hits"] -- the only trace the engine
    leaves -- and every statistic is finite. The error against the oracle is
    printed and recorded; it has no bar. Measured: 6.0e-5
    (table) and 3.7e-4 (matrix-core Gram), every item at the cap."""
    s, k, p_kernel, table = R.CAP_CASES[cls]
    d = Designed(cls + "/cap", s, {k: [R.cap_block(cls, i) for i in range(R.CAP_REPLICAS)]}, 2 * R.CAP_REPLICAS)
    n_perm = d.pis.shape[0]
    R.assert_planned([k], s, d.x.shape[1], "packed", p_kernel, table, n_perm)
    eng = d.engine()
    eng.reset_timing()
    nulls = eng.run(0, n_perm, 1, pi=d.pis)
    assert eng.gram_table() == table
    g = eng.diagnostics()
    print(f"cap case, {cls}: {g}")
    assert g["eig_cap_hits"] >= g["eig_items"] >= n_perm   # every item reports the cap
    obs = eng.observed()
    assert np.isfinite(nulls).all() and np.isfinite(obs).all()
    fin = np.abs(np.concatenate([(nulls - d.exp).ravel(), (obs - d.obs).ravel()]))
    ref = np.maximum(np.abs(np.concatenate([d.exp.ravel(), d.obs.ravel()])), 1e-2)
    err = float((fin / ref).max())
    record(f"step cap reached (no bar): {cls}", err, n_samples=s, size=k, spectrum=R.spec_name(R.CAP_SPECTRUM),
           eig_cap_hits=g["eig_cap_hits"], eig_items=g["eig_items"])
    eng.close()


# ----------------------------------------------------------------------------
# uncentred data on every class
# ----------------------------------------------------------------------------

# class -> (module sizes, S, seed of test_gpu_*'s case of that shape, nodes, planned class, kernel, Gram table)
UNCENTRED = {
    "wave": ([200, 113, 112, 61, 60, 59, 7], 60, 33, 3000, "wave", "wave", False),
    "small": ([112, 96, 64, 33, 16], 300, 35, 3000, "small", "small", False),
    "table": ([300, 240, 170, 120, 75, 44, 30], 320, 37, 3000, "packed", "packed_fixed", True),
    "packed_fixed": ([300, 220, 151, 150, 90], 150, 39, 3000, "packed", "packed_fixed", False),
    "packed_runtime": ([520, 350, 330, 300, 120, 45], 400, 21, 3000, "packed", "packed_runtime", False),
    "packed_big": ([905, 577, 330, 120], 600, 43, 3000, "packed", "packed_big", False),
}
UNC_PERM = 4
UNC_SEED = 23
# offsets of one sign, b_j = a_j U(0, ONE_SIGN): u comes close to the constant
# vector. The largest of 0.5, 0.25, ... that keeps var_u >= 0.05 on every item
# of both shapes (chosen on the CPU from the oracle's side; asserted below).
ONE_SIGN = 0.5


def affine(x, seed, one_sign=None):
    """y_j = a_j x_j + b_j: a_j log-uniform in [0.25, 4], b_j = a_j U(-0.5, 0.5)
    (one_sign: a_j U(0, one_sign)). corr and net of the data do not change."""
    rng = np.random.default_rng(seed)
    a = np.exp(rng.uniform(np.log(0.25), np.log(4.0), x.shape[1]))
    b = a * (rng.uniform(-0.5, 0.5, x.shape[1]) if one_sign is None else rng.uniform(0.0, one_sign, x.shape[1]))
    return np.asfortranarray(x * a + b)


def cancellation_margins(y, mi, pis):
    """From the oracle's side, over the observed and every null item: the
    smallest var_u = 1 - S u_bar^2 of a summary profile, and the smallest
    var_x / G_jj = 1 - S m_j^2 / G_jj of a column. Both well above zero: the
    kernels' centred moments lose no digits to cancellation."""
    s = y.shape[0]
    m = y.mean(axis=0)
    var_x = 1.0 - s * m * m / (y * y).sum(axis=0)
    var_u = 1.0
    items = [mi.test_idx] + [mi.random_idx(pi.astype(np.int64)) for pi in pis]
    for item in items:
        for mod in mi.mods_present:
            srt, _ = O.sort_nodes(item[mod])
            u = O.summary_profile(y, srt)
            var_u = min(var_u, 1.0 - s * u.mean() ** 2)
    return float(var_u), float(np.nanmin(var_x))


class Uncentred:
    def __init__(self, cls, one_sign=None, oracle=True):
        sizes, s, seed, n_nodes, *_ = UNCENTRED[cls]
        lay, self.mi, self.disc, txs, self.tc, self.tn = _case(sizes, s, seed, n_nodes=n_nodes)
        self.y = affine(txs, seed + 1000, one_sign)
        self.pis = N.prp_table(UNC_SEED, 0, UNC_PERM, self.mi.null_idx.size)
        _freeze(self.y, self.tc, self.tn)
        if oracle:
            self.margins = cancellation_margins(self.y, self.mi, self.pis)
            self.exp, self.obs = _cpp(self.mi, self.disc, self.y, self.tc, self.tn, self.pis)
            _freeze(self.exp, self.obs)


def _uncentred_vs_oracle(cls, d, tag):
    sizes, s, _, n_nodes, p_cls, p_kernel, table = UNCENTRED[cls]
    # the launch of the largest modules is the class under test
    R.assert_planned(sizes, s, n_nodes, p_cls, p_kernel, table, UNC_PERM, first_only=True)
    var_u, var_x = d.margins
    print(f"{tag}, {cls}: min var_u {var_u:.3f}, min var_x / G_jj {var_x:.3f}")
    assert var_u >= 0.05 and var_x >= 0.5
    eng = _engine_from(d.mi, d.disc, d.y, d.tc, d.tn)
    obs = eng.observed()
    nulls = eng.run(0, UNC_PERM, UNC_SEED)
    assert eng.gram_table() == table
    e_obs = assert_stats_close(obs, d.obs, what=f"observed ({tag}, {cls})")
    e_null = assert_stats_close(nulls, d.exp, what=f"nulls ({tag}, {cls})")
    e_vec = _vectors_vs_oracle(eng, d.y, [d.mi.test_idx[m] for m in d.mi.mods_present], 1e-2, f"{tag}, {cls}")
    record(f"{tag}: {cls}", max(e_obs, e_null, e_vec), observed=e_obs, nulls=e_null, vectors=e_vec,
           min_var_u=var_u, min_var_x_over_gjj=var_x)
    eng.close()


@pytest.fixture(scope="module", params=list(UNCENTRED))
def uncentred(request):
    return request.param, Uncentred(request.param)


def test_uncentred_data_vs_cpp_oracle(uncentred):
    cls, d = uncentred
    _uncentred_vs_oracle(cls, d, "uncentred data")


@pytest.mark.parametrize("cls", ["wave", "table"])
def test_uncentred_data_offsets_of_one_sign(cls):
    """Every offset positive: the column means add up in u_bar instead of
    cancelling, and u comes close to the constant vector."""
    _uncentred_vs_oracle(cls, Uncentred(cls, one_sign=ONE_SIGN), "uncentred data, offsets of one sign")


def test_uncentred_data_nan_column_gives_na():
    """A NaN column inside a module of the table class, on transformed data:
    the module's summary-profile statistics are NA exactly where the oracle
    has them, in the observed row and in every null item that draws the
    column; everything else keeps the bar."""
    cls, d = "table", Uncentred("table", oracle=False)
    sizes, s, _, n_nodes, p_cls, p_kernel, table = UNCENTRED[cls]
    R.assert_planned(sizes, s, n_nodes, p_cls, p_kernel, table, 2)
    y = d.y.copy()
    m0 = d.mi.mods_present[2]
    y[:, d.mi.test_idx[m0][5]] = np.nan
    eng = _engine_from(d.mi, d.disc, y, d.tc, d.tn)
    obs = eng.observed()
    nulls = eng.run(0, 2, UNC_SEED)
    assert eng.gram_table() == table
    exp, exp_obs = O.permutation_procedure(d.disc, y, d.tc, d.tn, d.mi, d.pis[:2].astype(np.int64))
    assert_stats_close(obs, exp_obs, what="observed (uncentred data, NaN column)")
    assert_stats_close(nulls, exp, what="nulls (uncentred data, NaN column)")
    row = d.mi.modules.index(m0)
    assert not np.isfinite(obs[row, [1, 4, 6]]).any()
    assert np.isfinite(obs[[r for r in range(obs.shape[0]) if r != row]]).all()
    eng.close()
