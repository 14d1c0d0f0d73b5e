"""The column sweep (netrep_amd/csrc/sweep.hip) at every chunk regime and with
general network weights, against the numpy oracle on identical PRP shuffles.

A column is cut into LDS chunks (nr::sweep_chunk_rows: at most 160,000 bytes,
9,984 rows of {corr, net}); the kernels take one of three paths by the number
of chunks: one chunk, exactly two (the split travels in the slot record,
sw_range) and three or more (the bndh table). Everything keyed on an entry's
global index against its chunk -- the lane parity e0 + gl, the diagonal's rank
pj, the first term after it pj + 2 (sw_ff), the tail e > pj + 2, the column's
own row zeroed in one chunk only, a short last chunk, an item with no entry in
a chunk, the finish kernel's chunk-order sums -- exists only with two or more
chunks. The test knob NR_DEBUG_SWEEP_CHUNK_ROWS (nr_debug_set) lowers the cap
on the chunk height, so a 600-node network runs at 2, 3, 5 and 10 chunks and
a 1,024-node one at the limit of 16; a 10,048-node network runs the production
two-chunk shape with the knob untouched.

Every test first asserts on the host, from the engine's exported indices and
the chunk height in force, that its seed produces the situations it is there
for (`situations`); a seed that misses one fails. All cases are network-only
(the column sweep computes all four statistics), every cell is compared
(`assert_stats_close` at its defaults), and no module has two nodes.

The network weights: beside net = |corr|^5 with a unit diagonal (the synthetic
datasets), unsymmetric standard-normal matrices whose diagonal is drawn per
node from {0, 1, negative, ~1e-9, denormal, dominant}: the weighted-degree
cancellation model (wd_grid_exp, the fixed-point parts, sw_wd_final's
fallbacks, sw_fx's branch for terms >= 2^52 grid units) chooses its path per
column from |net(c, c)|. The dominant class proves its own sensitivity: plain
np.sum column sums miss the bar against the oracle there.
"""
import contextlib
import time

import numpy as np
import pytest

from netrep_amd import _lib as L
from netrep_amd import synthetic as S
from oracle import netrep_oracle as O
from oracle import prp

from conftest import FLOOR, RTOL, assert_stats_close, record
from test_gpu_parity import _engine_case, _engine_from

pytestmark = pytest.mark.gpu

SWEEP_CHUNK_BYTES = 160000      # kSweepChunkBytes
SWEEP_MAX_CHUNKS = 16           # kSweepMaxChunks
SWEEP_PRE = 6                   # kSweepPre: entries per lane in flight
SWEEP_WAVES = 16                # kSweepWaves
SIZES = (300, 150, 90, 40, 12, 3, 1)


def chunk_rows(n, elem_bytes=16, cap_rows=0):
    """nr::sweep_chunk_rows restated: balanced chunks of whole 64-row groups
    under the LDS cap (or the knob's lower one)."""
    lds_cap = SWEEP_CHUNK_BYTES // elem_bytes // 64 * 64
    cap = min(cap_rows, lds_cap) if cap_rows > 0 else lds_cap
    n_chunks = -(-n // cap)
    rows = -(-n // n_chunks)
    return min(cap, (rows + 63) // 64 * 64)


def n_chunks_of(n, rows):
    return -(-n // rows)


@contextlib.contextmanager
def chunk_height(cap_rows):
    """The knob for the block's duration (0: the production height)."""
    lib = L.load()
    assert lib.nr_debug_set(L.NR_DEBUG_SWEEP_CHUNK_ROWS, cap_rows) == L.NR_OK
    try:
        yield
    finally:
        lib.nr_debug_set(L.NR_DEBUG_SWEEP_CHUNK_ROWS, 0)


def situations(idx, node_off, n, rows, lanes=8):
    """Which chunk-edge situations the null items of `idx` ([perm, node]: the
    exported test columns) hold at `rows` rows per chunk. Entry e of an item is
    its e-th smallest column; chunk h holds the entries with column // rows ==
    h, entries e0[h] .. e0[h + 1]."""
    c = n_chunks_of(n, rows)
    last0 = (c - 1) * rows
    s = dict(empty_chunk=False, all_in_last_chunk=False, column_first_row_of_chunk=False,
             column_last_row_of_chunk=False, column_in_short_last_chunk=False,
             diag_and_first_after_in_different_chunks=False, first_after_diag_past_the_end=False,
             range_longer_than_the_prefetch=False, odd_e0=False, entries_in_every_chunk=False)
    for p in range(idx.shape[0]):
        for a, b in zip(node_off[:-1], node_off[1:]):
            cols = np.sort(idx[p, a:b])
            k = cols.size
            ch = cols // rows
            cnt = np.bincount(ch, minlength=c)
            e0 = np.concatenate([[0], np.cumsum(cnt)])
            s["first_after_diag_past_the_end"] |= k >= 1          # ranks k - 2, k - 1: pj + 2 >= k
            s["range_longer_than_the_prefetch"] |= bool((cnt > SWEEP_PRE * lanes).any())
            s["entries_in_every_chunk"] |= bool((cnt > 0).all())
            if c == 1:
                continue
            s["empty_chunk"] |= bool((cnt == 0).any())
            s["all_in_last_chunk"] |= bool(cnt[-1] == k)
            s["column_first_row_of_chunk"] |= bool(((cols % rows == 0) & (cols > 0)).any())
            s["column_last_row_of_chunk"] |= bool(((cols % rows == rows - 1) | (cols == n - 1)).any())
            s["column_in_short_last_chunk"] |= bool(n - last0 < rows and (cols >= last0).any())
            s["diag_and_first_after_in_different_chunks"] |= bool(k > 2 and (ch[:-2] != ch[2:]).any())
            s["odd_e0"] |= bool(((e0[1:c] % 2 == 1) & (cnt[1:] > 0)).any())
    s["column_over_two_wave_rounds"] = bool(np.bincount(idx.ravel()).max() > 2 * (64 // lanes) * SWEEP_WAVES)
    return s


EDGES = ("empty_chunk", "all_in_last_chunk", "column_first_row_of_chunk", "column_last_row_of_chunk",
         "diag_and_first_after_in_different_chunks", "first_after_diag_past_the_end", "odd_e0")


def assert_situations(idx, node_off, n, rows, need, lanes=8):
    got = situations(idx, node_off, n, rows, lanes)
    missing = [w for w in need if not got[w]]
    assert not missing, f"the seed does not produce {missing} at {rows} rows per chunk (n = {n})"


def pi_tables(mi, seed, n_perm):
    return prp.permutation_table(mi.null_idx.size, seed, 0, n_perm).astype(np.int64)


def assert_indices(idx, mi, pis):
    """The exported columns are the oracle's index sets (the situations are
    asserted on the former, the expected cube computed from the latter)."""
    for p in (0, idx.shape[0] - 1):
        ridx = mi.random_idx(pis[p])
        np.testing.assert_array_equal(idx[p], np.concatenate([ridx[m] for m in mi.mods_present]))


class Case:
    """A network-only dataset with its oracle cube, computed once."""

    def __init__(self, mi, disc, tc, tn, seed, n_perm):
        self.mi, self.disc, self.tc, self.tn, self.seed, self.n_perm = mi, disc, tc, tn, seed, n_perm
        self.n = tc.shape[0]
        self.pis = pi_tables(mi, seed, n_perm)
        self.exp, self.obs = O.permutation_procedure(disc, None, tc, tn, mi, self.pis, with_data=False)

    def engine(self):
        return _engine_from(self.mi, self.disc, None, self.tc, self.tn, with_data=False)

    def indices(self, eng):
        idx = eng.export_indices(0, self.n_perm, self.seed)
        assert_indices(idx, self.mi, self.pis)
        return idx

    def check(self, eng, what):
        e1 = assert_stats_close(eng.observed(), self.obs, what=f"observed, {what}")
        e2 = assert_stats_close(eng.run(0, self.n_perm, self.seed), self.exp, what=f"nulls, {what}")
        return max(e1, e2)


def synthetic_case(n, sizes, seed, n_perm, run_seed):
    _lay, mi, disc, _tx, tc, tn = _engine_case(n_nodes=n, n_samples=24, sizes=sizes, seed=seed, with_data=False)
    return Case(mi, disc, tc, tn, run_seed, n_perm)


# --------------------------------------------------------------------------
# B1. the chunk-edge matrix
# --------------------------------------------------------------------------

# 288 permutations: every column occurs ~286 times in the batch, so a wave of
# its workgroup (128 occurrences per round of the 16 waves) takes three
# batches and the metadata prefetch (cur, nxt, nn) is live three deep.
@pytest.fixture(scope="module")
def n600():
    return synthetic_case(600, SIZES, 11, 288, 23)


@pytest.fixture(scope="module")
def n1024():
    return synthetic_case(1024, SIZES, 12, 96, 24)


# (case, knob, chunks, situations required of the seed)
MATRIX = [
    ("n600", 0, 1, ("first_after_diag_past_the_end", "range_longer_than_the_prefetch",
                    "column_over_two_wave_rounds")),
    ("n600", 320, 2, EDGES + ("column_in_short_last_chunk", "range_longer_than_the_prefetch",
                              "column_over_two_wave_rounds")),
    ("n600", 256, 3, EDGES + ("column_in_short_last_chunk", "column_over_two_wave_rounds")),
    ("n600", 128, 5, EDGES + ("column_in_short_last_chunk", "entries_in_every_chunk")),
    ("n600", 64, 10, EDGES + ("column_in_short_last_chunk", "entries_in_every_chunk")),
    ("n1024", 64, 16, EDGES + ("entries_in_every_chunk",)),
]


@pytest.mark.parametrize("case,knob,chunks,need", MATRIX, ids=[f"{m[0]}-{m[2]}chunks" for m in MATRIX])
def test_chunk_edge_matrix_vs_oracle(request, case, knob, chunks, need):
    cs = request.getfixturevalue(case)
    rows = chunk_rows(cs.n, 16, knob)
    assert n_chunks_of(cs.n, rows) == chunks
    eng = cs.engine()
    try:
        assert_situations(cs.indices(eng), eng.node_off, cs.n, rows, need)
        with chunk_height(knob):
            err = cs.check(eng, f"n = {cs.n}, {chunks} chunks of {rows} rows")
    finally:
        eng.close()
    record(f"sweep chunks: n = {cs.n}, {chunks} chunk(s) of {rows} rows, modules {SIZES}", err, perms=cs.n_perm)


def test_rising_chunk_count_on_one_engine(n600):
    """1, 2, 3, 5 and 10 chunks in turn on one engine: the buffer sets regrow
    (P.n_chunks > b.chunk_cap) and the bndh table, which only exists beyond two
    chunks, is allocated after a smaller set was live; then back to one chunk
    on the larger buffers."""
    cs = n600
    eng = cs.engine()
    worst = 0.0
    try:
        last = 0
        for knob in (0, 320, 256, 128, 64, 0):
            rows = chunk_rows(cs.n, 16, knob)
            c = n_chunks_of(cs.n, rows)
            assert c > last or knob == 0
            last = c
            with chunk_height(knob):
                worst = max(worst, cs.check(eng, f"rising, {c} chunks of {rows} rows"))
    finally:
        eng.close()
    record("sweep chunks: 1, 2, 3, 5, 10, 1 chunks on one engine (n = 600)", worst, perms=cs.n_perm)


def test_knob_contract(n600):
    """A height that is no multiple of 64 is refused; more than 16 chunks is an
    error that names the knob, not another kernel; <= 0 restores the default."""
    lib = L.load()
    try:
        assert lib.nr_debug_set(L.NR_DEBUG_SWEEP_CHUNK_ROWS, 100) == L.NR_ERR_INVALID
        assert lib.nr_debug_set(L.NR_DEBUG_SWEEP_CHUNK_ROWS, 63) == L.NR_ERR_INVALID
    finally:
        lib.nr_debug_set(L.NR_DEBUG_SWEEP_CHUNK_ROWS, 0)
    _lay, mi, disc, _tx, tc, tn = _engine_case(n_nodes=1100, n_samples=8, sizes=(12, 3), seed=13, with_data=False)
    assert n_chunks_of(1100, chunk_rows(1100, 16, 64)) > SWEEP_MAX_CHUNKS
    eng = _engine_from(mi, disc, None, tc, tn, with_data=False)
    try:
        ref = eng.run(0, 4, 3)
        with chunk_height(64):
            with pytest.raises(L.NetRepError) as ex:
                eng.run(0, 4, 3)
            assert ex.value.code == L.NR_ERR_INVALID
            assert "NR_DEBUG_SWEEP_CHUNK_ROWS" in str(ex.value)
        with chunk_height(-5):
            got = eng.run(0, 4, 3)
        np.testing.assert_array_equal(got.view(np.uint64), ref.view(np.uint64))
    finally:
        eng.close()


# --------------------------------------------------------------------------
# B2. the sixteen-lane path over chunks
# --------------------------------------------------------------------------

@pytest.fixture(scope="module")
def wide():
    """test_wide_modules_sixteen_lane_sweep_vs_oracle's shapes, network-only:
    finite, and with its NaN correlation inside the wide module."""
    _lay, mi, disc, _tx, tc, tn = _engine_case(n_nodes=2600, n_samples=20, sizes=(1100, 40), seed=5,
                                               with_data=False)
    m0 = max(mi.mods_present, key=lambda m: mi.test_idx[m].size)
    a, b = mi.test_idx[m0][3], mi.test_idx[m0][10]
    tcn = tc.copy()
    tcn[a, b] = tcn[b, a] = np.nan
    return {False: Case(mi, disc, tc, tn, 31, 4), True: Case(mi, disc, tcn, tn, 31, 4)}


WIDE_NEED = {
    # 16 lanes: a chunk range longer than 6 x 16 = 96 entries enters the t0 loop
    2: ("range_longer_than_the_prefetch", "diag_and_first_after_in_different_chunks", "odd_e0",
        "column_in_short_last_chunk", "first_after_diag_past_the_end", "entries_in_every_chunk"),
    14: ("empty_chunk", "diag_and_first_after_in_different_chunks", "odd_e0", "column_first_row_of_chunk",
         "column_last_row_of_chunk", "column_in_short_last_chunk", "entries_in_every_chunk"),
}


@pytest.mark.parametrize("nonfinite", [False, True], ids=["finite", "nan-corr"])
@pytest.mark.parametrize("knob,chunks", [(1344, 2), (192, 14)])
def test_sixteen_lane_sweep_over_chunks_vs_oracle(wide, knob, chunks, nonfinite):
    cs = wide[nonfinite]
    rows = chunk_rows(cs.n, 16, knob)
    assert n_chunks_of(cs.n, rows) == chunks
    eng = cs.engine()
    try:
        assert eng.finite()[0] == (not nonfinite)
        idx = cs.indices(eng)
        # (1,100 and 40 nodes: no item leaves one of two chunks empty)
        assert_situations(idx, eng.node_off, cs.n, rows, WIDE_NEED[chunks], lanes=16)
        with chunk_height(knob):
            err = cs.check(eng, f"16 lanes, {chunks} chunks of {rows} rows, nonfinite={nonfinite}")
    finally:
        eng.close()
    record(f"sweep chunks: 16 lanes (n = 2,600, modules (1100, 40)), {chunks} chunks of {rows} rows, "
           f"{'NaN correlation' if nonfinite else 'finite'}", err, perms=cs.n_perm)


# --------------------------------------------------------------------------
# B3. complete-case records over chunks
# --------------------------------------------------------------------------

def _items_with_pair(idx, node_off, bad):
    """Null items (of two or more nodes) holding a pair (r, c), r != c, with bad[r, c]."""
    hits = 0
    for p in range(idx.shape[0]):
        for a, b in zip(node_off[:-1], node_off[1:]):
            cols = idx[p, a:b]
            sub = bad[np.ix_(cols, cols)].copy()
            np.fill_diagonal(sub, False)
            hits += bool(sub.any())
    return hits


@pytest.fixture(scope="module")
def nan_rows(n600):
    """n600 with NaN on the whole rows and columns of five nodes of the test
    correlation (the first 96 permutations)."""
    tc = n600.tc.copy()
    nodes = np.random.default_rng(3).choice(n600.n, 5, replace=False)
    tc[nodes, :] = np.nan
    tc[:, nodes] = np.nan
    return Case(n600.mi, n600.disc, tc, n600.tn, n600.seed, 96)


@pytest.mark.parametrize("knob,chunks", [(320, 2), (128, 5)])
def test_complete_case_records_over_chunks_vs_oracle(nan_rows, knob, chunks):
    cs = nan_rows
    rows = chunk_rows(cs.n, 16, knob)
    assert n_chunks_of(cs.n, rows) == chunks
    eng = cs.engine()
    try:
        assert eng.finite() == (False, True)
        idx = cs.indices(eng)
        assert_situations(idx, eng.node_off, cs.n, rows, EDGES + ("column_in_short_last_chunk",))
        assert _items_with_pair(idx, eng.node_off, ~np.isfinite(cs.tc)) > 0
        with chunk_height(knob):
            err = cs.check(eng, f"NaN rows and columns, {chunks} chunks of {rows} rows")
    finally:
        eng.close()
    record(f"sweep chunks: NaN rows / columns of corr (n = 600), {chunks} chunks of {rows} rows", err,
           perms=cs.n_perm)


# --------------------------------------------------------------------------
# B4. the production two-chunk shape, knob untouched
# --------------------------------------------------------------------------

def _production_case():
    """n = 10,048 (2 x 5,056 rows). One n x n pair is built, the test dataset:
    corr as a plain product of the normalised data (symmetric to rounding
    only), net = |corr|^5 by products; the discovery properties come from a
    512-node dataset over the same module sizes."""
    n, sizes = 10048, (300, 150, 40, 7)
    small = S.make_layout(512, sizes, 42)
    _dx, dc, dn = S.numpy_dataset(small, 24, 43)
    smi = O.ModuleIndex(small.names, small.labels, small.names, small.modules)
    disc = O.intermediate_properties(None, dc, dn, smi.disc_idx(small.names), with_data=False)
    lay = S.make_layout(n, sizes, 41)
    mi = O.ModuleIndex(lay.names, lay.labels, lay.names, lay.modules)
    x = S._gen_numpy(lay, 24, np.random.default_rng(44), set(lay.modules[::2]))
    x -= x.mean(axis=0)
    x /= np.sqrt((x * x).sum(axis=0))
    tc = (x.T @ x).T                      # column-major without a copy
    np.fill_diagonal(tc, 1.0)
    a = np.abs(tc)
    tn = a * a
    tn *= tn
    tn *= a
    del a
    return Case(mi, disc, tc, tn, 17, 16)


def test_production_two_chunk_shape_vs_oracle():
    """The shape of a 10,000-20,000 gene dataset with the knob untouched:
    n = 10,048 gives 2 x 5,056 rows, 80,896 bytes of LDS per workgroup."""
    t0 = time.perf_counter()
    cs = _production_case()
    n, n_perm = cs.n, cs.n_perm
    rows = chunk_rows(n)
    assert rows == 5056 and n_chunks_of(n, rows) == 2
    t1 = time.perf_counter()
    eng = cs.engine()
    try:
        idx = cs.indices(eng)
        for p in range(n_perm):                       # entries on both sides of row 5,056
            for a0, b0 in zip(eng.node_off[:-1], eng.node_off[1:]):
                if b0 - a0 >= 40:
                    assert (idx[p, a0:b0] < rows).any() and (idx[p, a0:b0] >= rows).any()
        assert_situations(idx, eng.node_off, n, rows,
                          ("diag_and_first_after_in_different_chunks", "odd_e0", "column_in_short_last_chunk",
                           "range_longer_than_the_prefetch", "entries_in_every_chunk", "empty_chunk"))
        err = cs.check(eng, "n = 10,048, production two chunks")
    finally:
        eng.close()
    t2 = time.perf_counter()
    print(f"production two-chunk shape: host set-up and oracle {t1 - t0:.2f} s, engine (upload, observed, "
          f"{n_perm} permutations) {t2 - t1:.2f} s")
    record("sweep chunks: n = 10,048, production 2 x 5,056 rows, modules (300, 150, 40, 7)", err, perms=n_perm,
           host_s=round(t1 - t0, 2), engine_s=round(t2 - t1, 2))


# --------------------------------------------------------------------------
# B5. general network weights
# --------------------------------------------------------------------------

DIAG_CLASSES = ("zero", "one", "negative", "tiny", "denormal", "dominant")


def _general_matrices(n, rng):
    """Unsymmetric standard-normal corr and net; the net diagonal per node from
    DIAG_CLASSES. The dominant values lie in [1.1, 1.9] x 2^20 with either
    sign: 4,000 or more times a 300-node module's column sum (~240), inside
    the fixed-point model's range (column sum < 2^-8 |diagonal|, sw_wd_final's
    2^60 check) and clear of the next binade (the model's chain check)."""
    corr = rng.standard_normal((n, n))
    net = rng.standard_normal((n, n))
    cls = rng.integers(0, len(DIAG_CLASSES), n)
    u = rng.uniform(0.0, 1.0, n)
    sign = rng.choice([-1.0, 1.0], n)
    diag = np.select([cls == 0, cls == 1, cls == 2, cls == 3, cls == 4, cls == 5],
                     [0.0, 1.0, -(0.5 + u), 1e-9 * (1.0 + u), 5e-320 * (1.0 + np.floor(100 * u)),
                      sign * (1.1 + 0.8 * u) * 2.0 ** 20])
    np.fill_diagonal(net, diag)
    return corr, net, cls


@pytest.fixture(scope="module")
def general():
    n = 600
    lay = S.make_layout(n, SIZES, 51)
    mi = O.ModuleIndex(lay.names, lay.labels, lay.names, lay.modules)
    rng = np.random.default_rng(52)
    dc, dn, _ = _general_matrices(n, rng)
    disc = O.intermediate_properties(None, dc, dn, mi.disc_idx(lay.names), with_data=False)
    tc, tn, cls = _general_matrices(n, rng)
    finite = Case(mi, disc, tc, tn, 29, 96)
    # non-finite weights: whole rows and columns of four nodes, and single entries
    tnn = tn.copy()
    nodes = rng.choice(n, 4, replace=False)
    for node, v in zip(nodes, (np.nan, np.inf, -np.inf, np.nan)):
        tnn[node, :] = v
        tnn[:, node] = v
    r, c = rng.integers(0, n, 40), rng.integers(0, n, 40)
    tnn[r, c] = np.tile([np.nan, np.inf, -np.inf, np.nan], 10)
    with np.errstate(invalid="ignore"):     # the reference's Inf - Inf on an infinite diagonal
        nonfinite = Case(mi, disc, tc, tnn, 29, 96)
    return dict(finite=finite, nonfinite=nonfinite, cls=cls)


def _naive_weighted_degree_stats(cs):
    """avg.weight and cor.degree of the null items with plain np.sum column
    sums in place of the reference's summation order (O.weighted_degree)."""
    out = np.full((len(cs.mi.modules), 2, cs.n_perm), np.nan)
    for p in range(cs.n_perm):
        ridx = cs.mi.random_idx(cs.pis[p])
        for m in cs.mi.mods_present:
            srt, rank = O.sort_nodes(ridx[m])
            sub = np.abs(cs.tn[np.ix_(srt, srt)])
            wd = (np.sum(sub, axis=0) - np.abs(cs.tn[srt, srt]))[rank]
            out[cs.mi.modules.index(m), :, p] = [O.average_edge_weight(wd),
                                                 O.correlation(cs.disc["degree"][m], wd)]
    return out


def test_general_weights_naive_sums_miss_the_bar(general):
    """The sensitivity of the general-weights cases, on the host: with plain
    column sums the statistics of the dominant-diagonal nodes miss the bar, so
    the engine passes only if its model reproduces the reference's rounding
    (the effect DESIGN.md section 5.1 cites)."""
    cs = general["finite"]
    naive = _naive_weighted_degree_stats(cs)
    exp = cs.exp[:, [0, 2], :]
    fin = np.isfinite(exp)
    assert (np.isfinite(naive) == fin).all()
    err = np.abs(naive[fin] - exp[fin]) / np.maximum(np.abs(exp[fin]), FLOOR)
    print(f"naive column sums against the oracle: max scaled error {err.max():.3e}, "
          f"{int((err > RTOL).sum())} of {err.size} cells over the bar")
    assert err.max() > 10 * RTOL
    # ... and the cause is the dominant class: without it the naive sums pass
    tn = cs.tn.copy()
    d = np.diagonal(tn).copy()
    d[general["cls"] == DIAG_CLASSES.index("dominant")] = 1.0
    np.fill_diagonal(tn, d)
    tame = Case(cs.mi, cs.disc, cs.tc, tn, cs.seed, 8)
    naive = _naive_weighted_degree_stats(tame)
    exp = tame.exp[:, [0, 2], :]
    fin = np.isfinite(exp)
    assert (np.abs(naive[fin] - exp[fin]) / np.maximum(np.abs(exp[fin]), FLOOR)).max() <= RTOL


@pytest.mark.parametrize("weights", ["finite", "nonfinite"])
@pytest.mark.parametrize("knob,chunks", [(0, 1), (320, 2), (128, 5)])
def test_general_weights_vs_oracle(general, knob, chunks, weights):
    cs = general[weights]
    rows = chunk_rows(cs.n, 16, knob)
    assert n_chunks_of(cs.n, rows) == chunks
    eng = cs.engine()
    try:
        assert eng.finite() == (True, weights == "finite")      # corr finite: the finite-data records stay on
        idx = cs.indices(eng)
        if chunks > 1:
            assert_situations(idx, eng.node_off, cs.n, rows, EDGES + ("column_in_short_last_chunk",))
        # every diagonal class is some null item's column in every module of 12 or more nodes
        for a, b in zip(eng.node_off[:-1], eng.node_off[1:]):
            if b - a >= 12:
                assert set(general["cls"][idx[:, a:b]].ravel()) == set(range(len(DIAG_CLASSES)))
        if weights == "nonfinite":
            assert _items_with_pair(idx, eng.node_off, ~np.isfinite(cs.tn)) > 0
        with chunk_height(knob):
            err = cs.check(eng, f"general weights ({weights}), {chunks} chunk(s) of {rows} rows")
    finally:
        eng.close()
    record(f"sweep chunks: general weights ({weights} net, n = 600), {chunks} chunk(s) of {rows} rows", err,
           perms=cs.n_perm)


# --------------------------------------------------------------------------
# B6. no CorrVector: sweep_column_kernel<false, false, L>, 8-byte LDS elements
# --------------------------------------------------------------------------

@pytest.fixture(scope="module")
def singles():
    return synthetic_case(600, (1,) * 8, 61, 96, 37)


@pytest.mark.parametrize("knob", [0, 64])
def test_single_node_modules_without_corrvector_vs_oracle(singles, knob):
    """Every present module has one node: no CorrVector pair anywhere, so the
    engine holds no discovery vector and the sweep runs its net-only
    instantiation (10 chunks of 64 rows with the knob). The reference's
    statistics of a one-node module are all NA (0 / 0 average weight, no pair,
    one degree); the cube is the oracle's, NA pattern included."""
    cs = singles
    rows = chunk_rows(cs.n, 8, knob)
    assert rows == (64 if knob else 640)
    assert sum(v.size for v in cs.disc["corr"].values()) == 0
    eng = cs.engine()
    try:
        idx = cs.indices(eng)
        if knob:
            assert_situations(idx, eng.node_off, cs.n, rows, ("empty_chunk", "all_in_last_chunk",
                                                               "column_in_short_last_chunk"))
        with chunk_height(knob):
            err = cs.check(eng, f"single-node modules, {n_chunks_of(cs.n, rows)} chunk(s) of {rows} rows")
    finally:
        eng.close()
    assert not np.isfinite(cs.exp).any()
    record(f"sweep chunks: eight single-node modules (n = 600), {n_chunks_of(cs.n, rows)} chunk(s)", err,
           perms=cs.n_perm)
