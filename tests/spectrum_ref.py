"""Designed data for the summary-profile kernels: scaled data blocks whose
correlation matrix has an exactly prescribed spectrum, datasets that lay such
blocks side by side, permutation tables that send a module's null items onto
them, and a small numpy emulation of the kernels' Lanczos stop rule that
certifies the case table on the CPU. numpy / scipy only; test infrastructure.

The spectra are what the eigen-solver's rules rest on (kernels.hip,
lanczos_ritz): the gap between the two top eigenvalues, how many eigenvalues
crowd the top, and the numerical rank. CASES is the table both
tests/test_spectrum_host.py (CPU: certifies every case) and
tests/test_gpu_spectra.py (GPU: runs them) read."""
import functools
import os
import subprocess

import numpy as np
import scipy.linalg
from scipy.stats import random_correlation

# The kernels' rules the emulator restates (netrep_amd/csrc/kernels.hip, lanczos_ritz).
LZ_TOL = 5e-15          # stop: residual <= LZ_TOL * theta
FIRST_CHECK = 16        # first convergence check (the wave class: 18)
CHECK_EVERY = 8         # later checks come at most this many steps apart


def step_cap(k_gram):
    """profile_m_max (netrep_amd/csrc/profile_plan.hip) of a Lanczos dimension
    k_gram = min(k, S): the basis columns, i.e. the step cap."""
    return min(k_gram, 160) if k_gram <= 320 else 320


# ----------------------------------------------------------------------------
# spectrum families (r: the number of non-zero eigenvalues)
# ----------------------------------------------------------------------------

def pair(r, g):
    return np.concatenate([[1.0, 1.0 - g], 0.6 * np.linspace(1.0, 0.02, r - 2) ** 2])


def cluster(r, c, width):
    return np.concatenate([np.linspace(1.0, 1.0 - width, c), np.linspace(0.5, 0.01, r - c)])


def flat(r, width):
    return np.concatenate([np.linspace(1.0, 1.0 - width, r - 1), [0.3]])


def spectrum(spec, k, n_samples):
    """The k eigenvalues (descending, unnormalised) of a family given as a
    tuple: ("pair", g), ("cluster", c, width), ("flat", width), ("half_rank",),
    ("rank3",). The full-rank families take r = min(k, S - 1) non-zero values
    (a scaled S x k block has no higher rank); half_rank is pair(1e-2) on
    r = k / 2 (bounded by S - 1 likewise), rank3 is [1, 0.8, 0.5]; the rest
    exactly zero."""
    r_max = min(k, n_samples - 1)
    name = spec[0]
    if name == "pair":
        w = pair(r_max, spec[1])
    elif name == "cluster":
        w = cluster(r_max, spec[1], spec[2])
    elif name == "flat":
        w = flat(r_max, spec[1])
    elif name == "half_rank":
        w = pair(min(k // 2, r_max), 1e-2)
    elif name == "rank3":
        w = np.array([1.0, 0.8, 0.5])
    else:
        raise ValueError(spec)
    return np.concatenate([w, np.zeros(k - w.size)])


def spec_name(spec):
    return spec[0] + "".join(f"_{v:g}" for v in spec[1:])


def top_gap(spec, k, n_samples):
    w = spectrum(spec, k, n_samples)
    return (w[0] - w[1]) / w[0]


# ----------------------------------------------------------------------------
# designed data
# ----------------------------------------------------------------------------

def designed_block(eig, n_samples, rng):
    """An S x k block with column means 0, column sd 1 (n - 1) and the
    correlation spectrum `eig` (k values, descending, non-negative, scaled here
    to sum k; at most min(k, S - 1) non-zero): C = random_correlation.rvs(eig),
    X = sqrt(S - 1) U diag(sqrt(w)) V^T over C's designed-non-zero eigenpairs
    (w, V) and an S x r matrix U of orthonormal zero-mean columns, so that
    X^T X / (S - 1) = V diag(w) V^T has unit diagonal and exact rank r."""
    eig = np.asarray(eig, dtype=np.float64)
    k = eig.size
    r = int(np.count_nonzero(eig))
    assert (np.diff(eig) <= 0).all() and (eig >= 0).all() and 2 <= r <= min(k, n_samples - 1), (k, r, n_samples)
    eig = eig * (k / eig.sum())
    for _ in range(4):          # the rounding remainder on the first entry (rvs checks the sum)
        eig[0] += k - eig.sum()
    c = random_correlation.rvs(eig, random_state=rng, tol=1e-10, diag_tol=1e-7)
    c = 0.5 * (c + c.T)
    np.fill_diagonal(c, 1.0)
    w, v = np.linalg.eigh(c)
    w, v = w[::-1][:r], v[:, ::-1][:, :r]   # rvs leaves rounding-level values in place of the zeros: dropped
    u = rng.standard_normal((n_samples, r))
    u -= u.mean(axis=0)
    u, _ = np.linalg.qr(u)                  # an orthonormal basis of centred columns: zero-mean itself
    u -= u.mean(axis=0)
    return np.sqrt(n_samples - 1.0) * (u * np.sqrt(w)) @ v.T


def block_dataset(blocks, n_samples, n_background, rng):
    """The blocks side by side in the columns of one S x N data matrix,
    followed by n_background noise columns scaled as the oracle scales
    ((x - mean) / sd, n - 1). Returns (data, corr, net, positions):
    corr = X^T X / (S - 1) made exactly symmetric with a unit diagonal,
    net = |corr|^5, positions[i] the columns of blocks[i]."""
    pos, o = [], 0
    for b in blocks:
        assert b.shape[0] == n_samples
        pos.append(np.arange(o, o + b.shape[1]))
        o += b.shape[1]
    bg = rng.standard_normal((n_samples, n_background))
    bg = (bg - bg.mean(axis=0)) / bg.std(axis=0, ddof=1)
    x = np.asfortranarray(np.concatenate(list(blocks) + [bg], axis=1))
    corr = (x.T @ x) / (n_samples - 1.0)
    corr = np.triu(corr) + np.triu(corr, 1).T
    np.fill_diagonal(corr, 1.0)
    return x, corr, np.abs(corr) ** 5, pos


def rotation_tables(mi, blocks_of_module, n_perm, rng):
    """Explicit permutation tables (n_perm x n_null, pi[p][q] = source
    position in the null pool) for Engine.run(pi=...) and
    ref_cpp.permutation_procedure(pi=...): row p sends module m's null_pos to
    the pool positions of replica p mod R_m of m's blocks
    (blocks_of_module[m]: R_m arrays of test-data columns, each as long as
    the module; modules without an entry are left to the fill), in an order
    shuffled within the block; the remaining entries
    take the remaining pool positions, shuffled, so every row is a permutation
    of the pool. A null item of module m is then a designed block itself --
    a random draw from the pool would have no designed spectrum."""
    n_null = mi.null_idx.size
    pool_of = {int(c): q for q, c in enumerate(mi.null_idx)}
    pis = np.empty((n_perm, n_null), dtype=np.uint32)
    for p in range(n_perm):
        row = np.full(n_null, -1, dtype=np.int64)
        used = np.zeros(n_null, dtype=bool)
        for m, reps in blocks_of_module.items():
            src = np.array([pool_of[int(c)] for c in reps[p % len(reps)]], dtype=np.int64)
            assert src.size == mi.null_pos[m].size and not used[src].any()
            row[mi.null_pos[m]] = rng.permutation(src)
            used[src] = True
        free = row < 0
        row[free] = rng.permutation(np.nonzero(~used)[0])
        assert np.array_equal(np.sort(row), np.arange(n_null))
        pis[p] = row
    return pis


# ----------------------------------------------------------------------------
# the kernels' Lanczos run, emulated
# ----------------------------------------------------------------------------

def lanczos_steps(G, cap=None, first_check=FIRST_CHECK, start="column"):
    """Steps of the kernels' Lanczos run on the symmetric G: start G e_c* for
    the column c* of largest norm (start="column", kernels.hip start_column;
    "constant": the all-ones start of the full-Gram kernel, whose 1% hashed
    ripple is left out), the three-term step with full reorthogonalisation
    (what the kernels' partial one amounts to), stopped at the first step
    >= first_check whose top Ritz pair has residual beta_j |y_j| <=
    5e-15 theta, or at min(dim, cap). Returns (steps, capped): capped when the
    cap ended the run unconverged. The kernels stop at a check only, and
    checks come at most 8 steps apart: they take up to 8 steps more."""
    n = G.shape[0]
    mcap = n if cap is None else min(n, cap)
    if start == "column":
        q = G[:, int(np.argmax((G * G).sum(axis=0)))].astype(np.float64)
    else:
        q = np.ones(n)
    q = q / np.linalg.norm(q)
    Q = np.zeros((n, mcap + 1))
    Q[:, 0] = q
    al, be = [], []
    qp, b = np.zeros(n), 0.0
    for j in range(mcap):
        w = G @ q - b * qp
        a = q @ w
        w -= a * q
        for _ in range(2):
            w -= Q[:, :j + 1] @ (Q[:, :j + 1].T @ w)
        b = np.linalg.norm(w)
        al.append(a)
        be.append(b)
        if j + 1 >= min(first_check, mcap):
            if j == 0:
                theta, y_last = a, 1.0
            else:
                ev, evec = scipy.linalg.eigh_tridiagonal(np.array(al), np.array(be[:-1]), select="i",
                                                         select_range=(j, j))
                theta, y_last = ev[0], evec[-1, 0]
            if b * abs(y_last) <= LZ_TOL * abs(theta):
                return j + 1, False
        if j + 1 == mcap:
            break
        qp, q = q, w / b
        Q[:, j + 1] = q
    return mcap, mcap < n


# ----------------------------------------------------------------------------
# the case table (tests/test_spectrum_host.py certifies it, tests/test_gpu_spectra.py runs it)
# ----------------------------------------------------------------------------

PAIRS = [("pair", 1e-1), ("pair", 1e-2), ("pair", 1e-3), ("pair", 3e-4)]
CLUSTER40, FLAT, HALF, RANK3 = ("cluster", 40, 0.05), ("flat", 0.3), ("half_rank",), ("rank3",)
# the spectrum that reaches the step cap (recorded, not repaired: DESIGN.md section 8)
CAP_SPECTRUM = ("cluster", 140, 0.05)

# class -> (S, {module size: spectra}, planned class, planned kernel, Gram table).
# The smallest shapes that reach each class; primal designed blocks need k <= S - 1.
CASES = {
    "wave": (104, {150: PAIRS + [FLAT, HALF, RANK3], 96: PAIRS + [FLAT, HALF, RANK3],
                   33: PAIRS + [FLAT, HALF, RANK3]}, "wave", "wave", False),
    "small": (300, {112: PAIRS + [FLAT, HALF, RANK3], 64: PAIRS + [FLAT, HALF, RANK3]}, "small", "small", False),
    "packed_fixed": (150, {300: PAIRS + [HALF], 140: PAIRS + [HALF]}, "packed", "packed_fixed", False),
    "table": (320, {300: PAIRS + [CLUSTER40, FLAT, HALF, RANK3], 200: PAIRS + [CLUSTER40, FLAT, HALF, RANK3],
                    161: PAIRS + [HALF, RANK3], 96: PAIRS + [HALF, RANK3]}, "packed", "packed_fixed", True),
    "packed_runtime": (400, {520: [("pair", 1e-2), ("pair", 3e-4), CLUSTER40],
                             350: [("pair", 1e-2), ("pair", 3e-4), CLUSTER40]}, "packed", "packed_runtime", False),
    "packed_big": (600, {905: [("pair", 1e-3), ("pair", 3e-4)], 577: [("pair", 1e-3), ("pair", 3e-4)]},
                   "packed", "packed_big", False),
    "full_gram": (1800, {1744: [("pair", 1e-3)]}, "full_partials_in_scratch", "full_gram", False),
}

# the spectra that crowd the top: many Lanczos steps, held under the step cap by the host test
SLOW = (CLUSTER40, FLAT)

# The cap cases: class -> (S, module size, planned kernel, Gram table); one
# module, every replica of CAP_SPECTRUM. A Lanczos run ends by its dimension,
# so only the largest modules of the 160-step layouts leave room for a run of
# 1.5 times the cap: 320 nodes, primal on the table (S = 400) and dual on the
# matrix-core Gram (S = 319: a module with more nodes than samples keeps the
# dataset off the table). In this emulator cluster(80, 0.05) ends after 195
# steps at these sizes, cluster(140, 0.05) after 249.
CAP_CASES = {"table": (400, 320, "packed_fixed", True), "packed_fixed": (319, 320, "packed_fixed", False)}
CAP_REPLICAS = 3
CAP_DRAWS = (0, 3, 6)   # (three draws within about a quarter of the conditioning bound, as REDRAW below)

# Blocks whose first draw came within a factor 4 of the host test's
# conditioning bound (the two LAPACK drivers' statistics or per-node vectors
# more than 2.5e-12 apart, against the bound of 1e-11; the worst first draws:
# 4.1e-11, 3.4e-11, 1.5e-11): the first later draw of the same spectrum with at
# most 2.5e-12 takes their place. The margin is for LAPACK itself: its
# threaded drivers do not repeat bit for bit, and one block measured 4.2e-12
# in one process and 1.06e-11 in another. The draw is chosen by the reference's
# conditioning alone (tests/test_spectrum_host.py), on the CPU, never by a GPU
# result.
REDRAW = {
    ("wave", 96, ("pair", 1e-3)): 2,
    ("wave", 33, ("pair", 3e-4)): 1,
    ("small", 112, ("pair", 1e-3)): 1,
    ("small", 112, ("pair", 3e-4)): 1,
    ("small", 112, ("flat", 0.3)): 1,
    ("packed_fixed", 300, ("pair", 1e-3)): 3,
    ("packed_fixed", 300, ("pair", 3e-4)): 3,
    ("packed_fixed", 140, ("pair", 1e-3)): 1,
    ("table", 200, ("pair", 1e-3)): 1,
    ("table", 161, ("pair", 1e-3)): 3,
    ("table", 161, ("pair", 3e-4)): 1,
    ("table", 96, ("pair", 3e-4)): 1,
    ("packed_big", 577, ("pair", 3e-4)): 2,
}


def case_seed(cls, k, spec):
    """One fixed seed per (class, module size, spectrum): the host test
    certifies exactly the block the GPU test runs."""
    import zlib
    draw = REDRAW.get((cls, k, spec), 0)
    return zlib.crc32((f"{cls}/{k}/{spec_name(spec)}" + (f"/draw{draw}" if draw else "")).encode())


@functools.lru_cache(maxsize=None)
def case_block(cls, n_samples, k, spec):
    """The block of a case (shared between tests: leave it unchanged)."""
    x = designed_block(spectrum(spec, k, n_samples), n_samples, np.random.default_rng(case_seed(cls, k, spec)))
    x.setflags(write=False)
    return x


def cap_block(cls, replica):
    n_samples, k = CAP_CASES[cls][:2]
    return case_block(f"{cls}/cap{CAP_DRAWS[replica]}", n_samples, k, CAP_SPECTRUM)


def all_cases():
    return [(cls, s, k, spec) for cls, (s, sizes, *_) in CASES.items() for k, specs in sizes.items() for spec in specs]


def case_id(case):
    cls, s, k, spec = case
    return f"{cls}-S{s}-k{k}-{spec_name(spec)}"


# ----------------------------------------------------------------------------
# the planner's answer for a launch (host code, no GPU)
# ----------------------------------------------------------------------------

PLAN_CHECK = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "netrep_amd", "_lib",
                          "profile_plan_check")


def launch_plans(sizes, n_samples, n_nodes, n_perm=1):
    """The plans of the summary-profile launches of modules of `sizes` nodes
    (engine.hip, launch_profiles: the modules beyond the packed kernel's
    320-node layout in one launch, the rest in another, each planned for its
    largest module), as `profile_plan_check plans` prints them: a list of
    dicts, largest modules first."""
    assert os.path.exists(PLAN_CHECK), f"{PLAN_CHECK} missing: __graft_entry__.build() makes it"
    segs = [[k for k in sizes if k > 320], [k for k in sizes if k <= 320]]
    segs = [s for s in segs if s]
    lines = "".join(f"{max(s)} {n_samples} {len(s) * n_perm} {n_nodes * n_samples + 2 * n_samples}\n" for s in segs)
    r = subprocess.run([PLAN_CHECK, "plans"], input=lines, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = [dict(kv.split("=") for kv in ln.split()) for ln in r.stdout.splitlines()]
    out = [o for o in out if "table_kernel" not in o]
    assert len(out) == len(segs) and all(o["status"] == "0" for o in out), r.stdout
    return out


def assert_planned(sizes, n_samples, n_nodes, cls, kernel, table, n_perm=1, first_only=False):
    """Every launch of these modules (first_only: the launch of the largest
    ones) is planned on the class and kernel the case is meant to reach, and
    its plan takes the Gram table or not as intended: if the planner moves a
    boundary, the case fails here instead of silently testing another kernel."""
    plans = launch_plans(sizes, n_samples, n_nodes, n_perm)
    for p in plans[:1] if first_only else plans:
        got = (p["class"], p["kernel"], p["takes_table"] == "1")
        assert got == (cls, kernel, table), (f"modules {sorted(sizes)} at S = {n_samples}: planned {got}, "
                                             f"the case is meant for {(cls, kernel, table)}")
