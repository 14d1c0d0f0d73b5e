"""Eigengenes, module membership and close-module merging on a resident
from-data dataset, in one process on one GPU:

  (a) at the metric's shape (20,000 genes x 500 samples, beta = 5, unsigned,
      tom=True, module-structured data) with the labels of a static cut of the
      dataset's own dendrogram: the wall time of the eigengene call
      (Engine.module_eigengenes) against module_vectors (what net_props runs)
      for the same index sets on the same engine; the kME kernels' device time
      (nr_membership_ms) and the share of the HBM peak it reaches for its
      8 S n + 8 n M bytes; the whole merge loop on a handle and its rounds.
  (b) at 8,000 x 500: FromDataDataset.module_membership against the numpy
      route -- the host's data, an SVD per module and corrcoef, on the host's
      threads -- with both wall times and the largest difference.

Writes the record to --out (default profiles/eigengene/record.json) and prints
it as one JSON line. Run it as one command under its own timeout.

    python tools/eigengene_record.py [--n 20000] [--n-host 8000] [--s 500] [--out PATH]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import netrep_amd as N  # noqa: E402
from netrep_amd.api import RMatrix  # noqa: E402

HBM_PEAK_GBS = 8000.0


def module_data(n, s, seed, n_factors):
    """Module-structured data: every node loads on one of n_factors latent
    factors (or on none: one node in five is background noise); every other
    factor is correlated at 0.9 with the one before it."""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((s, n_factors + 1))
    for j in range(1, n_factors, 2):
        f[:, j] = 0.9 * f[:, j - 1] + np.sqrt(1 - 0.81) * f[:, j]
    f[:, n_factors] = 0.0
    which = rng.integers(0, n_factors, n)
    which[rng.random(n) < 0.2] = n_factors
    x = f[:, which] * rng.uniform(0.6, 1.0, n) + 0.6 * rng.standard_normal((s, n))
    return np.asfortranarray(x)


def static_labels(tree, min_size, want):
    """Labels of the static cut, on a fixed grid of heights, with the module
    count closest to `want`."""
    best = None
    for cut in np.linspace(0.80, 0.999, 60):
        labels = N.cutreeStatic(tree, float(cut), min_size)
        m = int(np.unique(labels[labels > 0]).size)
        if best is None or abs(m - want) < abs(best[1] - want):
            best = (float(cut), m, labels)
    return best


def csr(labels):
    mods = np.unique(labels[labels > 0])
    idx = [np.flatnonzero(labels == m) for m in mods]
    return np.cumsum([0] + [i.size for i in idx]).astype(np.int64), np.concatenate(idx).astype(np.int32)


def timed(fn, repeats=3):
    out, wall = None, []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        wall.append(time.perf_counter() - t0)
    return out, wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--n-host", type=int, default=8000)
    ap.add_argument("--s", type=int, default=500)
    ap.add_argument("--beta", type=float, default=5.0)
    ap.add_argument("--out", default=os.path.join("profiles", "eigengene", "record.json"))
    a = ap.parse_args()
    s = a.s
    rec = {"s": s, "beta": a.beta, "net_type": "unsigned", "tom": True, "hbm_peak_gbs": HBM_PEAK_GBS}

    # (a)
    n = a.n
    names = [f"g{i}" for i in range(n)]
    x = module_data(n, s, 20, 50)
    with N.FromDataDataset(RMatrix(x, None, names), a.beta, tom=True) as ds:
        tree = ds.hclust()
        cut, m, labels = static_labels(tree, 30, 50)
        merged, merge_wall = timed(lambda: ds.merge_close_modules(labels, 0.25), 2)
        _table, table_wall = timed(lambda: ds.module_membership(labels), 2)
    node_off, idx = csr(labels)
    with N.Engine(0) as eng:
        eng.set_dataset_from_data(x, a.beta, "unsigned", scale=True, tom=True)
        _e, eig_wall = timed(lambda: eng.module_eigengenes(node_off, idx))
        _v, vec_wall = timed(lambda: eng.module_vectors(node_off, idx, True))
        eng.module_eigengenes(node_off, idx)
        kme_ms = []
        for _ in range(5):
            eng.module_membership(m)
            kme_ms.append(eng.membership_ms())
    nbytes = 8 * s * n + 8 * n * m
    rec["a"] = dict(n=n, cut_height=cut, modules=m, labelled_nodes=int((labels > 0).sum()),
                    largest_module=int(np.diff(node_off).max()),
                    module_eigengenes_wall_s=eig_wall, module_vectors_wall_s=vec_wall,
                    speedup_over_module_vectors=min(vec_wall) / min(eig_wall),
                    membership_ms=kme_ms, membership_bytes=nbytes,
                    membership_gbs=nbytes / (min(kme_ms) * 1e-3) / 1e9,
                    membership_share_of_hbm_peak=nbytes / (min(kme_ms) * 1e-3) / 1e9 / HBM_PEAK_GBS,
                    membership_table_wall_s=table_wall,
                    merge_loop_wall_s=merge_wall, merge_rounds=merged["rounds"],
                    modules_after_merge=int(np.unique(merged["labels"][merged["labels"] > 0]).size))

    # (b)
    n = a.n_host
    names = [f"g{i}" for i in range(n)]
    x = module_data(n, s, 21, 20)
    with N.FromDataDataset(RMatrix(x, None, names), a.beta, tom=True) as ds:
        cut, m, labels = static_labels(ds.hclust(), 30, 20)
        table, wall_dev = timed(lambda: ds.module_membership(labels), 2)
    t0 = time.perf_counter()
    xs = (x - x.mean(axis=0)) / x.std(axis=0, ddof=1)
    mods = np.unique(labels[labels > 0])
    eig = np.empty((s, mods.size))
    for j, lab in enumerate(mods):
        cols = xs[:, labels == lab]
        u = np.linalg.svd(cols, full_matrices=False)[0][:, 0]
        eig[:, j] = -u if np.corrcoef(cols.mean(axis=1), u)[0, 1] < 0 else u
    t1 = time.perf_counter()
    host = np.corrcoef(xs.T, eig.T)[:n, n:]
    t2 = time.perf_counter()
    ec = eig - eig.mean(axis=0)                      # the same table by centred dot products (xs is centred)
    host2 = (xs.T @ ec) / np.sqrt((xs * xs).sum(axis=0))[:, None] / np.sqrt((ec * ec).sum(axis=0))[None, :]
    t3 = time.perf_counter()
    wall_host = t2 - t0
    rec["b"] = dict(n=n, cut_height=cut, modules=int(mods.size), device_route_wall_s=wall_dev,
                    host_route_wall_s=wall_host, speedup=wall_host / min(wall_dev),
                    host_route_parts_s=dict(scale_and_svd=t1 - t0, corrcoef=t2 - t1, centred_dot_products_instead=t3 - t2),
                    speedup_with_dot_products=(t1 - t0 + t3 - t2) / min(wall_dev),
                    dot_products_difference=float(np.abs(table.values - host2).max()),
                    host_threads=int(os.environ.get("OMP_NUM_THREADS", "0")) or os.cpu_count(),
                    largest_difference=float(np.abs(table.values - host).max()))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(rec, sort_keys=True))
    assert rec["b"]["largest_difference"] <= 1e-8, "the device table and the numpy route differ"


if __name__ == "__main__":
    main()
