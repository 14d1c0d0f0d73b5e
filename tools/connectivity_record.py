"""Connectivity by module on a resident from-data dataset, in one process on
one GPU:

  (a) at the metric's shape (20,000 genes x 500 samples, beta = 5, unsigned,
      tom=True, module-structured data) with the labels of the static cut that
      tools/eigengene_record.py uses: the device time of the connectivity
      kernel (nr_connectivity_ms) on the pair array and again on the Gram
      table that a permutation run leaves, the rate it reaches for its
      16 n^2 (pair array) or 32 n^2 (Gram table) bytes per pass against the
      HBM peak, the number of passes, and the wall time of
      FromDataDataset.module_connectivity and node_order. Every list holds
      the calls in order, the first call first; "best" is their minimum.
  (b) at 8,000 x 500: FromDataDataset.module_connectivity against the route
      without it -- matrices(), then a one-hot product in numpy on the host's
      threads -- with both wall times and the largest relative difference
      between the two tables.

Writes the record to --out (default profiles/connectivity/record.json) and
prints it as one JSON line. Run it as one command under its own timeout.

    python tools/connectivity_record.py [--n 20000] [--n-host 8000] [--s 500] [--out PATH]
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

from eigengene_record import HBM_PEAK_GBS, csr, module_data, static_labels, timed  # noqa: E402

TILE_MAX = 64           # modules per pass at most (nr_module_connectivity): ceil(M / 64) passes


def slots_of(labels):
    mods = np.unique(labels[labels > 0])
    slot = np.full(labels.size, -1, dtype=np.int32)
    slot[labels > 0] = np.searchsorted(mods, labels[labels > 0])
    return slot, int(mods.size)


def kernel_times(eng, m, slot, repeats=5):
    out = []
    for _ in range(repeats):
        eng.module_connectivity(m, slot)
        out.append(eng.connectivity_ms())
    return out


def rate(bytes_per_pass, passes, ms):
    gbs = bytes_per_pass * passes / (min(ms) * 1e-3) / 1e9
    return dict(ms=ms, best_ms=min(ms), bytes_per_pass=bytes_per_pass, gbs=gbs, share_of_hbm_peak=gbs / HBM_PEAK_GBS,
                ms_per_pass_at_peak=bytes_per_pass / (HBM_PEAK_GBS * 1e9) * 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--n-host", type=int, default=8000)
    ap.add_argument("--s", type=int, default=500)
    ap.add_argument("--beta", type=float, default=5.0)
    ap.add_argument("--out", default=os.path.join("profiles", "connectivity", "record.json"))
    a = ap.parse_args()
    s = a.s
    rec = {"s": s, "beta": a.beta, "net_type": "unsigned", "tom": True, "hbm_peak_gbs": HBM_PEAK_GBS}

    # (a)
    n = a.n
    names = [f"g{i}" for i in range(n)]
    x = module_data(n, s, 20, 50)
    with N.FromDataDataset(RMatrix(x, None, names), a.beta, tom=True) as ds:
        cut, m, labels = static_labels(ds.hclust(), 30, 50)
        _table, table_wall = timed(lambda: ds.module_connectivity(labels))
        _order, order_wall = timed(lambda: ds.node_order(labels))
        _intra, intra_wall = timed(lambda: ds.intramodular_connectivity(labels))
    slot, m = slots_of(labels)
    passes = -(-m // TILE_MAX)
    rec["a"] = dict(n=n, cut_height=cut, modules=m, labelled_nodes=int((labels > 0).sum()), passes=passes,
                    module_connectivity_wall_s=table_wall, node_order_wall_s=order_wall,
                    intramodular_connectivity_wall_s=intra_wall)
    with N.Engine(0) as eng:
        eng.set_dataset_from_data(x, a.beta, "unsigned", scale=True, tom=True)
        rec["a"]["pair_array"] = rate(16 * n * n, passes, kernel_times(eng, m, slot))
        one = np.where(slot == 0, 0, -1).astype(np.int32)
        rec["a"]["pair_array_one_module"] = rate(16 * n * n, 1, kernel_times(eng, 1, one))
        many = (np.arange(n) % 150).astype(np.int32)                     # three passes of 50 modules
        rec["a"]["pair_array_150_modules"] = dict(rate(16 * n * n, 3, kernel_times(eng, 150, many, 3)), passes=3)
        # a permutation run on four 200-node modules (the packed class, more samples than nodes: the shapes
        # for which the run builds the Gram table) with this dataset as its own discovery side
        rng = np.random.default_rng(3)
        idx = np.sort(rng.permutation(n)[:800].reshape(4, 200), axis=1).astype(np.int32).ravel()
        node_off = np.arange(5, dtype=np.int64) * 200
        disc = eng.module_vectors(node_off, idx, True)
        eng.set_modules(4, np.arange(4), node_off, idx, np.arange(800), disc["corr"], disc["degree"],
                        disc["contribution"])
        eng.set_null_pool(idx)
        eng.run(0, 8, 77)
        rec["a"]["gram_table_after_the_run"] = eng.gram_table()
        if eng.gram_table():
            rec["a"]["gram_table"] = rate(32 * n * n, passes, kernel_times(eng, m, slot))

    # (b)
    n = a.n_host
    names = [f"g{i}" for i in range(n)]
    x = module_data(n, s, 21, 20)
    with N.FromDataDataset(RMatrix(x, None, names), a.beta, tom=True) as ds:
        cut, m, labels = static_labels(ds.hclust(), 30, 20)
        (table, k_total), wall_dev = timed(lambda: ds.module_connectivity(labels))
        t0 = time.perf_counter()
        _corr, net = ds.matrices()
        t1 = time.perf_counter()
    slot, m = slots_of(labels)
    t2 = time.perf_counter()
    w = net.values.copy()
    np.fill_diagonal(w, 0.0)
    onehot = np.zeros((n, m + 1))
    onehot[np.flatnonzero(slot >= 0), slot[slot >= 0]] = 1.0
    onehot[:, m] = 1.0                                                   # the last column gives kTotal
    host = w.T @ onehot
    t3 = time.perf_counter()
    wall_host = (t1 - t0) + (t3 - t2)
    got = np.column_stack([table.values, k_total])
    nz = host > 0
    rec["b"] = dict(n=n, cut_height=cut, modules=m, device_route_wall_s=wall_dev, host_route_wall_s=wall_host,
                    host_route_parts_s=dict(matrices=t1 - t0, one_hot_product=t3 - t2),
                    speedup=wall_host / min(wall_dev),
                    host_threads=int(os.environ.get("OMP_NUM_THREADS", "0")) or os.cpu_count(),
                    largest_relative_difference=float((np.abs(got[nz] - host[nz]) / host[nz]).max()))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(rec, sort_keys=True))
    assert rec["b"]["largest_relative_difference"] <= 1e-10, "the device table and the numpy route differ"


if __name__ == "__main__":
    main()
