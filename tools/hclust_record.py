"""The average-linkage dendrogram of a resident from-data dataset
(nr_hclust_average / FromDataDataset.hclust), in one process on one GPU:

  (a) at the metric's shape (20,000 genes x 500 samples, beta = 5, unsigned,
      tom=True, module-structured data): the device time of the extract and
      all chain launches (nr_hclust_ms), the wall time of the call, the
      nearest-neighbour searches per node, the launches and the time per
      launch at the default merges per launch, and the scratch bytes.
  (b) at 8,000 x 500: FromDataDataset.hclust() against the route without it
      -- matrices() copied back, 1 - net, scipy's linkage(squareform(.),
      "average") on the host's threads -- with both wall times, their ratio,
      and the check that the two trees hold the same clusters (heights within
      (n + 16) 2^-52 relative).

Writes the record to --out (default profiles/hclust/record.json) and prints it
as one JSON line. Run it as one command under its own timeout.

    python tools/hclust_record.py [--n 20000] [--n-host 8000] [--s 500] [--out PATH]
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


def module_data(n, s, seed, n_factors):
    """Module-structured data: every node loads on one of n_factors latent
    factors (or on none: one node in five is background noise)."""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((s, n_factors + 1))
    f[:, n_factors] = 0.0
    which = rng.integers(0, n_factors, n)
    which[rng.random(n) < 0.2] = n_factors
    x = f[:, which] * rng.uniform(0.6, 1.0, n) + 0.6 * rng.standard_normal((s, n))
    return np.asfortranarray(x)


def cluster_keys(n, rows, heights, rng_seed=1):
    """{(size, sum of the leaves' random 64-bit keys): height} of a tree given
    as rows (x, y), ids below n leaves and n + t the cluster of row t."""
    key = np.random.default_rng(rng_seed).integers(0, 2 ** 63, n, dtype=np.uint64)
    size = np.ones(2 * n - 1, dtype=np.int64)
    ksum = np.zeros(2 * n - 1, dtype=np.uint64)
    ksum[:n] = key
    out = {}
    with np.errstate(over="ignore"):
        for t, (x, y) in enumerate(rows):
            x, y = int(x), int(y)
            size[n + t] = size[x] + size[y]
            ksum[n + t] = ksum[x] + ksum[y]                   # wraps: a sum mod 2^64
            out[(int(size[n + t]), int(ksum[n + t]))] = float(heights[t])
    return out


def merge_rows(n, merge):
    return [[(-c - 1) if c < 0 else n + c - 1 for c in (int(r[0]), int(r[1]))] for r in merge]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--n-host", type=int, default=8000)
    ap.add_argument("--s", type=int, default=500)
    ap.add_argument("--beta", type=float, default=5.0)
    ap.add_argument("--out", default=os.path.join("profiles", "hclust", "record.json"))
    a = ap.parse_args()
    s = a.s
    rec = {"s": s, "beta": a.beta, "net_type": "unsigned", "tom": True}

    # (a)
    n = a.n
    x = module_data(n, s, 20, 40)
    with N.Engine(0) as eng:
        eng.set_dataset_from_data(x, a.beta, "unsigned", scale=True, tom=True)
        assert eng.finite() == (True, True) and eng.symmetric()
        wall, ms, info = [], [], None
        for _ in range(2):
            t0 = time.perf_counter()
            raw = eng.hclust_average()
            wall.append(time.perf_counter() - t0)
            ms.append(eng.hclust_ms())
            info = eng.hclust_info()
        t0 = time.perf_counter()
        _merge, height, _order, repairs = N.hclustFinish(n, *raw[:3])
        finish_s = time.perf_counter() - t0
    rec["a"] = dict(n=n, hclust_ms=ms, wall_s=wall, searches=info["searches"], searches_per_node=info["searches"] / n,
                    launches=info["launches"], merges_per_launch=512, ms_per_launch=min(ms) / info["launches"],
                    scratch_bytes=info["scratch_bytes"], finish_host_s=finish_s, n_repairs=repairs,
                    top_height=float(height[-1]))

    # (b)
    from scipy.cluster.hierarchy import linkage
    from scipy.spatial.distance import squareform
    n = a.n_host
    names = [f"g{i}" for i in range(n)]
    x = module_data(n, s, 21, 20)
    with N.FromDataDataset(RMatrix(x, None, names), a.beta, tom=True) as ds:
        wall_dev = []
        for _ in range(2):
            t0 = time.perf_counter()
            tree = ds.hclust()
            wall_dev.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        _corr, net = ds.matrices()
        t1 = time.perf_counter()
        d = 1.0 - net.values
        np.fill_diagonal(d, 0.0)
        cond = squareform(d, checks=False)
        t2 = time.perf_counter()
        Z = linkage(cond, "average")
        t3 = time.perf_counter()
    got = cluster_keys(n, merge_rows(n, tree["merge"]), tree["height"])
    exp = cluster_keys(n, Z[:, :2], Z[:, 2])
    same = set(got) == set(exp)
    worst = max(abs(got[k] - exp[k]) / exp[k] for k in exp) if same else float("nan")
    bar = (n + 16) * 2.0 ** -52
    rec["b"] = dict(n=n, device_route_wall_s=wall_dev, host_route_wall_s=t3 - t0,
                    host_route_parts_s=dict(matrices=t1 - t0, dissimilarity=t2 - t1, scipy_linkage=t3 - t2),
                    host_threads=int(os.environ.get("OMP_NUM_THREADS", "0")) or os.cpu_count(),
                    speedup=(t3 - t0) / min(wall_dev), same_clusters=same, worst_relative_height_difference=worst,
                    relative_bar=bar, n_repairs=tree["n_repairs"])
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(rec, sort_keys=True))
    assert same, "the device tree and scipy's tree hold different clusters"
    assert worst <= bar, f"heights differ by {worst:.3e} relative, above {bar:.3e}"


if __name__ == "__main__":
    main()
