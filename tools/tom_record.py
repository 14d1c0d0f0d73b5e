"""The topological-overlap option of the from-data set-up (NR_NET_TOM), in one
process on one GPU:

  (a) at the metric's shape (20,000 genes x 500 samples, beta = 5, unsigned,
      tom=True): wall time of the set-up from the raw host data, twice (the
      first call also pays one-off allocations); the correlation / adjacency
      kernel's own time (nr_netbuild_ms) and the TOM step's (nr_tom_ms:
      extract, degrees and the TOM kernel; HIP events on the context's
      stream), the latter as a fraction of the fp64 matrix peak (78.6 TF,
      DESIGN.md) in n^2 (n + T) flops; the scratch bytes of the call.
  (b) at 8,000 x 500: the same set-up against the only route to a TOM network
      without the option -- BuildNetwork for the adjacency, the TOM in numpy
      on the host's threads, Engine.set_dataset with the host matrices -- with
      the wall time and the host-to-device bytes of each, and the worst
      relative difference between the two TOMs.

Writes the record to --out (default profiles/tom/record.json) and prints it as
one JSON line. Run it as one command under its own timeout.

    python tools/tom_record.py [--n 20000] [--n-host 8000] [--s 500] [--out PATH]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import netrep_amd as N  # noqa: E402

FP64_MATRIX_PEAK = 78.6e12   # flop/s


def host_tom(a):
    """The definition (include/netrep_gpu.h, NR_NET_TOM) in numpy."""
    a = np.array(a, dtype=np.float64, order="F")
    np.fill_diagonal(a, 0.0)
    k = a.sum(axis=0)
    t = a @ a
    t += a
    t /= np.minimum(k[:, None], k[None, :]) + 1.0 - a
    np.fill_diagonal(t, 1.0)
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--n-host", type=int, default=8000)
    ap.add_argument("--s", type=int, default=500)
    ap.add_argument("--beta", type=float, default=5.0)
    ap.add_argument("--out", default=os.path.join("profiles", "tom", "record.json"))
    a = ap.parse_args()
    s, tile = a.s, N.Engine.NETBUILD_TILE
    rec = {"s": s, "beta": a.beta, "net_type": "unsigned", "tile": tile}
    eng = N.Engine(0)

    # (a)
    n = a.n
    x = np.asfortranarray(np.random.default_rng(20).normal(size=(s, n)))
    wall, nb_ms, tom_ms, h2d = [], [], [], []
    for _ in range(2):
        before = N.h2d_bytes()
        t0 = time.perf_counter()
        eng.set_dataset_from_data(x, a.beta, "unsigned", scale=True, tom=True)
        wall.append(time.perf_counter() - t0)
        h2d.append(N.h2d_bytes() - before)
        nb_ms.append(eng.netbuild_ms())
        tom_ms.append(eng.tom_ms())
    assert eng.finite() == (True, True) and eng.symmetric()
    wall_plain = []
    for _ in range(3):
        t0 = time.perf_counter()
        eng.set_dataset_from_data(x, a.beta, "unsigned", scale=True)
        wall_plain.append(time.perf_counter() - t0)
    assert eng.tom_ms() == 0.0
    flops = float(n) * n * (n + tile)   # n (n + T) / 2 elements of the lower triangle's tiles, 2 n flops each
    rec["a"] = dict(
        n=n, setup_wall_s=wall, setup_wall_without_tom_s=wall_plain, h2d_bytes=h2d, netbuild_ms=nb_ms,
        tom_ms=tom_ms, tom_flops=flops, tom_fraction_of_fp64_matrix_peak=flops / (min(tom_ms) * 1e-3) / FP64_MATRIX_PEAK,
        tom_flops_bound_ms=flops / FP64_MATRIX_PEAK * 1e3, scratch_bytes=8 * n * (n + 2) + 8 * n)

    # (b)
    n = a.n_host
    x = np.asfortranarray(np.random.default_rng(21).normal(size=(s, n)))
    wall_dev, h2d_dev = [], []
    for _ in range(2):
        before = N.h2d_bytes()
        t0 = time.perf_counter()
        eng.set_dataset_from_data(x, a.beta, "unsigned", scale=True, tom=True)
        wall_dev.append(time.perf_counter() - t0)
        h2d_dev.append(N.h2d_bytes() - before)
    t_dev = eng.matrices()[1]
    tom_ms_b = eng.tom_ms()
    eng.close()
    before = N.h2d_bytes()
    t0 = time.perf_counter()
    corr, adj = N.BuildNetwork(x, a.beta, "unsigned", scaleData=True)
    t1 = time.perf_counter()
    t_host = host_tom(adj.values)
    t2 = time.perf_counter()
    with N.Engine(0) as e2:
        xs = e2.scale(x)
        t3 = time.perf_counter()
        e2.set_dataset(corr.values, t_host, xs)
        t4 = time.perf_counter()
    h2d_host = N.h2d_bytes() - before
    rel = np.abs(t_dev - t_host) / np.maximum(np.abs(t_host), np.finfo(float).tiny)
    rec["b"] = dict(
        n=n, device_route_wall_s=wall_dev, device_route_h2d_bytes=h2d_dev, device_tom_ms=tom_ms_b,
        host_route_wall_s=t4 - t0, host_route_parts_s=dict(build_network=t1 - t0, numpy_tom=t2 - t1, scale=t3 - t2,
                                                           set_dataset=t4 - t3),
        host_route_h2d_bytes=h2d_host, host_threads=int(os.environ.get("OMP_NUM_THREADS", "0")) or os.cpu_count(),
        setup_speedup=(t4 - t0) / min(wall_dev), worst_relative_difference=float(rel.max()),
        relative_bar=(n + 16) * 2.0 ** -52)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(rec, sort_keys=True))


if __name__ == "__main__":
    main()
