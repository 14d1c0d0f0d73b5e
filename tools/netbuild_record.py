"""The from-data set-up at the metric's shape (20,000 genes x 500 samples,
beta = 5, unsigned) against the host-matrix set-up of the same dataset, in one
process on one GPU:

  * wall time of nr_set_dataset_from_data from the raw host data (upload of
    S x n doubles, scaling, the lower-triangle SYRK + epilogue, 16 n^2 bytes
    written), twice (the first call also pays one-off allocations);
  * wall time of nr_set_dataset from the equivalent host matrices (the export
    of the dataset just built) and the scaled data, twice;
  * the kernel's own time (HIP events on the context's stream) as a fraction
    of the fp64 matrix peak (78.6 TF) in S n (n + T) flops and of
    the HBM peak (8 TB/s) in 16 n^2 bytes written.

Writes the record to --out (default profiles/netbuild/record.json) and prints
it as one JSON line. Run it as one command under its own timeout; the engine's
staging copies use its default 8 host threads.

    python tools/netbuild_record.py [--n 20000] [--s 500] [--out PATH]
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
HBM_PEAK = 8.0e12            # bytes/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--s", type=int, default=500)
    ap.add_argument("--beta", type=float, default=5.0)
    ap.add_argument("--out", default=os.path.join("profiles", "netbuild", "record.json"))
    a = ap.parse_args()
    n, s, tile = a.n, a.s, N.Engine.NETBUILD_TILE
    x = np.asfortranarray(np.random.default_rng(20).normal(size=(s, n)))
    rec = {"n": n, "s": s, "beta": a.beta, "net_type": "unsigned", "tile": tile,
           "data_bytes": 8 * s * n, "matrix_bytes": 16 * n * n}
    eng = N.Engine(0)
    from_data, kernel_ms, h2d = [], [], []
    for _ in range(2):
        before = N.h2d_bytes()
        t = time.perf_counter()
        eng.set_dataset_from_data(x, a.beta, "unsigned", scale=True)
        from_data.append(time.perf_counter() - t)
        h2d.append(N.h2d_bytes() - before)
        kernel_ms.append(eng.netbuild_ms())
    assert eng.finite() == (True, True) and eng.symmetric()
    corr, net = eng.matrices()
    xs = eng.scale(x)
    host, h2d_host = [], []
    for _ in range(2):
        before = N.h2d_bytes()
        t = time.perf_counter()
        eng.set_dataset(corr, net, xs)
        host.append(time.perf_counter() - t)
        h2d_host.append(N.h2d_bytes() - before)
    assert eng.symmetric()
    eng.close()
    k = min(kernel_ms) * 1e-3
    flops = float(s) * n * (n + tile)   # n (n + T) / 2 elements of the lower triangle's tiles, 2 S flops each
    rec.update(
        from_data_wall_s=from_data, host_matrix_wall_s=host, from_data_h2d_bytes=h2d, host_matrix_h2d_bytes=h2d_host,
        setup_speedup=min(host) / min(from_data), kernel_ms=kernel_ms, kernel_flops=flops,
        kernel_fraction_of_fp64_matrix_peak=flops / k / FP64_MATRIX_PEAK,
        kernel_fraction_of_hbm_peak=16.0 * n * n / k / HBM_PEAK,
        flops_bound_ms=flops / FP64_MATRIX_PEAK * 1e3, write_bound_ms=16.0 * n * n / HBM_PEAK * 1e3)
    rec["bound_by"] = ("HBM write" if rec["write_bound_ms"] >= rec["flops_bound_ms"] else "fp64 matrix peak")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(rec, sort_keys=True))


if __name__ == "__main__":
    main()
