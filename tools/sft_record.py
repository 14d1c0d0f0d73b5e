"""The soft-threshold pick from the data matrix alone (nr_soft_connectivity,
netrep_PickSoftThreshold), in one process on one GPU:

  (a) at the metric's shape (20,000 genes x 500 samples, unsigned): the
      connectivities of pickSoftThreshold's 15 default powers (the integer
      chain) and of 15 non-integer powers (one pow each), three calls each:
      wall time of Engine.soft_connectivity from the raw host data, the two
      kernels' own time (nr_sft_ms, HIP events), the host-to-device bytes,
      the kernels' time as a fraction of the fp64 matrix peak (78.6 TF,
      DESIGN.md) in 2 S n (n + T) flops per sweep of the full matrix, and the
      scratch bytes of the call; then PickSoftThreshold's wall time (the
      fits on the host included) and its answer.
  (b) at 8,000 x 500: PickSoftThreshold against the route without it --
      BuildNetwork for the host correlation matrix, then one numpy sweep of
      it per power on the host's threads and the same fits -- with the wall
      time and host-to-device bytes of each, and the worst relative
      difference between the two sets of connectivities.

Writes the record to --out (default profiles/sft/record.json) and prints it as
one JSON line. Run it as one command under its own timeout.

    python tools/sft_record.py [--n 20000] [--n-host 8000] [--s 500] [--out PATH]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import netrep_amd as N  # noqa: E402
from netrep_amd.api import DEFAULT_POWERS  # noqa: E402

FP64_MATRIX_PEAK = 78.6e12   # flop/s
POW_SLOTS = 8                # distinct non-integer powers per sweep (kSftPowSlots, csrc/netbuild.hip)
CHAIN_SLOTS = 16             # distinct integer powers per sweep (kSftChainSlots)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--n-host", type=int, default=8000)
    ap.add_argument("--s", type=int, default=500)
    ap.add_argument("--out", default=os.path.join("profiles", "sft", "record.json"))
    a = ap.parse_args()
    s, tile = a.s, N.Engine.NETBUILD_TILE
    chain = [float(p) for p in DEFAULT_POWERS]
    frac = [p + 0.5 for p in chain]
    rec = {"s": s, "net_type": "unsigned", "tile": tile, "powers_chain": chain, "powers_pow": frac}

    # (a)
    n = a.n
    x = np.asfortranarray(np.random.default_rng(20).normal(size=(s, n)))
    n_tiles = -(-n // tile)
    row_groups = min(-(-n_tiles // 16), 32)
    rec["a"] = {"n": n, "row_groups": row_groups,
                "scratch_bytes": 8 * row_groups * len(chain) * n + 8 * len(chain) * n}
    with N.Engine(0) as eng:
        for name, powers, per_sweep in (("chain", chain, CHAIN_SLOTS), ("pow", frac, POW_SLOTS)):
            wall, ms, h2d = [], [], []
            for _ in range(3):
                before = N.h2d_bytes()
                t0 = time.perf_counter()
                k = eng.soft_connectivity(x, powers, "unsigned", scale=True)
                wall.append(time.perf_counter() - t0)
                h2d.append(N.h2d_bytes() - before)
                ms.append(eng.sft_ms())
            assert np.isfinite(k).all()
            sweeps = -(-len(set(powers)) // per_sweep)
            flops = sweeps * 2.0 * s * n * (n_tiles * tile)   # every tile of the full matrix, 2 S flops per element
            rec["a"][name] = dict(wall_s=wall, sft_ms=ms, h2d_bytes=h2d, sweeps=sweeps, syrk_flops=flops,
                                  syrk_flops_bound_ms=flops / FP64_MATRIX_PEAK * 1e3,
                                  fraction_of_fp64_matrix_peak=flops / (min(ms) * 1e-3) / FP64_MATRIX_PEAK)
    t0 = time.perf_counter()
    got = N.PickSoftThreshold(x)
    rec["a"]["pick_wall_s"] = time.perf_counter() - t0
    rec["a"]["power_estimate"] = got["powerEstimate"]
    rec["a"]["sft_r_sq"] = got["fitIndices"]["SFT.R.sq"].tolist()

    # (b)
    n = a.n_host
    x = np.asfortranarray(np.random.default_rng(21).normal(size=(s, n)))
    wall_dev, h2d_dev = [], []
    for _ in range(2):
        before = N.h2d_bytes()
        t0 = time.perf_counter()
        dev = N.PickSoftThreshold(x, returnConnectivity=True)
        wall_dev.append(time.perf_counter() - t0)
        h2d_dev.append(N.h2d_bytes() - before)
    before = N.h2d_bytes()
    t0 = time.perf_counter()
    corr, _net = N.BuildNetwork(x, 1.0, "unsigned", scaleData=True)
    t1 = time.perf_counter()
    b = np.abs(corr.values)
    np.fill_diagonal(b, 0.0)
    k_host = np.empty((n, len(chain)), order="F")
    for m, p in enumerate(chain):
        k_host[:, m] = (b ** p).sum(axis=0)
    t2 = time.perf_counter()
    fits = [N.ScaleFreeFit(k_host[:, m]) for m in range(len(chain))]
    t3 = time.perf_counter()
    h2d_host = N.h2d_bytes() - before
    rel = np.abs(dev["connectivity"] - k_host) / np.maximum(np.abs(k_host), np.finfo(float).tiny)
    rec["b"] = dict(
        n=n, device_route_wall_s=wall_dev, device_route_h2d_bytes=h2d_dev, host_route_wall_s=t3 - t0,
        host_route_parts_s=dict(build_network=t1 - t0, numpy_sweeps=t2 - t1, fits=t3 - t2),
        host_route_h2d_bytes=h2d_host, host_route_matrix_bytes=8 * n * n,
        host_threads=int(os.environ.get("OMP_NUM_THREADS", "0")) or os.cpu_count(),
        speedup=(t3 - t0) / min(wall_dev), worst_relative_difference=float(rel.max()),
        relative_bar=(n + 2 * max(chain) + 16) * 2.0 ** -52,
        sft_r_sq_worst_difference=float(np.abs(dev["fitIndices"]["SFT.R.sq"]
                                               - np.array([f["Rsquared.SFT"] for f in fits])).max()))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(rec, sort_keys=True))


if __name__ == "__main__":
    main()
