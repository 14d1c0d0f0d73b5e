"""The correlation types of the from-data set-up (NR_COR_SPEARMAN,
NR_COR_BICOR), in one process on one GPU:

  (a) at the metric's shape (20,000 genes x 500 samples, beta = 5, unsigned):
      for Pearson (the unchanged code path), Spearman and bicor, the wall time
      of the set-up from the raw host data, first and second call; the
      correlation / adjacency kernel's own time (nr_netbuild_ms), the
      transform step's (nr_cor_ms: HIP events on the context's stream), the
      host-to-device bytes and the scratch bytes of the call.
  (b) at 8,000 x 500: the same set-up against the only correct route without
      the option -- the transform and the correlation in numpy on the host's
      threads, the network from it, Engine.set_dataset with the host matrices
      -- with the wall time and the host-to-device bytes of each, and the
      largest difference between the two routes' corr.

No threshold is set on any time. Writes the record to --out (default
profiles/cor/record.json) and prints it as one JSON line. Run it as one command
under its own timeout.

    python tools/cor_record.py [--n 20000] [--n-host 8000] [--s 500] [--out PATH]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import netrep_amd as N  # noqa: E402

COR_TYPES = ("pearson", "spearman", "bicor")


def host_scale(x):
    return (x - x.mean(axis=0)) / x.std(axis=0, ddof=1)


def host_ranks(xs):
    """Average ranks per column: L + (E + 1) / 2 (include/netrep_gpu.h)."""
    s, n = xs.shape
    order = np.argsort(xs, axis=0, kind="stable")
    srt = np.take_along_axis(xs, order, axis=0)
    out = np.empty((s, n))
    pos = np.arange(1, s + 1, dtype=np.float64)
    for j in range(n):
        new = np.empty(s, bool)
        new[0] = True
        np.not_equal(srt[1:, j], srt[:-1, j], out=new[1:])
        start = np.flatnonzero(new)
        cnt = np.diff(np.append(start, s))
        out[order[:, j], j] = np.repeat((pos[start] + pos[start + cnt - 1]) / 2.0, cnt)
    return out


def host_median(v):
    s = v.shape[0]
    p = np.partition(v, [(s - 1) // 2, s // 2], axis=0)
    return 0.5 * ((p[(s - 1) // 2] + 0.0) + (p[s // 2] + 0.0))


def host_bicor_z(xs):
    """The definition (include/netrep_gpu.h, NR_COR_BICOR) in numpy, all columns at once."""
    s = xs.shape[0]
    med = host_median(xs)
    dx = xs - med
    mad = host_median(np.abs(dx))
    with np.errstate(invalid="ignore", divide="ignore"):
        u = dx / (9.0 * mad)
        h = 1.0 - u * u
        a = dx * np.where(np.abs(u) < 1.0, h * h, 0.0)
    fb = mad == 0.0
    if fb.any():
        a[:, fb] = xs[:, fb] - xs[:, fb].mean(axis=0)
    return a * np.sqrt(float(s - 1)) / np.sqrt((a * a).sum(axis=0))


def host_corr(x, cor_type):
    xs = host_scale(x)
    z = host_scale(host_ranks(xs)) if cor_type == "spearman" else host_bicor_z(xs)
    return xs, np.clip(z.T @ z / (x.shape[0] - 1), -1.0, 1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--n-host", type=int, default=8000)
    ap.add_argument("--s", type=int, default=500)
    ap.add_argument("--beta", type=float, default=5.0)
    ap.add_argument("--out", default=os.path.join("profiles", "cor", "record.json"))
    a = ap.parse_args()
    s = a.s
    rec = {"s": s, "beta": a.beta, "net_type": "unsigned", "lds_rows": N.Engine.COR_LDS_ROWS,
           "wave_rows": N.Engine.COR_WAVE_ROWS}
    eng = N.Engine(0)

    # (a)
    n = a.n
    x = np.asfortranarray(np.random.default_rng(20).normal(size=(s, n)))
    rec["a"] = {"n": n, "compare_pairs": float(n) * s * s}
    for ct in COR_TYPES:
        wall, nb_ms, cor_ms, h2d = [], [], [], []
        for _ in range(2):
            before = N.h2d_bytes()
            t0 = time.perf_counter()
            eng.set_dataset_from_data(x, a.beta, "unsigned", scale=True, cor_type=ct)
            wall.append(time.perf_counter() - t0)
            h2d.append(N.h2d_bytes() - before)
            nb_ms.append(eng.netbuild_ms())
            cor_ms.append(eng.cor_ms())
        assert eng.finite() == (True, True) and eng.symmetric()
        scratch = 0 if ct == "pearson" else 8 * s * (n + 2) + (8 * s * n if ct == "spearman" else 0)
        rec["a"][ct] = dict(setup_wall_s=wall, h2d_bytes=h2d, netbuild_ms=nb_ms, cor_ms=cor_ms, scratch_bytes=scratch)

    # (b)
    n = a.n_host
    x = np.asfortranarray(np.random.default_rng(21).normal(size=(s, n)))
    rec["b"] = {"n": n, "host_threads": int(os.environ.get("OMP_NUM_THREADS", "0")) or os.cpu_count()}
    for ct in COR_TYPES[1:]:
        wall_dev, h2d_dev = [], []
        for _ in range(2):
            before = N.h2d_bytes()
            t0 = time.perf_counter()
            eng.set_dataset_from_data(x, a.beta, "unsigned", scale=True, cor_type=ct)
            wall_dev.append(time.perf_counter() - t0)
            h2d_dev.append(N.h2d_bytes() - before)
        c_dev = eng.matrices()[0]
        cor_ms_b = eng.cor_ms()
        before = N.h2d_bytes()
        t0 = time.perf_counter()
        xs, c_host = host_corr(x, ct)
        t1 = time.perf_counter()
        w_host = np.abs(c_host) ** a.beta
        t2 = time.perf_counter()
        with N.Engine(0) as e2:
            e2.set_dataset(c_host, w_host, xs)
            t3 = time.perf_counter()
        rec["b"][ct] = dict(
            device_route_wall_s=wall_dev, device_route_h2d_bytes=h2d_dev, device_cor_ms=cor_ms_b,
            host_route_wall_s=t3 - t0,
            host_route_parts_s=dict(numpy_transform_and_corr=t1 - t0, numpy_network=t2 - t1, set_dataset=t3 - t2),
            host_route_h2d_bytes=N.h2d_bytes() - before, setup_speedup=(t3 - t0) / min(wall_dev),
            max_corr_difference=float(np.abs(c_dev - c_host).max()),
            corr_bar=(s + (16 if ct == "spearman" else 64)) * 2.0 ** -52)
    eng.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(rec, sort_keys=True))


if __name__ == "__main__":
    main()
