"""The discovery side from the data matrix alone, and one resident dataset in
two permutation calls, at the metric's shape (20,000 genes x 500 samples,
bench.py's 50 modules, beta = 5, unsigned), without and with the TOM, in one
process on one GPU:

  (a) discovery properties of pre-scaled data by the host-matrix route
      (BuildNetwork copies corr and net back, IntermediateProperties uploads
      them again) and by IntermediatePropertiesFromData: wall time of the
      first and the second call of each, and the host -> device bytes;
  (b) two permutation_procedure calls on one FromDataDataset against two
      PermutationProcedureFromData calls, at nPermutations = 0, so that the
      set-up is what is timed;
  (c) the outputs of the two routes of (a) and of (b) agree bit for bit
      (asserted), and so do the byte counts one can derive: the from-data
      route uploads the 8 S n bytes of data and the module metadata, the host
      route at least 16 n^2 + 8 S n, a second call on a handle no data.

Writes the record to --out (default profiles/discovery/record.json) and prints
it as one JSON line. Run it as one command under its own timeout.

    python tools/discovery_record.py [--n 20000] [--s 500] [--out PATH]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import netrep_amd as N  # noqa: E402
from netrep_amd import synthetic as S  # noqa: E402
from netrep_amd.api import RMatrix  # noqa: E402


def timed(fn):
    before = N.h2d_bytes()
    t = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t, N.h2d_bytes() - before


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def same_disc(a, b):
    return all(list(a[k]) == list(b[k]) and all(same_bits(a[k][m], b[k][m]) for m in a[k])
               for k in ("degree", "corr", "contribution"))


def one(tom, xs, names, ma, modules, beta):
    s, n = xs.values.shape
    data_bytes, matrix_bytes = 8 * s * n, 16 * n * n
    rec = {}

    def host_route():
        corr, net = N.BuildNetwork(xs, beta, scaleData=False, tom=tom)
        return N.IntermediateProperties(xs, corr, net, names, ma, modules)

    def data_route():
        return N.IntermediatePropertiesFromData(xs, beta, names, ma, modules, scaleData=False, tom=tom)

    for key, route in (("host_matrix_route", host_route), ("from_data_route", data_route)):
        N.ReleaseResident()
        runs = [timed(route) for _ in range(2)]
        rec[key] = {"wall_s": [r[1] for r in runs], "h2d_bytes": [r[2] for r in runs]}
        rec[key + "_out"] = runs[1][0]
    disc = rec.pop("from_data_route_out")
    assert same_disc(disc, rec.pop("host_matrix_route_out")), "discovery vectors differ between the routes"
    for b in rec["from_data_route"]["h2d_bytes"]:
        assert data_bytes <= b < data_bytes + (1 << 20), b
    # the first call; the second may find its matrices resident (the exported
    # arrays land at the same addresses with the same values) and then pays
    # the fingerprint pass over them instead of the upload
    assert rec["host_matrix_route"]["h2d_bytes"][0] >= matrix_bytes + data_bytes, rec["host_matrix_route"]
    rec["discovery_speedup"] = min(rec["host_matrix_route"]["wall_s"]) / min(rec["from_data_route"]["wall_s"])

    N.ReleaseResident()
    shots = [timed(lambda: N.PermutationProcedureFromData(disc, xs, beta, ma, modules, 0, scaleData=False, tom=tom))
             for _ in range(2)]
    N.ReleaseResident()
    ds, t_build, b_build = timed(lambda: N.FromDataDataset(xs, beta, scaleData=False, tom=tom))
    with ds:
        calls = [timed(lambda: ds.permutation_procedure(disc, ma, modules, 0)) for _ in range(2)]
    for r in shots + calls:
        assert same_bits(r[0]["observed"], shots[0][0]["observed"]), "observed statistics differ between the routes"
    assert data_bytes <= b_build < data_bytes + 16 * n, b_build
    assert calls[1][2] < data_bytes and calls[0][2] < data_bytes
    rec["one_shot_permutation_setup"] = {"wall_s": [r[1] for r in shots], "h2d_bytes": [r[2] for r in shots]}
    rec["handle_permutation_setup"] = {"build_wall_s": t_build, "build_h2d_bytes": b_build,
                                       "wall_s": [r[1] for r in calls], "h2d_bytes": [r[2] for r in calls]}
    rec["two_calls_speedup"] = sum(r[1] for r in shots) / (t_build + sum(r[1] for r in calls))
    rec["bitwise_agreement"] = True
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20000)
    ap.add_argument("--s", type=int, default=500)
    ap.add_argument("--beta", type=float, default=5.0)
    ap.add_argument("--out", default=os.path.join("profiles", "discovery", "record.json"))
    a = ap.parse_args()
    n, s = a.n, a.s
    sizes = S.CONFIGS["C3"][2] if n >= 20000 else np.round(np.linspace(30, 300, 50) * n / 20000).astype(int) + 2
    lay = S.make_layout(n, sizes, 20)
    raw = S._gen_numpy(lay, s, np.random.default_rng(21), set(lay.modules))
    names, ma, modules = list(lay.names), dict(zip(lay.names, lay.labels)), list(lay.modules)
    xs = N.Scale(RMatrix(np.asfortranarray(raw), None, names))
    rec = {"n": n, "s": s, "beta": a.beta, "net_type": "unsigned", "modules": len(modules),
           "module_sizes": [int(sizes.min()), int(sizes.max())], "data_bytes": 8 * s * n, "matrix_bytes": 16 * n * n}
    for tom in (False, True):
        rec["tom" if tom else "plain"] = one(tom, xs, names, ma, modules, a.beta)
    N.ReleaseResident()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(rec, sort_keys=True))


if __name__ == "__main__":
    main()
