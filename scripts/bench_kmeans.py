"""The room level's KMeans both ways on the same inputs: hmsg_kmeans per set on 16 host threads (what the graph object does by
default) against one hmsg_kmeans_batch call on the device (hmsg_graph_params::kmeans_device).
    python scripts/bench_kmeans.py [--out profiles/kmeans_device.json] [--commit HASH]
Inputs: 8 sets of 3000 x 512 (unit rows around a few directions, case (b) of tests/test_kmeans_device.py), k = 24, n_init = 5,
max_iter = 100; and 1 set of 333 x 512.  The first thing it does is check that both paths return equal bits.  Then the median wall
time of 5 calls after one warm-up, each way.  The result (and the commit / source hash it was taken on) goes to --out and, as one
JSON line, to stdout."""
import argparse
import json
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import torch  # noqa: E402,F401  (before the library, as tests/conftest.py does)

from holoagent_amd._lib import HmsgLib, kmeans, kmeans_batch  # noqa: E402
from scripts.csrc_sha import csrc_sha16  # noqa: E402

K, N_INIT, MAX_ITER, THREADS = 24, 5, 100, 16


def make(n, D, seed):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((7, D))
    X = c[rng.integers(0, 7, n)] + 0.3 * rng.standard_normal((n, D))
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    return np.ascontiguousarray(X, np.float32)


def host_path(L, sets, pool):
    # (ctypes releases the GIL for the duration of the call: the fits run side by side, one per thread)
    return list(pool.map(lambda X: kmeans(X, K, N_INIT, MAX_ITER, 0, lib_=L), sets))


def device_path(L, sets):
    return kmeans_batch(sets, K, N_INIT, MAX_ITER, 0, lib_=L)


def median_ms(fn, repeat=5):
    fn()                                                   # warm-up
    t = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), [round(v, 3) for v in t]


def commit_hash():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True, check=True).stdout.strip()
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans_device.json"))
    ap.add_argument("--commit", default=None, help="the commit the tree was taken from (a tree without .git cannot tell)")
    a = ap.parse_args()
    L = HmsgLib()
    res = {"metric": "kmeans_device_vs_host", "commit": a.commit or commit_hash(), "csrc_sha16": csrc_sha16(), "k": K, "n_init": N_INIT,
           "max_iter": MAX_ITER, "host_threads": THREADS, "device": torch.cuda.get_device_name(0), "cases": []}
    with ThreadPoolExecutor(THREADS) as pool:
        for name, sets in (("8 x 3000 x 512", [make(3000, 512, 500 + i) for i in range(8)]), ("1 x 333 x 512", [make(333, 512, 600)])):
            h, d = host_path(L, sets, pool), device_path(L, sets)
            for a_, b_ in zip(h, d):                       # equal bits first: a timing of two different computations says nothing
                assert np.array_equal(a_[0], b_[0]) and np.array_equal(a_[1].view(np.uint32), b_[1].view(np.uint32))
                assert np.float32(a_[2]).view(np.uint32) == np.float32(b_[2]).view(np.uint32) and a_[3] == b_[3]
            host_ms, host_all = median_ms(lambda: host_path(L, sets, pool))
            dev_ms, dev_all = median_ms(lambda: device_path(L, sets))
            res["cases"].append({"sets": name, "equal_bits": True, "n_iter": [int(f[3]) for f in h], "host_ms": round(host_ms, 3),
                                 "device_ms": round(dev_ms, 3), "host_over_device": round(host_ms / dev_ms, 3), "host_ms_all": host_all,
                                 "device_ms_all": dev_all})
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
