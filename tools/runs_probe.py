"""Measure layer_runs against the route a caller had before it: raster_layers with the image returned, then
run-length encoding on the host.

Scene: config 4's tree, rect +-1, 2048 x 2048 pixels, the raster section's 64 planes; one sample per pixel at
thresholds 0 (grey) and 1, and 4 x 4 samples per pixel at threshold 0; at pruning levels 2 and 0.  Per
configuration: the wall time of the whole call (median and min-max of 20 calls after 5 warm-up calls), the
passes by HIP events (layer_runs_kernel_ms: the median of the timed calls), the runs per layer and the bytes
that cross the bus in each direction.  The earlier route: raster_layers' wall time with the image, measured
the same way in the same process, plus the host encoding of the returned stack by the restatement
(tests/np_runs.py encode, numpy), timed on the whole stack; its result must equal the query's.  Writes
profiles/r<next round>_runs_probe.json.

    python tools/runs_probe.py [--size 2048] [--layers 64] [--calls 20] [--warmup 5] [--host-calls 3]
"""
import argparse
import glob
import json
import os
import re
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def next_round():
    rounds = [int(m.group(1)) for f in glob.glob(os.path.join(ROOT, "profiles", "r*"))
              for m in [re.match(r"r(\d+)", os.path.basename(f))] if m]
    return max(rounds, default=0) + 1


def summary(ms):
    return {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms))}


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return summary(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048, help="pixels per axis")
    ap.add_argument("--layers", type=int, default=64)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-calls", type=int, default=3, help="host encodings of the whole stack per configuration")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    try:   # torch's HIP runtime first, as in bench.py
        import torch
        torch.cuda.is_available()
    except Exception:
        pass
    import implisolid_amd as I
    from implisolid_amd import scenes
    import np_runs

    shape = scenes.config4()[0]
    rect = np.array([-1, 1, -1, 1], np.float32)
    W, L = a.size, a.layers
    z = (-1.0 + 2.0 * (np.arange(L) + 0.5) / L).astype(np.float32)
    res = {"scene": "config4 tree", "width": W, "height": W, "layers": L, "calls": a.calls, "warmup": a.warmup,
           "passes": ["raster", "count_scan", "emit"]}
    for level in (2, 0):
        I.set_pruning(level)
        try:
            for s, threshold in ((1, 0), (1, 1), (4, 0)):
                r = timed(lambda: I.layer_runs(shape, rect, W, W, z, s, threshold), a.calls, a.warmup)
                I.layer_runs_kernel_ms(True)
                passes = []
                for _ in range(a.calls):
                    offs, start, value, sums, stats = I.layer_runs(shape, rect, W, W, z, s, threshold, return_stats=True)
                    passes.append(I.layer_runs_kernel_ms(True))
                I.layer_runs_kernel_ms(False)
                per = np.diff(offs)
                r["pass_ms_median"] = [float(v) for v in np.median(np.array(passes), axis=0)]
                r["run_passes_ms"] = float(sum(r["pass_ms_median"][1:]))
                r.update(stats=stats, runs=stats[5], runs_nonzero=stats[6], runs_per_layer_min=int(per.min()),
                         runs_per_layer_median=float(np.median(per)), runs_per_layer_max=int(per.max()),
                         bytes_down=int(5 * stats[5] + 4 * (L + 1) * stats[4] + 16 * stats[4] + 8 * L),
                         bytes_up=int(4 * (2 * W * s + L)))
                # the earlier route: the image comes down, the host encodes it
                rr = timed(lambda: I.raster_layers(shape, rect, W, W, z, s), a.calls, a.warmup)
                rr["bytes_down"] = int(W * W * L + 8 * L)
                cov, _ = I.raster_layers(shape, rect, W, W, z, s)
                enc = []
                for _ in range(a.host_calls):
                    t0 = time.perf_counter()
                    ho, hs, hv = np_runs.encode(cov, threshold)
                    enc.append((time.perf_counter() - t0) * 1e3)
                same = bool(np.array_equal(ho, offs) and np.array_equal(hs, start) and np.array_equal(hv, value))
                del cov
                r["earlier_route"] = {"raster_with_image": rr, "host_encode": summary(enc), "equal_runs": same,
                                      "ms_median": rr["ms_median"] + float(np.median(enc))}
                r["ratio_to_earlier_route"] = r["earlier_route"]["ms_median"] / r["ms_median"]
                res["runs_level_%d_s%d_threshold_%d" % (level, s, threshold)] = r
                print("runs level", level, "s", s, "threshold", threshold, r, flush=True)
        finally:
            I.set_pruning(2)
    out = a.out or os.path.join(ROOT, "profiles", "r%02d_runs_probe.json" % next_round())
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
