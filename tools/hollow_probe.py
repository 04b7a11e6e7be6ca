"""Measure layer_hollow against the route a caller had before it: layer_distance with the distance stack returned,
then the window over the layers in numpy.

Scene: config 4's tree, rect +-1, 2048 x 2048 pixels, the raster section's 64 planes, one sample per pixel,
threshold 1, pruning level 2, wall2 = hollow_wall2(8, 2) (reach 4), ends 3.
(a) layer_hollow: the wall time of the whole call without and with out (median and min-max of the calls after the
    warm-up calls) and the passes by HIP events (layer_hollow_kernel_ms: the median of the timed calls).
(b) The earlier route, same process: layer_distance with dist (wall time, and its passes by events), then the
    numpy combination core[l] = AND over j of dist[l + j] > wall2[|j|] with the ends; for the images also
    raster_layers with cov and out = where(core, 0, cov).  The two cores are compared.
Prints one JSON object; --out writes it to a file as well.

    python tools/hollow_probe.py [--size 2048] [--layers 64] [--calls 10] [--warmup 3] [--host-calls 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PASSES = ["raster", "ring_copy_columns", "rows", "window"]


def summary(ms):
    return {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms)), "runs": len(ms)}


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return summary(ms)


def passes(switch, fn, calls):
    switch(True)
    try:
        rows = []
        for _ in range(calls):
            fn()
            rows.append(switch(True))
    finally:
        switch(False)
    return [float(v) for v in np.median(np.array(rows), axis=0)]


def combine(dist, wall2, ends):
    """the window in numpy over a downloaded distance stack"""
    L = len(dist)
    reach = len(wall2) - 1
    core = np.empty(dist.shape, bool)
    for l in range(L):
        if (ends & 1 and l < reach) or (ends & 2 and l + reach >= L):
            core[l] = False
            continue
        c = dist[l] > wall2[0]
        for j in range(1, reach + 1):
            for m in (l - j, l + j):
                if 0 <= m < L:
                    c &= dist[m] > wall2[j]
        core[l] = c
    return core


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048, help="pixels per axis")
    ap.add_argument("--layers", type=int, default=64)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-calls", type=int, default=3, help="runs of the earlier route's download and numpy window")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    try:   # torch's HIP runtime first, as in bench.py
        import torch
        torch.cuda.is_available()
    except Exception:
        pass
    import implisolid_amd as I
    from implisolid_amd import scenes

    shape = scenes.config4()[0]
    rect = np.array([-1, 1, -1, 1], np.float32)
    W, L = a.size, a.layers
    z = (-1.0 + 2.0 * (np.arange(L) + 0.5) / L).astype(np.float32)
    wall2 = I.hollow_wall2(8, 2)
    ends = 3
    res = {"scene": "config4 tree", "width": W, "height": W, "layers": L, "supersample": 1, "threshold": 1, "level": 2,
           "wall2": wall2.tolist(), "ends": ends, "calls": a.calls, "warmup": a.warmup, "passes": PASSES}
    I.set_pruning(2)

    def hollow(want_out):
        return I.layer_hollow(shape, rect, W, W, z, wall2, 1, 1, ends, want_out=want_out, return_stats=True)

    r = {"without_out": timed(lambda: hollow(False), a.calls, a.warmup),
         "pass_ms_median": passes(I.layer_hollow_kernel_ms, lambda: hollow(False), a.calls),
         "with_out": timed(lambda: hollow(True), a.calls, 1),
         "pass_ms_median_with_out": passes(I.layer_hollow_kernel_ms, lambda: hollow(True), a.calls)}
    out, rec, stats = hollow(True)
    r.update(stats=stats, solid_voxels=stats[5], core_voxels=stats[6], bytes_down=int(16 * L), bytes_down_with_out=int(16 * L + W * W * L))
    r["window_ns_per_voxel"] = 1e6 * r["pass_ms_median"][3] / (W * W * L)
    res["layer_hollow"] = r
    print("layer_hollow", r, flush=True)

    e = {"layer_distance_with_dist": timed(lambda: I.layer_distance(shape, rect, W, W, z, 1, 1, 0), a.host_calls, 1),
         "layer_distance_pass_ms_median": passes(I.layer_distance_kernel_ms, lambda: I.layer_distance(shape, rect, W, W, z, 1, 1, 0, want_dist=False),
                                                 a.calls),
         "raster_with_cov": timed(lambda: I.raster_layers(shape, rect, W, W, z, 1), a.host_calls, 1)}
    dist = I.layer_distance(shape, rect, W, W, z, 1, 1, 0)[0]
    cov = I.raster_layers(shape, rect, W, W, z, 1)[0]
    w2 = [int(v) for v in wall2]
    e["numpy_window"] = timed(lambda: combine(dist, w2, ends), a.host_calls, 0)
    core = combine(dist, w2, ends)
    e["numpy_out"] = timed(lambda: np.where(core, np.uint8(0), cov), a.host_calls, 0)
    e["route_ms_without_out"] = e["layer_distance_with_dist"]["ms_median"] + e["numpy_window"]["ms_median"]
    e["route_ms_with_out"] = e["route_ms_without_out"] + e["raster_with_cov"]["ms_median"] + e["numpy_out"]["ms_median"]
    e["bytes_down"] = int(32 * L + 4 * W * W * L)
    e["same_core"] = bool(np.array_equal(core, (out == 0) & (cov > 0)) and core.sum(axis=(1, 2)).tolist() == rec["core"].tolist())
    res["earlier_route"] = e
    print("earlier route", e, flush=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
