"""Measure layer_distance against the route a caller had before it: raster_layers with the image returned,
then an exact Euclidean distance transform on the host.

(a) Scene: config 4's tree, rect +-1, 2048 x 2048 pixels, the raster section's 64 planes, one sample per
    pixel, threshold 1, reach2 4, at pruning levels 2 and 0.  Per level: the wall time of the whole call
    without and with the distance stack returned (median and min-max of the calls after the warm-up calls),
    the passes by HIP events (layer_distance_kernel_ms: the median of the timed calls) and the bytes that
    cross the bus.
(b) The worst case of the row pass's outward search: one painted layer of 512 x 512 pixels, solid but for
    one pixel, timed the same way; and the nanoseconds per pixel of the column and row passes of (a) and (b).
(c) The earlier route: raster_layers' wall time with the image, measured the same way in the same process,
    plus the host transform of the returned stack: scipy.ndimage.distance_transform_edt of both classes on
    --host-layers layers, scaled by the layer count, where scipy is installed; otherwise the blocked brute
    force of tests/np_distance.py on a 128 x 128 corner of one layer, which is said in the result.
Writes profiles/r<next round>_distance_probe.json.

    python tools/distance_probe.py [--size 2048] [--layers 64] [--calls 20] [--warmup 5] [--host-layers 8]
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

PASSES = ["raster", "columns", "rows_records"]


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


def passes(I, fn, calls):
    I.layer_distance_kernel_ms(True)
    try:
        rows = []
        for _ in range(calls):
            fn()
            rows.append(I.layer_distance_kernel_ms(True))
    finally:
        I.layer_distance_kernel_ms(False)
    return [float(v) for v in np.median(np.array(rows), axis=0)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048, help="pixels per axis")
    ap.add_argument("--layers", type=int, default=64)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-layers", type=int, default=8, help="layers the host transform is timed on")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    try:   # torch's HIP runtime first, as in bench.py
        import torch
        torch.cuda.is_available()
    except Exception:
        pass
    import implisolid_amd as I
    from implisolid_amd import scenes
    import island_inputs as ii

    shape = scenes.config4()[0]
    rect = np.array([-1, 1, -1, 1], np.float32)
    W, L = a.size, a.layers
    few = max(3, a.calls // 4)
    z = (-1.0 + 2.0 * (np.arange(L) + 0.5) / L).astype(np.float32)
    res = {"scene": "config4 tree", "width": W, "height": W, "layers": L, "supersample": 1, "threshold": 1, "reach2": 4,
           "calls": a.calls, "warmup": a.warmup, "passes": PASSES}
    # (a) and the raster half of (c)
    for level in (2, 0):
        I.set_pruning(level)
        try:
            r = timed(lambda: I.layer_distance(shape, rect, W, W, z, 1, 1, 4, want_dist=False), a.calls, a.warmup)
            r["pass_ms_median"] = passes(I, lambda: I.layer_distance(shape, rect, W, W, z, 1, 1, 4, want_dist=False), a.calls)
            r["distance_passes_ms"] = float(sum(r["pass_ms_median"][1:]))
            r["ns_per_pixel"] = [1e6 * v / (W * W * L) for v in r["pass_ms_median"][1:]]
            r["with_dist"] = timed(lambda: I.layer_distance(shape, rect, W, W, z, 1, 1, 4), few, 1)
            _, rec, stats = I.layer_distance(shape, rect, W, W, z, 1, 1, 4, want_dist=False, return_stats=True)
            r.update(stats=stats, solid_pixels=stats[5], unsupported_pixels=stats[6], widest=int(rec["widest"].max()),
                     bytes_down=int(32 * L + 16), bytes_down_with_dist=int(32 * L + 4 * W * W * L), bytes_up=int(4 * (2 * W + L)))
            res["distance_level_%d" % level] = r
            print("layer_distance level", level, r, flush=True)
            r = timed(lambda: I.raster_layers(shape, rect, W, W, z, 1), a.calls, a.warmup)
            r["bytes_down"] = int(W * W * L + 8 * L)
            res["raster_with_image_level_%d" % level] = r
            print("raster_layers with the image, level", level, r, flush=True)
        finally:
            I.set_pruning(2)
    # (b) the longest searches: every pixel of 512 x 512 walks to the one hole
    S = 512
    bits = np.ones((1, S, S), bool)
    bits[0, S // 2 + 3, S // 2 - 5] = False
    node, prect, pz = ii.painted(bits)
    r = timed(lambda: I.layer_distance(node, prect, S, S, pz, want_dist=False), a.calls, a.warmup)
    r["pass_ms_median"] = passes(I, lambda: I.layer_distance(node, prect, S, S, pz, want_dist=False), a.calls)
    r["ns_per_pixel"] = [1e6 * v / (S * S) for v in r["pass_ms_median"][1:]]
    dist, rec = I.layer_distance(node, prect, S, S, pz)
    y, x = np.mgrid[0:S, 0:S]
    want = (x - (S // 2 - 5)) ** 2 + (y - (S // 2 + 3)) ** 2
    want[S // 2 + 3, S // 2 - 5] = -1
    r.update(exact=bool(np.array_equal(dist[0], want)), widest=int(rec["widest"][0]))
    res["one_hole_512"] = r
    print("one hole in 512 x 512", r, flush=True)
    # (c) the host transform of the image the earlier route returns
    cov, _ = I.raster_layers(shape, rect, W, W, z, 1)
    solid = cov >= 1
    busy = np.argsort(-solid.reshape(L, -1).sum(axis=1))[:max(1, min(a.host_layers, L))]
    try:
        from scipy import ndimage   # optional
        t0 = time.perf_counter()
        for l in busy:
            ndimage.distance_transform_edt(solid[l])
            ndimage.distance_transform_edt(~solid[l])
        sec = time.perf_counter() - t0
        res["host_scipy_edt"] = {"layers_timed": len(busy), "seconds": sec, "seconds_all_layers_scaled": sec * L / len(busy),
                                 "note": "float64 distances of both classes, the busiest layers; the squared integers would still need rounding"}
    except ImportError:
        import np_distance
        l, c = int(busy[0]), 128
        my, mx = (int(v) for v in np.argwhere(solid[l])[len(np.argwhere(solid[l])) // 2]) if solid[l].any() else (0, 0)
        y0, x0 = min(max(my - c // 2, 0), W - c), min(max(mx - c // 2, 0), W - c)
        t0 = time.perf_counter()
        np_distance.layer_d2(solid[l, y0:y0 + c, x0:x0 + c])
        sec = time.perf_counter() - t0
        res["host_brute_force"] = {"layer": l, "corner": c, "seconds": sec,
                                   "note": "scipy is not installed: tests/np_distance.py on a %d x %d window of one layer only" % (c, c)}
    print("host transform", {k: v for k, v in res.items() if k.startswith("host_")}, flush=True)
    out = a.out or os.path.join(ROOT, "profiles", "r%02d_distance_probe.json" % next_round())
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
