"""Measure layer_islands against the route a caller had before it: raster_layers with the image returned,
then connected-component labelling on the host.

Scene: config 4's tree, rect +-1, 2048 x 2048 pixels, the raster section's 64 planes, one sample per pixel,
threshold 1, at pruning levels 2 and 0 and both connectivities.  Per configuration: the wall time of the
whole call (median and min-max of 20 calls after 5 warm-up calls), the passes by HIP events
(islands_kernel_ms: the median of the timed calls), the component, island and solid-pixel counts and the
bytes that cross the bus in each direction.  The earlier route: raster_layers' wall time with the image,
measured the same way in the same process, plus the host labelling of the returned stack -- by the
restatement's algorithm (tests/np_islands.py, minimum-label propagation) on one layer, under a wall-clock
cap, scaled by the layer count (the whole stack would take the cap times the layers), and by
scipy.ndimage.label on the whole stack where scipy happens to be installed (optional).  Writes
profiles/r<next round>_islands_probe.json.

    python tools/islands_probe.py [--size 2048] [--layers 64] [--calls 20] [--warmup 5] [--host-cap 30]
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


def propagate(solid, connectivity, cap_s):
    """np_islands.labels' loop on one layer under a wall-clock cap: (seconds, rounds, converged)"""
    import np_islands
    H, W = solid.shape
    big = H * W
    lab = np.where(solid, np.arange(big, dtype=np.int64).reshape(H, W), big)
    st = np_islands.steps(connectivity)
    t0 = time.perf_counter()
    rounds = 0
    while True:
        p = np.pad(lab, 1, constant_values=big)
        m = lab
        for dy, dx in st:
            m = np.minimum(m, p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W])
        m = np.where(solid, m, big)
        rounds += 1
        done = np.array_equal(m, lab)
        lab = m
        if done or time.perf_counter() - t0 > cap_s:
            return time.perf_counter() - t0, rounds, bool(done)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048, help="pixels per axis")
    ap.add_argument("--layers", type=int, default=64)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--host-cap", type=float, default=30.0, help="seconds the restatement's loop may take on its one layer")
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
    res = {"scene": "config4 tree", "width": W, "height": W, "layers": L, "supersample": 1, "threshold": 1, "calls": a.calls,
           "warmup": a.warmup, "passes": ["raster", "tiles", "merge", "rows_scan", "records_tally"]}
    for level in (2, 0):
        I.set_pruning(level)
        try:
            for conn in (4, 8):
                r = timed(lambda: I.layer_islands(shape, rect, W, W, z, 1, 1, conn), a.calls, a.warmup)
                I.islands_kernel_ms(True)
                passes = []
                for _ in range(a.calls):
                    offs, comps, stats = I.layer_islands(shape, rect, W, W, z, 1, 1, conn, return_stats=True)
                    passes.append(I.islands_kernel_ms(True))
                I.islands_kernel_ms(False)
                r["pass_ms_median"] = [float(v) for v in np.median(np.array(passes), axis=0)]
                r["label_passes_ms"] = float(sum(r["pass_ms_median"][1:]))
                r["with_labels"] = timed(lambda: I.layer_islands(shape, rect, W, W, z, 1, 1, conn, want_labels=True), max(3, a.calls // 4), 1)
                r.update(stats=stats, components=stats[5], islands=stats[6], solid_pixels=stats[7],
                         bytes_down=int(32 * stats[5] + 4 * (L + 1) + 16 + 8), bytes_down_with_labels=int(32 * stats[5] + 4 * W * W * L),
                         bytes_up=int(4 * (2 * W + L)), largest_area=int(comps["area"].max()) if len(comps) else 0)
                res["islands_level_%d_conn_%d" % (level, conn)] = r
                print("islands level", level, "connectivity", conn, r, flush=True)
            r = timed(lambda: I.raster_layers(shape, rect, W, W, z, 1), a.calls, a.warmup)
            r["bytes_down"] = int(W * W * L + 8 * L)
            res["raster_with_image_level_%d" % level] = r
            print("raster_layers with the image, level", level, r, flush=True)
        finally:
            I.set_pruning(2)
    # host labelling of the image the earlier route returns
    cov, _ = I.raster_layers(shape, rect, W, W, z, 1)
    solid = cov >= 1
    mid = int(np.argmax(solid.reshape(L, -1).sum(axis=1)))
    for conn in (4, 8):
        sec, rounds, done = propagate(solid[mid], conn, a.host_cap)
        res["host_restatement_conn_%d" % conn] = {"layer": mid, "seconds_one_layer": sec, "rounds": rounds, "converged": done,
                                                 "seconds_all_layers_scaled": sec * L}
        print("host restatement, connectivity", conn, res["host_restatement_conn_%d" % conn], flush=True)
    try:
        from scipy import ndimage   # optional
        for conn in (4, 8):
            s = ndimage.generate_binary_structure(2, 1 if conn == 4 else 2)
            t0 = time.perf_counter()
            n = sum(ndimage.label(solid[l], structure=s)[1] for l in range(L))
            res["host_scipy_conn_%d" % conn] = {"seconds": time.perf_counter() - t0, "components": int(n)}
            print("scipy.ndimage.label, connectivity", conn, res["host_scipy_conn_%d" % conn], flush=True)
    except ImportError:
        res["host_scipy"] = "scipy is not installed"
    out = a.out or os.path.join(ROOT, "profiles", "r%02d_islands_probe.json" % next_round())
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
