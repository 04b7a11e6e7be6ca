"""Measure layer_cups against layer_bodies of the empty class on the same stack.

Scene: config 4's tree, rect +-1, 2048 x 2048 pixels, the raster section's 64 planes, one sample per pixel, threshold
1, pruning level 2: the stack of DESIGN.md's figures for layer_bodies.
(a) layer_cups, connectivity 6: the wall time of the whole call (median and min-max of the calls after the warm-up
    calls), without and with the cupped runs, and the four passes by HIP events (layer_cups_kernel_ms: the median of
    the timed calls): raster, count + scan + emit + frame, the layers' link + mark + head, finish.  The empty row
    runs, the cups, the cupped voxels and the bytes that come down.
(b) layer_bodies(target=0, connectivity=6) on the same stack, measured the same way: the same count, emit and link
    without the per-layer queries.  --bodies-only measures nothing else, for a run against another build of the
    library (IMPLISOLID_LIB), the parent commit's for instance.
Prints one JSON object; --out writes it to a file as well.

    python tools/cups_probe.py [--size 2048] [--layers 64] [--calls 9] [--warmup 3] [--bodies-only] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CUP_PASSES = ["raster", "count_scan_emit_frame", "link_mark_head", "finish"]
BODY_PASSES = ["raster", "count_scan_emit", "link", "finish"]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048, help="pixels per axis")
    ap.add_argument("--layers", type=int, default=64)
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bodies-only", action="store_true", help="measure layer_bodies alone")
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
    res = {"scene": "config4 tree", "width": W, "height": W, "layers": L, "supersample": 1, "threshold": 1, "level": 2,
           "connectivity": 6, "calls": a.calls, "warmup": a.warmup, "library": I.LIB_PATH}
    I.set_pruning(2)

    def bodies():
        return I.layer_bodies(shape, rect, W, W, z, 1, 1, 0, 6, return_stats=True)

    b = dict(timed(bodies, a.calls, a.warmup), passes=BODY_PASSES, pass_ms_median=passes(I.layer_bodies_kernel_ms, bodies, a.calls))
    stats = bodies()[2]
    b.update(stats=stats, row_runs=stats[5], bodies=stats[6], bytes_down=int(64 * stats[6] + 8 * (L + 1) + 16))
    res["layer_bodies_target_0"] = b
    print("layer_bodies target 0", b, flush=True)

    if not a.bodies_only:
        def cups():
            return I.layer_cups(shape, rect, W, W, z, 1, 1, 6, return_stats=True)

        def cups_runs():
            return I.layer_cups(shape, rect, W, W, z, 1, 1, 6, want_runs=True, return_stats=True)

        c = dict(timed(cups, a.calls, a.warmup), passes=CUP_PASSES, pass_ms_median=passes(I.layer_cups_kernel_ms, cups, a.calls))
        offs, recs, roffs, runs, stats = cups_runs()
        c.update(stats=stats, row_runs=stats[5], cups=stats[6], cupped_voxels=stats[7], cupped_runs=int(len(runs)),
                 layers_with_cups=int((np.diff(offs) > 0).sum()), device_bytes_runs=int(24 * stats[5]),
                 bytes_down=int(56 * stats[6] + 2 * 4 * (L + 1) + 4 * (L + 1) * stats[4] + 16 * stats[4] + 8))
        c["with_runs"] = dict(timed(cups_runs, a.calls, a.warmup), bytes_down=c["bytes_down"] + int(12 * len(runs)))
        ms = c["pass_ms_median"]
        c["share_of_passes"] = {name: v / sum(ms) for name, v in zip(CUP_PASSES, ms)}
        c["ratio_to_layer_bodies"] = c["ms_median"] / b["ms_median"]
        res["layer_cups"] = c
        print("layer_cups", c, flush=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
