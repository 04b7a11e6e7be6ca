"""Measure layer_supports against the route a caller had before it: layer_distance with the distance stack returned,
overhang_mask, then the cells' tips and feet in numpy.

Scene: config 4's tree, rect +-1, 2048 x 2048 pixels, the raster section's 64 planes, one sample per pixel,
threshold 1, pruning level 2, reach2 0; per cell side given with --cells (default 32 and 1).
(a) layer_supports: the wall time of the whole call (median and min-max of the calls after the warm-up calls) and
    the passes by HIP events (layer_supports_kernel_ms: the median of the timed calls).
(b) layer_distance(want_dist=False) on the same scene, wall time and passes: what the distance passes alone cost.
(c) The earlier route, same process: layer_distance with dist (wall time), overhang_mask, then per layer a loop over
    the non-empty cells in numpy (for a cell of one pixel the unsupported pixels are the tips and no loop is
    needed) and the feet from a running array of the highest solid layer.  The two results are compared.
Prints one JSON object; --out writes it to a file as well.

    python tools/supports_probe.py [--size 2048] [--layers 64] [--cells 32 1] [--calls 10] [--warmup 3] [--host-calls 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PASSES = ["raster", "columns_rows", "cells", "count_scan_emit_top"]


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


def host_tips(dist, mask, cell):
    """the tips {p, depth, foot, load} and their offsets from a downloaded distance stack and its overhang mask"""
    L, H, W = dist.shape
    ncx = -(-W // cell)
    top = np.full((H, W), -1, np.int32)   # the highest solid layer below the layer at hand
    rows, offs = [], [0]
    for l in range(L):
        ys, xs = np.nonzero(mask[l])
        n = 0
        if len(ys):
            p = ys.astype(np.int64) * W + xs
            depth = dist[l, ys, xs]
            if cell == 1:
                rows.append(np.stack([p, depth, top[ys, xs], np.ones(len(p), np.int64)], axis=1))
                n = len(p)
            else:
                c = (ys // cell) * ncx + xs // cell
                order = np.argsort(c, kind="stable")   # p stays increasing within a cell
                cs, first = np.unique(c[order], return_index=True)
                ends = np.append(first[1:], len(order))
                out = np.empty((len(cs), 4), np.int64)
                for k in range(len(cs)):   # the cell loop
                    idx = order[first[k]:ends[k]]
                    best = idx[np.argmax(depth[idx])]   # the first of the largest: the smallest p
                    out[k] = (p[best], depth[best], top[ys[best], xs[best]], len(idx))
                rows.append(out)
                n = len(cs)
        offs.append(offs[-1] + n)
        top[dist[l] > 0] = l
    return (np.concatenate(rows) if rows else np.zeros((0, 4), np.int64)), np.array(offs, np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2048, help="pixels per axis")
    ap.add_argument("--layers", type=int, default=64)
    ap.add_argument("--cells", type=int, nargs="+", default=[32, 1])
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-calls", type=int, default=2, help="runs of the earlier route's download and numpy steps")
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
    res = {"scene": "config4 tree", "width": W, "height": W, "layers": L, "supersample": 1, "threshold": 1, "level": 2, "reach2": 0,
           "calls": a.calls, "warmup": a.warmup, "passes": PASSES}
    I.set_pruning(2)

    def nodist():
        return I.layer_distance(shape, rect, W, W, z, 1, 1, 0, want_dist=False)

    res["layer_distance_without_dist"] = dict(timed(nodist, a.calls, a.warmup),
                                              pass_ms_median=passes(I.layer_distance_kernel_ms, nodist, a.calls))
    print("layer_distance without dist", res["layer_distance_without_dist"], flush=True)

    got = {}
    for cell in a.cells:
        def supports():
            return I.layer_supports(shape, rect, W, W, z, cell, 1, 1, 0, return_stats=True)

        r = dict(timed(supports, a.calls, a.warmup), pass_ms_median=passes(I.layer_supports_kernel_ms, supports, a.calls))
        got[cell] = supports()
        stats = got[cell][3]
        r.update(stats=stats, unsupported=stats[5], tips=stats[6], tips_on_the_plate=stats[7], bytes_down=int(16 * stats[6] + 24 * L + 8))
        res["layer_supports_cell_%d" % cell] = r
        print("layer_supports cell", cell, r, flush=True)

    e = {"layer_distance_with_dist": timed(lambda: I.layer_distance(shape, rect, W, W, z, 1, 1, 0), a.host_calls, 1)}
    dist = I.layer_distance(shape, rect, W, W, z, 1, 1, 0)[0]
    e["overhang_mask"] = timed(lambda: I.overhang_mask(dist, 0), a.host_calls, 0)
    mask = I.overhang_mask(dist, 0)
    e["bytes_down"] = int(32 * L + 4 * W * W * L)
    for cell in a.cells:
        e["numpy_tips_cell_%d" % cell] = timed(lambda: host_tips(dist, mask, cell), a.host_calls, 0)
        e["route_ms_cell_%d" % cell] = (e["layer_distance_with_dist"]["ms_median"] + e["overhang_mask"]["ms_median"] +
                                        e["numpy_tips_cell_%d" % cell]["ms_median"])
        rows, offs = host_tips(dist, mask, cell)
        tips = got[cell][0]
        mine = np.stack([tips[n] for n in tips.dtype.names], axis=1).astype(np.int64)
        e["same_tips_cell_%d" % cell] = bool(np.array_equal(rows, mine) and np.array_equal(offs, got[cell][1]))
    res["earlier_route"] = e
    print("earlier route", e, flush=True)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
