"""Measure raster_layers against the route the library offered before it: every sample of every layer
through ImplicitService.eval, in calls of a few planes each (the numpy count that would follow is not
timed, nor is building the point arrays).

Scene: config 4's tree, rect +-1, 2048 x 2048 pixels, 64 planes evenly spaced inside z in (-1, 1), at
1 and 2 sub-samples per axis.  Wall clock around each call (the image is host resident when it
returns): median and min-max of 20 calls after 5 warm-up calls, at pruning levels 2 and 0, with the
call's stats (tiles evaluated, tiles filled, samples evaluated).  Writes
profiles/r<next round>_raster_measure.json.

    python tools/raster_measure.py [--size 2048] [--layers 64] [--calls 20] [--warmup 5]
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
    ap.add_argument("--supersample", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--batch-samples", type=int, default=1 << 24, help="samples per ImplicitService.eval call, in whole planes")
    ap.add_argument("--no-route", action="store_true", help="skip the ImplicitService.eval route")
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
    res = {"scene": "config4 tree", "width": W, "height": W, "layers": L, "calls": a.calls, "warmup": a.warmup}
    for s in a.supersample:
        for level in (2, 0):
            I.set_pruning(level)
            try:
                r = timed(lambda: I.raster_layers(shape, rect, W, W, z, s), a.calls, a.warmup)
                cov, sums, stats = I.raster_layers(shape, rect, W, W, z, s, return_stats=True)
                # the same call without an image (cov = NULL): what is left is not the image's way to the host
                r["sums_only"] = timed(lambda: I.raster_layers(shape, rect, W, W, z, s, want_cov=False), a.calls, a.warmup)
            finally:
                I.set_pruning(2)
            r.update(covered_samples=int(sums.sum()), stats=stats, tiles_evaluated=stats[1], tiles_filled=stats[2],
                     samples_evaluated=stats[3], tiles_evaluated_share=stats[1] / stats[0], tiles_filled_share=stats[2] / stats[0])
            res["raster_s%d_level_%d" % (s, level)] = r
            print("raster s", s, "level", level, r, flush=True)
            del cov
        if a.no_route:
            continue
        # the earlier route: the same (W s)^2 L samples through the point evaluator, a few planes per call.
        # One point array serves every call: only its z column changes, outside the timed region
        mx, my = I.raster_coords(rect, W, W, s)
        per_plane = len(mx) * len(my)
        planes = max(1, min(L, a.batch_samples // per_plane))
        yy, xx = np.meshgrid(my, mx, indexing="ij")
        buf = np.empty((planes, per_plane, 3), np.float32)
        buf[:, :, 0] = xx.reshape(-1)
        buf[:, :, 1] = yy.reshape(-1)
        del xx, yy
        with I.ImplicitService(shape) as svc:
            def route():
                ms = 0.0
                for l0 in range(0, L, planes):
                    n = min(planes, L - l0)
                    buf[:n, :, 2] = z[l0:l0 + n, None]
                    pts = buf[:n].reshape(-1, 3)
                    t0 = time.perf_counter()
                    svc.eval(pts)
                    ms += (time.perf_counter() - t0) * 1e3
                return ms
            for _ in range(a.warmup):
                route()
            r = summary([route() for _ in range(a.calls)])
        # the service's point module compiles in the background: no exit with that compile in flight
        I.jit_wait()
        r.update(points=int(per_plane) * L, planes_per_call=planes, upload_bytes=int(per_plane) * L * 12)
        res["eval_points_route_s%d" % s] = r
        print("eval_points route s", s, r, flush=True)
        del buf
        for level in (2, 0):
            res["ratio_route_over_raster_s%d_level_%d" % (s, level)] = r["ms_median"] / res["raster_s%d_level_%d" % (s, level)]["ms_median"]
    out = a.out or os.path.join(ROOT, "profiles", "r%02d_raster_measure.json" % next_round())
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out, {k: v for k, v in res.items() if k.startswith("ratio")})


if __name__ == "__main__":
    main()
