"""Measure slice_layers against the route the library offered before it: every sample of every plane
through ImplicitService.eval (the numpy marching squares that would follow is not timed).

Scene: config 4's tree, rect +-1, R = 512, 256 planes evenly spaced inside z in (-1, 1).  Wall clock
around each call (the result is host resident when it returns): median and min-max of 20 calls after
5 warm-up calls, at pruning levels 0 and 2, with the call's stats.  Writes
profiles/r<next round>_slice_measure.json.

    python tools/slice_measure.py [--resolution 512] [--layers 256] [--calls 20] [--warmup 5]
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


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--resolution", type=int, default=512)
    ap.add_argument("--layers", type=int, default=256)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch-layers", type=int, default=16, help="planes per ImplicitService.eval call")
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
    R, L = a.resolution, a.layers
    z = (-1.0 + 2.0 * (np.arange(L) + 0.5) / L).astype(np.float32)
    res = {"scene": "config4 tree", "resolution": R, "layers": L, "calls": a.calls, "warmup": a.warmup}
    for level in (0, 2):
        I.set_pruning(level)
        try:
            r = timed(lambda: I.slice_layers(shape, rect, R, z), a.calls, a.warmup)
            seg, keys, offs, stats = I.slice_layers(shape, rect, R, z, return_stats=True)
        finally:
            I.set_pruning(2)
        r.update(segments=int(len(seg)), stats=stats, tiles_evaluated_share=stats[1] / stats[0])
        res["slice_level_%d" % level] = r
        print("slice level", level, r, flush=True)

    # the earlier route: the same (R + 1)^2 L samples through the point evaluator, in batches of planes
    xs, ys = I.slice_coords(rect, R)
    batches = []
    for l0 in range(0, L, a.batch_layers):
        zz, yy, xx = np.meshgrid(z[l0:l0 + a.batch_layers], ys, xs, indexing="ij")
        batches.append(np.ascontiguousarray(np.stack([xx, yy, zz], axis=-1).reshape(-1, 3), np.float32))
    with I.ImplicitService(shape) as svc:
        def route():
            for b in batches:
                svc.eval(b)
        r = timed(route, a.calls, a.warmup)
    # the service's point module compiles in the background: no exit with that compile in flight
    I.jit_wait()
    r.update(points=int(sum(len(b) for b in batches)), batch_layers=a.batch_layers)
    res["eval_points_route"] = r
    print("eval_points route", r, flush=True)
    for level in (0, 2):
        res["ratio_route_over_slice_level_%d" % level] = r["ms_median"] / res["slice_level_%d" % level]["ms_median"]
    out = a.out or os.path.join(ROOT, "profiles", "r%02d_slice_measure.json" % next_round())
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out, {k: v for k, v in res.items() if k.startswith("ratio")})


if __name__ == "__main__":
    main()
