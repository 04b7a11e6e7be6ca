"""Measure mass_moments against the route the library offered before it: every sample point of the
grid through ImplicitService.eval in chunks (the numpy sums that would follow are not timed, which
favours that route).

Scene: config 4's tree over its +-1 box at depth 9 (2^27 cells).  Wall clock around each call (the ten
sums and the layer counts are host resident when it returns): median and min-max of 20 calls after 5
warm-up calls, at pruning levels 2 and 0, with the call's stats.  Writes
profiles/r<next round>_mass_measure.json.

    python tools/mass_measure.py [--depth 9] [--calls 20] [--warmup 5] [--chunk-layers 32]
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
    ap.add_argument("--depth", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--chunk-layers", type=int, default=32, help="z layers per ImplicitService.eval call")
    ap.add_argument("--skip-route", action="store_true", help="do not time the ImplicitService.eval route")
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
    box = np.array([-1, 1, -1, 1, -1, 1], np.float32)
    depth, N = a.depth, 1 << a.depth
    res = {"scene": "config4 tree", "depth": depth, "cells": N ** 3, "calls": a.calls, "warmup": a.warmup}
    for level in (2, 0):
        I.set_pruning(level)
        try:
            r = timed(lambda: I.mass_moments(shape, box, depth), a.calls, a.warmup)
            mom, layers, stats = I.mass_moments(shape, box, depth, return_stats=True)
        finally:
            I.set_pruning(2)
        r.update(moments=[int(v) for v in mom], stats=stats, samples_share=stats[2] / N ** 3, whole_share=stats[1] / N ** 3)
        res["mass_level_%d" % level] = r
        print("mass level", level, r, flush=True)
    res["levels_agree"] = res["mass_level_0"]["moments"] == res["mass_level_2"]["moments"]
    p = I.mass_properties(shape, box, depth)
    res["properties"] = {"volume": p["volume"], "centre": p["centre"].tolist(), "inertia": p["inertia"].tolist()}

    if not a.skip_route:
        # the earlier route: the same N^3 sample points through the point evaluator, in chunks of layers
        M = I.mass_mids(box, depth)
        chunks = []
        for k0 in range(0, N, a.chunk_layers):
            zz, yy, xx = np.meshgrid(M[2][k0:k0 + a.chunk_layers], M[1], M[0], indexing="ij")
            chunks.append(np.ascontiguousarray(np.stack([xx, yy, zz], axis=-1).reshape(-1, 3), np.float32))
        with I.ImplicitService(shape) as svc:
            def route():
                for c in chunks:
                    svc.eval(c)
            r = timed(route, a.calls, a.warmup)
            n = sum(int((~(svc.eval(c) < 0)).sum()) for c in chunks)   # untimed: the route's count
        # the service's point module compiles in the background: no exit with that compile in flight
        I.jit_wait()
        r.update(points=int(sum(len(c) for c in chunks)), chunk_layers=a.chunk_layers, solid_cells=n)
        res["route_counts_the_same_cells"] = n == res["mass_level_2"]["moments"][0]
        res["eval_points_route"] = r
        print("eval_points route", r, flush=True)
        for level in (2, 0):
            res["ratio_route_over_mass_level_%d" % level] = r["ms_median"] / res["mass_level_%d" % level]["ms_median"]
    out = a.out or os.path.join(ROOT, "profiles", "r%02d_mass_measure.json" % next_round())
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out, {k: v for k, v in res.items() if k.startswith("ratio")})


if __name__ == "__main__":
    main()
