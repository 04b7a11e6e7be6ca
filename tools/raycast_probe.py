"""Time render_view on the GPU: a size x size orthographic view of config 4's tree and of the sphere of
radius 1/2, looking down a diagonal at the box +-1, N steps and B bisection rounds, at pruning levels 0
and 2.  The two kernels are timed with HIP events around their launches (raycast_kernel_ms); the wall
clock of the whole call (upload, kernels, results to the host) is printed beside them.  Medians of
`calls` calls after `warmup` warm-up calls.  Prints rays/s by the kernels' time, the segment figures of
the call's stats and the share of segments level 2 skips; --out writes the figures as JSON.

    python tools/raycast_probe.py [--size 1024] [--steps 1024] [--bisect 16] [--calls 10] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024, help="pixels per axis")
    ap.add_argument("--steps", type=int, default=1024)
    ap.add_argument("--bisect", type=int, default=16)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    try:   # torch's HIP runtime first, as in bench.py
        import torch
        torch.cuda.is_available()
    except Exception:
        pass
    import implisolid_amd as I
    from implisolid_amd import scenes

    W = a.size
    # the eye 3 away along a diagonal; the view plane 2.5 high covers the box's silhouette; the rays
    # cross the box between t = 3 - sqrt(3) and 3 + sqrt(3)
    view = dict(eye=(np.sqrt(3.0), np.sqrt(3.0), np.sqrt(3.0)), target=(0, 0, 0), up=(0, 0, 1), width=W, height=W,
                t0=1.0, t1=5.0, steps=a.steps, bisect=a.bisect, ortho_height=2.5)
    shapes = {"config4 tree": scenes.config4()[0], "sphere": {"type": "iellipsoid", "matrix": list(scenes.EYE)}}
    res = {"size": W, "steps": a.steps, "bisect": a.bisect, "calls": a.calls, "warmup": a.warmup}
    I.raycast_kernel_ms(True)
    try:
        for name, shape in shapes.items():
            for level in (0, 2):
                I.set_pruning(level)
                march, finish, wall = [], [], []
                for k in range(a.warmup + a.calls):
                    t0 = time.perf_counter()
                    depth, nrm, mask, stats = I.render_view(shape, return_stats=True, **view)
                    ms = (time.perf_counter() - t0) * 1e3
                    if k >= a.warmup:
                        m, f = I.raycast_kernel_ms(True)
                        march.append(m)
                        finish.append(f)
                        wall.append(ms)
                km = float(np.median(march)) + float(np.median(finish))
                r = {"march_ms": float(np.median(march)), "finish_ms": float(np.median(finish)), "call_wall_ms": float(np.median(wall)),
                     "rays_per_s_kernels": W * W / (km * 1e-3), "stats": stats, "hit_share": stats[3] / (W * W),
                     "segments_skipped_share_up_to_hit": stats[1] / max(stats[1] + stats[2], 1),
                     "segments_evaluated_share_of_all": stats[2] / stats[0]}
                res["%s level %d" % (name, level)] = r
                print(name, "level", level, json.dumps(r), flush=True)
    finally:
        I.set_pruning(2)
        I.raycast_kernel_ms(False)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
