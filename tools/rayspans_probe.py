"""Time ray_spans on the GPU on tools/raycast_probe.py's view: a size x size orthographic view of config 4's
tree and of the sphere of radius 1/2, looking down a diagonal at the box +-1, N steps and B bisection rounds,
at pruning levels 0 and 2.  The kernels are timed with HIP events around their launches
(ray_spans_kernel_ms: march; scan, tally and emit; refine); the wall clock of the whole call (upload,
kernels, the per-chunk read-backs, results to the host and the copy out of the slot) is printed beside them.
Medians of `calls` calls after `warmup` warm-up calls.  Prints rays/s by the kernels' time and the call's
stats; --out writes the figures as JSON.

    python tools/rayspans_probe.py [--size 1024] [--steps 1024] [--bisect 16] [--calls 10] [--warmup 3]
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
    # raycast_probe's view: the eye 3 away along a diagonal, the view plane 2.5 high, t in [1, 5]
    o, d = I.view_rays(eye=(np.sqrt(3.0), np.sqrt(3.0), np.sqrt(3.0)), target=(0, 0, 0), up=(0, 0, 1), width=W, height=W,
                       ortho_height=2.5)
    shapes = {"config4 tree": scenes.config4()[0], "sphere": {"type": "iellipsoid", "matrix": list(scenes.EYE)}}
    res = {"size": W, "steps": a.steps, "bisect": a.bisect, "calls": a.calls, "warmup": a.warmup}
    I.ray_spans_kernel_ms(True)
    try:
        for name, shape in shapes.items():
            for level in (0, 2):
                I.set_pruning(level)
                march, emit, refine, wall = [], [], [], []
                for k in range(a.warmup + a.calls):
                    t0 = time.perf_counter()
                    offs, kk, t, f, _, stats = I.ray_spans(shape, o, d, 1.0, 5.0, a.steps, a.bisect, return_stats=True)
                    ms = (time.perf_counter() - t0) * 1e3
                    if k >= a.warmup:
                        m, e, r = I.ray_spans_kernel_ms(True)
                        march.append(m)
                        emit.append(e)
                        refine.append(r)
                        wall.append(ms)
                length, count = I.span_lengths(offs, t, d)
                km = float(np.median(march)) + float(np.median(emit)) + float(np.median(refine))
                r = {"march_ms": float(np.median(march)), "emit_ms": float(np.median(emit)), "refine_ms": float(np.median(refine)),
                     "call_wall_ms": float(np.median(wall)), "rays_per_s_kernels": W * W / (km * 1e-3), "stats": stats,
                     "segments_proved_share": (stats[1] + stats[2]) / stats[0], "most_spans_a_ray": int(count.max()),
                     "mean_thickness_of_rays_with_a_span": float(length[count > 0].mean()) if stats[5] else 0.0}
                res["%s level %d" % (name, level)] = r
                print(name, "level", level, json.dumps(r), flush=True)
    finally:
        I.set_pruning(2)
        I.ray_spans_kernel_ms(False)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
