"""Measure layer_bodies against the route a caller had before it: raster_layers with the image returned, then a
3D labelling on the host.

Scene: config 4's tree, rect +-1, 2048 x 2048 pixels, the raster section's 64 planes, one sample per pixel, pruning
level 2; target 1 (the solid, connectivity 26) and target 0 (the empty class, connectivity 6).  Per target: the
wall time of the whole call (median and min-max of 9 calls after 3 warm-up calls), the four passes by HIP events
(layer_bodies_kernel_ms: the median of the timed calls), the row runs, the bodies, and the bytes that come down.
The earlier route: raster_layers' wall time with the image, measured the same way in the same process, plus the
host labelling of the returned stack (scipy.ndimage.label with the same connectivity, and the volumes by a
bincount), timed on the whole stack; its body count and sorted volumes must equal the query's.  Without scipy
the host labelling is not measured and the file says so.  Writes profiles/r<next round>_bodies_probe.json.

    python tools/bodies_probe.py [--size 2048] [--layers 64] [--calls 9] [--warmup 3] [--host-calls 3]
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
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-calls", type=int, default=3, help="host labellings of the whole stack per target")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    try:   # torch's HIP runtime first, as in bench.py
        import torch
        torch.cuda.is_available()
    except Exception:
        pass
    import implisolid_amd as I
    from implisolid_amd import scenes
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None

    shape = scenes.config4()[0]
    rect = np.array([-1, 1, -1, 1], np.float32)
    W, L = a.size, a.layers
    z = (-1.0 + 2.0 * (np.arange(L) + 0.5) / L).astype(np.float32)
    res = {"scene": "config4 tree", "width": W, "height": W, "layers": L, "calls": a.calls, "warmup": a.warmup, "pruning": 2,
           "passes": ["raster", "count_scan_emit", "link", "finish"]}
    I.set_pruning(2)
    # the earlier route's first half is the same for both targets: the image comes down
    rr = timed(lambda: I.raster_layers(shape, rect, W, W, z, 1), a.calls, a.warmup)
    rr["bytes_down"] = int(W * W * L + 8 * L)
    res["raster_with_image"] = rr
    print("raster with image", rr, flush=True)
    cov, _ = I.raster_layers(shape, rect, W, W, z, 1)
    for target, connectivity in ((1, 26), (0, 6)):
        r = timed(lambda: I.layer_bodies(shape, rect, W, W, z, 1, 1, target, connectivity), a.calls, a.warmup)
        I.layer_bodies_kernel_ms(True)
        passes = []
        for _ in range(a.calls):
            offs, bodies, stats = I.layer_bodies(shape, rect, W, W, z, 1, 1, target, connectivity, return_stats=True)
            passes.append(I.layer_bodies_kernel_ms(True))
        I.layer_bodies_kernel_ms(False)
        r["pass_ms_median"] = [float(v) for v in np.median(np.array(passes), axis=0)]
        r.update(stats=stats, row_runs=stats[5], bodies=stats[6], target_voxels=stats[7],
                 device_bytes_runs=int(16 * stats[5]), bytes_down=int(64 * stats[6] + 4 * (L + 1) * stats[4] + 16 * stats[4] + 16))
        rw = timed(lambda: I.layer_bodies(shape, rect, W, W, z, 1, 1, target, connectivity, want_runs=True), a.calls, a.warmup)
        rw["bytes_down"] = r["bytes_down"] + int(12 * stats[5])
        r["with_runs"] = rw
        if ndimage is None:
            r["earlier_route"] = "unmeasured: scipy is not installed, there is no host labelling to time"
        else:
            structure = ndimage.generate_binary_structure(3, 3 if connectivity == 26 else 1)
            lab = []
            for _ in range(a.host_calls):
                t0 = time.perf_counter()
                labels, n = ndimage.label((cov >= 1) == (target == 1), structure=structure)
                volumes = np.bincount(labels.reshape(-1), minlength=n + 1)[1:]
                lab.append((time.perf_counter() - t0) * 1e3)
            same = bool(n == len(bodies) and np.array_equal(np.sort(volumes), np.sort(bodies["volume"])))
            del labels
            r["earlier_route"] = {"raster_with_image": rr, "host_label": summary(lab), "host_calls": a.host_calls,
                                  "equal_bodies_and_volumes": same, "ms_median": rr["ms_median"] + float(np.median(lab))}
            r["ratio_to_earlier_route"] = r["earlier_route"]["ms_median"] / r["ms_median"]
            r["below_earlier_route"] = bool(r["ms_median"] < r["earlier_route"]["ms_median"])
        res["bodies_target_%d_connectivity_%d" % (target, connectivity)] = r
        print("bodies target", target, "connectivity", connectivity, r, flush=True)
    out = a.out or os.path.join(ROOT, "profiles", "r%02d_bodies_probe.json" % next_round())
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", out)


if __name__ == "__main__":
    main()
