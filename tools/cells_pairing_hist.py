#!/usr/bin/env python3
"""Config 4's non-empty MC units by non-trivial cell count (<= 32: small, paired in the vertex pass;
33-64; > 64) and the vertex pass's wave work items with and without pairing.
usage: python tools/cells_pairing_hist.py OUT.json [R ...]   (default 512 256)"""
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    import implisolid_amd as I
    from implisolid_amd import scenes
    torch.cuda.init()
    out = {"scene": "config 4", "wave_slots": 6144, "runs": []}
    for R in [int(x) for x in sys.argv[2:]] or [512, 256]:
        shape, mc = scenes.config4(R)
        s = I.Slab(shape, mc)
        s.run()
        st = (ctypes.c_int64 * 13)()
        assert I.lib().implisolid_slab_stats_n(s.h, st, 13) == 13
        sg = s.read_signs().astype(bool)
        s.close()
        c = [sg[dz:sg.shape[0] - 1 + dz, dy:sg.shape[1] - 1 + dy, dx:sg.shape[2] - 1 + dx]
             for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
        any_, all_ = c[0].copy(), c[0].copy()
        for x in c[1:]:
            any_ |= x
            all_ &= x
        per_row = (any_ & ~all_).sum(axis=2).reshape(-1)
        per_row = np.concatenate([per_row, np.zeros(-per_row.size % 4, per_row.dtype)])
        ne = per_row.reshape(-1, 4).sum(axis=1)
        ne = ne[ne > 0]
        n = int(ne.size)
        unit_parts, small, heavy_parts, items = int(st[9]), int(st[10]), int(st[11]), int(st[12])
        out["runs"].append({
            "R": R, "nonempty_units": n, "cells": int(ne.sum()),
            "mean": round(float(ne.mean()), 1), "p50": int(np.percentile(ne, 50)), "p99": int(np.percentile(ne, 99)),
            "max": int(ne.max()),
            "share_le_32": round(float((ne <= 32).mean()), 4), "share_le_64": round(float((ne <= 64).mean()), 4),
            "share_gt_64": round(float((ne > 64).mean()), 4),
            # the count kernel's classes: a small unit also has its cells in at most 8 of its chunks
            "small_units": small, "heavy_parts": heavy_parts, "light_parts": unit_parts - heavy_parts - small,
            "wave_items_without_pairing": unit_parts, "wave_items_with_pairing": items,
            "generations_without": round(unit_parts / 6144, 2), "generations_with": round(items / 6144, 2)})
        print(json.dumps(out["runs"][-1]), flush=True)
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    I.jit_wait()   # the trees' modules compile in the background: no exit with a compile in flight


if __name__ == "__main__":
    main()
