"""What raster_layers, layer_islands and layer_distance share on the host (abi_queries.hip LayerImages): the
chunk walk, the scratch and the staging slots.  Their own suites compare each with its restatement; here the
three run on one engine, alone with one chunk and then interleaved with a layer per chunk, and every integer
must be the same.  40 x 40 pixels are 3 x 3 raster tiles with an image pitch (48) that is not the width, so
raster's pitched copy runs; five chunks use both of its staging slots and end on the first; the other two
carry a layer from each chunk to the next.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_raster as gr   # noqa: E402  (its shapes, rects and planes; its tests are not collected from here)

pytestmark = pytest.mark.gpu

Z5 = np.array([-0.3, -0.125, 0.05, -0.2, -0.55], np.float32)
CHUNK_VARS = ("IMPLISOLID_RASTER_CHUNK", "IMPLISOLID_ISLANDS_CHUNK", "IMPLISOLID_DISTANCE_CHUNK")


@pytest.mark.parametrize("level", [0, 2])
def test_interleaved_and_chunked_calls_equal_the_solo_ones(impli, level, monkeypatch):
    a = (gr.SHAPES["tree_deep"], gr.RECTS["non_dyadic"], 40, 40, Z5, 2)
    other = (gr.SHAPES["tree_deep"], gr.RECTS["non_dyadic"], 33, 17, gr.Z, 4)
    impli.set_pruning(level)
    try:
        cov, sums, rstats = impli.raster_layers(*a, return_stats=True)
        offs, comps, labels, istats = impli.layer_islands(*a, 3, 8, want_labels=True, return_stats=True)
        dist, rec, dstats = impli.layer_distance(*a, 3, 2, return_stats=True)
        for v in CHUNK_VARS:
            monkeypatch.setenv(v, "1")   # below one layer's tiles: a layer per chunk
        dist_ms = impli.layer_distance_kernel_ms(False)
        dist2, rec2, dstats2 = impli.layer_distance(*a, 3, 2, return_stats=True)
        impli.islands_kernel_ms(True)
        try:
            offs2, comps2, labels2, istats2 = impli.layer_islands(*a, 3, 8, want_labels=True, return_stats=True)
        finally:
            ms = impli.islands_kernel_ms(False)
        impli.layer_islands(*other, 5, 4, want_labels=True)   # another size: the scratch is resized and used again
        impli.layer_distance(*other, 5, 0)
        cov2, sums2, rstats2 = impli.raster_layers(*a, return_stats=True)
    finally:
        impli.set_pruning(2)
    print("raster, tiles, merge, rows + scan, records + tally ms over five chunks", ms)
    assert len(ms) == 5 and all(v >= 0 for v in ms)
    assert impli.islands_kernel_ms(False) == ms, "an untimed call leaves the last timed call's figures"
    assert impli.layer_distance_kernel_ms(False) == dist_ms
    assert rstats[4] == istats[4] == dstats[4] == 1 and rstats2[4] == istats2[4] == dstats2[4] == 5
    assert np.array_equal(cov2, cov) and np.array_equal(sums2, sums) and rstats2[:4] == rstats[:4]
    assert np.array_equal(offs2, offs) and np.array_equal(comps2, comps) and np.array_equal(labels2, labels)
    assert istats2[:4] == istats[:4] and istats2[5:] == istats[5:]
    assert np.array_equal(dist2, dist) and np.array_equal(rec2, rec) and dstats2[:4] == dstats[:4] and dstats2[5:] == dstats[5:]
    assert rstats[:4] == istats[:4] == dstats[:4], "one image head"
    assert sums.sum() > 0 and istats[7] > 0 and len(comps) > 0 and dstats[5] > 0 and (dist > 0).any(), "or nothing was compared"
    assert cov.shape == (5, 40, 40) and labels.shape == dist.shape == (5, 40, 40)
