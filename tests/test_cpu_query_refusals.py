"""The refusal paths of the field queries (bounds, slice, raster, islands, layer distance, raycast, ray
spans, mass, their host-only companions and the two interval probes): the return value and the exact
implisolid_last_error() text of every request that is refused before anything reaches a device, and
that the library answers the next call.  The literals in EXPECTED were recorded from the library before
the queries moved to csrc/abi_queries.hip (the layer queries since to csrc/abi_layers.hip), and those of the layer and ray entries before these came to
share their request checks (LayerRequest, ray_request): they pin that neither changed an error path, nor
which of two faults at once is reported.  No GPU."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

fp = ctypes.POINTER(ctypes.c_float)
dp = ctypes.POINTER(ctypes.c_double)
ip = ctypes.POINTER(ctypes.c_int32)
up = ctypes.POINTER(ctypes.c_uint32)
lp = ctypes.POINTER(ctypes.c_int64)
ulp = ctypes.POINTER(ctypes.c_uint64)
bp = ctypes.POINTER(ctypes.c_uint8)

EYE = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]
SPHERE = ('{"type": "iellipsoid", "matrix": %s}' % EYE).encode()
TRUNCATED = b'{"type": "iellipsoid", "matrix": [1, 0'          # not JSON
NO_SUCH_TYPE = ('{"type": "no_such_solid", "matrix": %s}' % EYE).encode()
NAN, INF = float("nan"), float("inf")


def F(*v):
    return np.array(v, np.float32)


class Args:
    """One entry's valid request; a case replaces some arguments by name and calls it."""

    def __init__(self, fn, **valid):
        self.fn, self.valid = fn, valid

    def __call__(self, L, **changed):
        unknown = set(changed) - set(self.valid)
        assert not unknown, unknown
        keep = []   # the arrays outlive the call

        def c(v):
            if isinstance(v, np.ndarray):
                keep.append(v)
                t = {np.float32: fp, np.float64: dp, np.int32: ip, np.uint32: up, np.int64: lp, np.uint64: ulp, np.uint8: bp}
                return v.ctypes.data_as(t[v.dtype.type])
            return v
        return int(getattr(L, self.fn)(*[c(changed.get(k, v)) for k, v in self.valid.items()]))


BOX = F(-1, 1, -1, 1, -1, 1)
RECT = F(-1, 1, -1, 1)
Z2 = F(-0.25, 0.25)
RAYS = F(-2, 0, 0, -2, 0.25, 0)
DIRS = F(1, 0, 0, 1, 0, 0)


def i64(n):
    return np.zeros(n, np.int64)


ENTRY = {
    "bounds": Args("implisolid_bounds", shape=SPHERE, irm=0, search=BOX, depth=4, out=F(*[0] * 6), stats=i64(4)),
    "mass": Args("implisolid_mass", shape=SPHERE, irm=0, box=BOX, depth=4, moments=np.zeros(10, np.uint64), layers=i64(16),
                 stats=i64(4)),
    "slice": Args("implisolid_slice", shape=SPHERE, irm=0, rect=RECT, resolution=8, z=Z2, n_layers=2, offsets=i64(3),
                  stats=i64(4)),
    "raster": Args("implisolid_raster", shape=SPHERE, irm=0, rect=RECT, width=8, height=8, supersample=1, z=Z2, n_layers=2,
                   cov=np.zeros(128, np.uint8), sums=i64(2), stats=i64(5)),
    "raycast": Args("implisolid_raycast", shape=SPHERE, irm=0, origins=RAYS, dirs=DIRS, n=2, t0=0.0, t1=4.0, steps=8, bisect=4,
                    hit=np.zeros(2, np.int32), t=F(0, 0), f=F(0, 0), normals=F(*[0] * 6), stats=i64(6)),
    "islands": Args("implisolid_islands", shape=SPHERE, irm=0, rect=RECT, width=8, height=8, supersample=2, z=Z2, n_layers=2,
                    threshold=1, connectivity=8, offsets=i64(3), labels=np.zeros(128, np.int32), stats=i64(8)),
    "distance": Args("implisolid_layer_distance", shape=SPHERE, irm=0, rect=RECT, width=8, height=8, supersample=2, z=Z2,
                     n_layers=2, threshold=1, reach2=0, dist=np.zeros(128, np.int32), rec=i64(8), stats=i64(8)),
    "ray_spans": Args("implisolid_ray_spans", shape=SPHERE, irm=0, origins=RAYS, dirs=DIRS, n=2, t0=0.0, t1=4.0, steps=8, bisect=4,
                      want_normals=0, offsets=i64(3), stats=i64(8)),
    "intervals": Args("implisolid_debug_intervals", shape=SPHERE, irm=0, variant=0, boxes=F(*BOX), modes_in=None, n=1,
                      iv=F(0, 0), modes_out=np.zeros(1, np.uint64)),
    "eval_modes": Args("implisolid_debug_eval_modes", shape=SPHERE, irm=0, xyz=F(0, 0, 0), modes=np.zeros(1, np.uint64), n=1,
                       f=F(0)),
    # the host-only entries
    "bounds_edges": Args("implisolid_bounds_edges", search=BOX, depth=3, edges=F(*[0] * 27)),
    "fit_box": Args("implisolid_fit_box", search=BOX, bounds=F(-.5, .5, -.5, .5, -.5, .5), resolution=16, margin=2,
                    out=F(*[0] * 6)),
    "slice_coords": Args("implisolid_slice_coords", rect=RECT, resolution=4, xs=F(*[0] * 5), ys=F(*[0] * 5)),
    "slice_loops": Args("implisolid_slice_loops", keys=np.array([1, 2, 2, 1], np.uint32), n=2, order=i64(2), offsets=i64(3),
                        closed=np.zeros(2, np.uint8)),
    "slice_copy": Args("implisolid_slice_copy", xy=F(*[0] * 4), keys=np.zeros(2, np.uint32)),
    "raster_coords": Args("implisolid_raster_coords", rect=RECT, width=4, height=4, supersample=2, mx=F(*[0] * 8),
                          my=F(*[0] * 8)),
    "ray_params": Args("implisolid_ray_params", t0=0.0, t1=1.0, steps=4, ts=F(*[0] * 5)),
    "mass_mids": Args("implisolid_mass_mids", box=BOX, depth=3, mids=F(*[0] * 24)),
    "mass_physical": Args("implisolid_mass_physical", box=BOX, depth=3, moments=np.zeros(10, np.uint64),
                          out=np.zeros(10, np.float64)),
}

REVERSED_BOX = F(1, -1, -1, 1, -1, 1)
NAN_BOX = F(-1, 1, -1, NAN, -1, 1)
MANY_Z = np.zeros(65537, np.float32)
REVERSED_RECT = F(1, -1, -1, 1)
NAN_ORIGIN = F(-2, 0, 0, -2, NAN, 0)

# (entry, what the case changes in the entry's valid request)
CASES = {
    # ---- bounds -----------------------------------------------------------------------------------
    "bounds null shape": ("bounds", dict(shape=None)),
    "bounds null search": ("bounds", dict(search=None)),
    "bounds null out": ("bounds", dict(out=None)),
    "bounds depth 2": ("bounds", dict(depth=2)),
    "bounds depth 11": ("bounds", dict(depth=11)),
    "bounds reversed box": ("bounds", dict(search=REVERSED_BOX)),
    "bounds nan box": ("bounds", dict(search=NAN_BOX)),
    "bounds truncated shape": ("bounds", dict(shape=TRUNCATED)),
    "bounds unknown type": ("bounds", dict(shape=NO_SUCH_TYPE)),
    "bounds truncated shape, depth 2": ("bounds", dict(shape=TRUNCATED, depth=2)),
    "bounds unknown type, reversed box": ("bounds", dict(shape=NO_SUCH_TYPE, search=REVERSED_BOX)),
    # ---- mass -------------------------------------------------------------------------------------
    "mass null shape": ("mass", dict(shape=None)),
    "mass null box": ("mass", dict(box=None)),
    "mass null moments": ("mass", dict(moments=None)),
    "mass depth 2": ("mass", dict(depth=2)),
    "mass depth 11": ("mass", dict(depth=11)),
    "mass reversed box": ("mass", dict(box=REVERSED_BOX)),
    "mass nan box": ("mass", dict(box=NAN_BOX)),
    "mass truncated shape": ("mass", dict(shape=TRUNCATED)),
    "mass unknown type": ("mass", dict(shape=NO_SUCH_TYPE)),
    "mass truncated shape, depth 11": ("mass", dict(shape=TRUNCATED, depth=11)),
    "mass unknown type, nan box": ("mass", dict(shape=NO_SUCH_TYPE, box=NAN_BOX)),
    # ---- slice ------------------------------------------------------------------------------------
    "slice null shape": ("slice", dict(shape=None)),
    "slice null rect": ("slice", dict(rect=None)),
    "slice null z": ("slice", dict(z=None)),
    "slice null offsets": ("slice", dict(offsets=None)),
    "slice 0 layers": ("slice", dict(n_layers=0)),
    "slice 65537 layers": ("slice", dict(z=MANY_Z, n_layers=65537, offsets=i64(65538))),
    "slice inf z": ("slice", dict(z=F(0, INF))),
    "slice nan z": ("slice", dict(z=F(NAN, 0))),
    "slice resolution 0": ("slice", dict(resolution=0)),
    "slice resolution 4097": ("slice", dict(resolution=4097)),
    "slice reversed rect": ("slice", dict(rect=F(1, -1, -1, 1))),
    "slice truncated shape": ("slice", dict(shape=TRUNCATED)),
    "slice unknown type": ("slice", dict(shape=NO_SUCH_TYPE)),
    "slice truncated shape, 0 layers": ("slice", dict(shape=TRUNCATED, n_layers=0)),
    "slice unknown type, resolution 4097": ("slice", dict(shape=NO_SUCH_TYPE, resolution=4097)),
    "slice truncated shape, nan z": ("slice", dict(shape=TRUNCATED, z=F(NAN, 0))),
    # ---- raster -----------------------------------------------------------------------------------
    "raster null shape": ("raster", dict(shape=None)),
    "raster null rect": ("raster", dict(rect=None)),
    "raster null z": ("raster", dict(z=None)),
    "raster null sums": ("raster", dict(sums=None)),
    "raster 0 layers": ("raster", dict(n_layers=0)),
    "raster 65537 layers": ("raster", dict(z=MANY_Z, n_layers=65537, sums=i64(65537), cov=None)),
    "raster inf z": ("raster", dict(z=F(-INF, 0))),
    "raster nan z": ("raster", dict(z=F(0, NAN))),
    "raster width 0": ("raster", dict(width=0)),
    "raster width 16385": ("raster", dict(width=16385, cov=None)),
    "raster height 0": ("raster", dict(height=0)),
    "raster height 16385": ("raster", dict(height=16385, cov=None)),
    "raster supersample 3": ("raster", dict(supersample=3)),
    "raster supersample 0": ("raster", dict(supersample=0)),
    "raster reversed rect": ("raster", dict(rect=F(-1, 1, 1, -1))),
    "raster truncated shape": ("raster", dict(shape=TRUNCATED)),
    "raster unknown type": ("raster", dict(shape=NO_SUCH_TYPE)),
    "raster truncated shape, supersample 3": ("raster", dict(shape=TRUNCATED, supersample=3)),
    "raster unknown type, width 0": ("raster", dict(shape=NO_SUCH_TYPE, width=0)),
    "raster truncated shape, 65537 layers": ("raster", dict(shape=TRUNCATED, z=MANY_Z, n_layers=65537, sums=i64(65537), cov=None)),
    # two faults at once, across each step of the order: pointers, n_layers, z, width / height, supersample, rect, shape
    "raster null rect, 0 layers": ("raster", dict(rect=None, n_layers=0)),
    "raster 0 layers, nan z": ("raster", dict(n_layers=0, z=F(NAN, 0))),
    "raster nan z, width 0": ("raster", dict(z=F(NAN, 0), width=0)),
    "raster height 0, supersample 3": ("raster", dict(height=0, supersample=3)),
    "raster supersample 3, reversed rect": ("raster", dict(supersample=3, rect=REVERSED_RECT)),
    "raster unknown type, reversed rect": ("raster", dict(shape=NO_SUCH_TYPE, rect=REVERSED_RECT)),
    # ---- islands: the checks it shares with raster, its own between supersample and the rect ---------------
    "islands null shape": ("islands", dict(shape=None)),
    "islands null rect": ("islands", dict(rect=None)),
    "islands null z": ("islands", dict(z=None)),
    "islands null offsets": ("islands", dict(offsets=None)),
    "islands 0 layers": ("islands", dict(n_layers=0)),
    "islands 65537 layers": ("islands", dict(z=MANY_Z, n_layers=65537, offsets=i64(65538), labels=None)),
    "islands inf z": ("islands", dict(z=F(-INF, 0))),
    "islands nan z": ("islands", dict(z=F(0, NAN))),
    "islands width 0": ("islands", dict(width=0)),
    "islands width 16385": ("islands", dict(width=16385)),
    "islands height 0": ("islands", dict(height=0)),
    "islands height 16385": ("islands", dict(height=16385)),
    "islands supersample 3": ("islands", dict(supersample=3)),
    "islands supersample 0": ("islands", dict(supersample=0)),
    "islands threshold 0": ("islands", dict(threshold=0)),
    "islands threshold 5": ("islands", dict(threshold=5)),
    "islands supersample 1, threshold 2": ("islands", dict(supersample=1, threshold=2)),
    "islands connectivity 6": ("islands", dict(connectivity=6)),
    "islands reversed rect": ("islands", dict(rect=REVERSED_RECT)),
    "islands nan rect": ("islands", dict(rect=F(-1, 1, NAN, 1))),
    "islands truncated shape": ("islands", dict(shape=TRUNCATED)),
    "islands unknown type": ("islands", dict(shape=NO_SUCH_TYPE)),
    "islands null z, 0 layers": ("islands", dict(z=None, n_layers=0)),
    "islands 0 layers, nan z": ("islands", dict(n_layers=0, z=F(NAN, 0))),
    "islands nan z, width 0": ("islands", dict(z=F(NAN, 0), width=0)),
    "islands height 16385, supersample 3": ("islands", dict(height=16385, supersample=3)),
    "islands supersample 3, threshold 0": ("islands", dict(supersample=3, threshold=0)),
    "islands supersample 0, connectivity 6": ("islands", dict(supersample=0, connectivity=6)),
    "islands threshold 5, connectivity 6": ("islands", dict(threshold=5, connectivity=6)),
    "islands threshold 0, reversed rect": ("islands", dict(threshold=0, rect=REVERSED_RECT)),
    "islands connectivity 6, reversed rect": ("islands", dict(connectivity=6, rect=REVERSED_RECT)),
    "islands unknown type, reversed rect": ("islands", dict(shape=NO_SUCH_TYPE, rect=REVERSED_RECT)),
    "islands truncated shape, connectivity 6": ("islands", dict(shape=TRUNCATED, connectivity=6)),
    "islands truncated shape, threshold 0": ("islands", dict(shape=TRUNCATED, threshold=0)),
    "islands unknown type, 65537 layers": ("islands", dict(shape=NO_SUCH_TYPE, z=MANY_Z, n_layers=65537, offsets=i64(65538), labels=None)),
    # ---- distance: the checks it shares with raster, its own between supersample and the rect ---------------
    "distance null shape": ("distance", dict(shape=None)),
    "distance null rect": ("distance", dict(rect=None)),
    "distance null z": ("distance", dict(z=None)),
    "distance null rec": ("distance", dict(rec=None)),
    "distance 0 layers": ("distance", dict(n_layers=0)),
    "distance 65537 layers": ("distance", dict(z=MANY_Z, n_layers=65537, rec=i64(4 * 65537), dist=None)),
    "distance inf z": ("distance", dict(z=F(-INF, 0))),
    "distance nan z": ("distance", dict(z=F(0, NAN))),
    "distance width 0": ("distance", dict(width=0)),
    "distance width 16385": ("distance", dict(width=16385)),
    "distance height 0": ("distance", dict(height=0)),
    "distance height 16385": ("distance", dict(height=16385)),
    "distance supersample 3": ("distance", dict(supersample=3)),
    "distance supersample 0": ("distance", dict(supersample=0)),
    "distance threshold 0": ("distance", dict(threshold=0)),
    "distance threshold 5": ("distance", dict(threshold=5)),
    "distance supersample 1, threshold 2": ("distance", dict(supersample=1, threshold=2)),
    "distance reach2 -1": ("distance", dict(reach2=-1)),
    "distance reversed rect": ("distance", dict(rect=REVERSED_RECT)),
    "distance nan rect": ("distance", dict(rect=F(-1, 1, NAN, 1))),
    "distance truncated shape": ("distance", dict(shape=TRUNCATED)),
    "distance unknown type": ("distance", dict(shape=NO_SUCH_TYPE)),
    "distance null z, 0 layers": ("distance", dict(z=None, n_layers=0)),
    "distance 0 layers, nan z": ("distance", dict(n_layers=0, z=F(NAN, 0))),
    "distance nan z, width 0": ("distance", dict(z=F(NAN, 0), width=0)),
    "distance height 16385, supersample 3": ("distance", dict(height=16385, supersample=3)),
    "distance supersample 3, threshold 0": ("distance", dict(supersample=3, threshold=0)),
    "distance supersample 0, reach2 -1": ("distance", dict(supersample=0, reach2=-1)),
    "distance threshold 5, reach2 -1": ("distance", dict(threshold=5, reach2=-1)),
    "distance threshold 0, reversed rect": ("distance", dict(threshold=0, rect=REVERSED_RECT)),
    "distance reach2 -1, reversed rect": ("distance", dict(reach2=-1, rect=REVERSED_RECT)),
    "distance unknown type, reversed rect": ("distance", dict(shape=NO_SUCH_TYPE, rect=REVERSED_RECT)),
    "distance truncated shape, reach2 -1": ("distance", dict(shape=TRUNCATED, reach2=-1)),
    "distance truncated shape, threshold 0": ("distance", dict(shape=TRUNCATED, threshold=0)),
    "distance unknown type, 65537 layers": ("distance", dict(shape=NO_SUCH_TYPE, z=MANY_Z, n_layers=65537, rec=i64(4 * 65537), dist=None)),
    # ---- raycast ----------------------------------------------------------------------------------
    "raycast null shape": ("raycast", dict(shape=None)),
    "raycast null origins": ("raycast", dict(origins=None)),
    "raycast null dirs": ("raycast", dict(dirs=None)),
    "raycast null hit": ("raycast", dict(hit=None)),
    "raycast null t": ("raycast", dict(t=None)),
    "raycast null f": ("raycast", dict(f=None)),
    "raycast n -1": ("raycast", dict(n=-1)),
    "raycast n 2^24 + 1": ("raycast", dict(n=(1 << 24) + 1)),
    "raycast steps 0": ("raycast", dict(steps=0)),
    "raycast steps 65537": ("raycast", dict(steps=65537)),
    "raycast bisect -1": ("raycast", dict(bisect=-1)),
    "raycast bisect 33": ("raycast", dict(bisect=33)),
    "raycast empty range": ("raycast", dict(t0=1.0, t1=1.0)),
    "raycast nan origin": ("raycast", dict(origins=NAN_ORIGIN)),
    "raycast inf direction": ("raycast", dict(dirs=F(1, 0, 0, INF, 0, 0))),
    "raycast truncated shape": ("raycast", dict(shape=TRUNCATED)),
    "raycast unknown type": ("raycast", dict(shape=NO_SUCH_TYPE)),
    "raycast truncated shape, bisect 33": ("raycast", dict(shape=TRUNCATED, bisect=33)),
    "raycast unknown type, steps 0": ("raycast", dict(shape=NO_SUCH_TYPE, steps=0)),
    "raycast truncated shape, nan origin": ("raycast", dict(shape=TRUNCATED, origins=NAN_ORIGIN)),
    "raycast unknown type, n -1": ("raycast", dict(shape=NO_SUCH_TYPE, n=-1)),
    "raycast no rays, truncated shape": ("raycast", dict(shape=TRUNCATED, n=0)),
    "raycast no rays, unknown type, null arrays": ("raycast", dict(shape=NO_SUCH_TYPE, n=0, origins=None, dirs=None, hit=None,
                                                                   t=None, f=None, normals=None)),
    "raycast no rays, steps 0": ("raycast", dict(n=0, steps=0)),
    "raycast n -1, bisect 33": ("raycast", dict(n=-1, bisect=33)),
    "raycast bisect 33, steps 0": ("raycast", dict(bisect=33, steps=0)),
    "raycast steps 0, empty range": ("raycast", dict(steps=0, t0=1.0, t1=1.0)),
    "raycast empty range, nan origin": ("raycast", dict(t0=1.0, t1=1.0, origins=NAN_ORIGIN)),
    # ---- ray_spans: the checks it shares with raycast ------------------------------------------------------
    "ray_spans null shape": ("ray_spans", dict(shape=None)),
    "ray_spans null origins": ("ray_spans", dict(origins=None)),
    "ray_spans null dirs": ("ray_spans", dict(dirs=None)),
    "ray_spans null offsets": ("ray_spans", dict(offsets=None)),
    "ray_spans n -1": ("ray_spans", dict(n=-1)),
    "ray_spans n 2^24 + 1": ("ray_spans", dict(n=(1 << 24) + 1)),
    "ray_spans bisect -1": ("ray_spans", dict(bisect=-1)),
    "ray_spans bisect 33": ("ray_spans", dict(bisect=33)),
    "ray_spans steps 0": ("ray_spans", dict(steps=0)),
    "ray_spans steps 65537": ("ray_spans", dict(steps=65537)),
    "ray_spans empty range": ("ray_spans", dict(t0=1.0, t1=1.0)),
    "ray_spans nan t1": ("ray_spans", dict(t1=NAN)),
    "ray_spans nan origin": ("ray_spans", dict(origins=NAN_ORIGIN)),
    "ray_spans inf direction": ("ray_spans", dict(dirs=F(1, 0, 0, INF, 0, 0))),
    "ray_spans truncated shape": ("ray_spans", dict(shape=TRUNCATED)),
    "ray_spans unknown type": ("ray_spans", dict(shape=NO_SUCH_TYPE)),
    "ray_spans null offsets, n -1": ("ray_spans", dict(offsets=None, n=-1)),
    "ray_spans n -1, bisect 33": ("ray_spans", dict(n=-1, bisect=33)),
    "ray_spans bisect 33, steps 0": ("ray_spans", dict(bisect=33, steps=0)),
    "ray_spans steps 0, empty range": ("ray_spans", dict(steps=0, t0=1.0, t1=1.0)),
    "ray_spans steps 0, nan origin": ("ray_spans", dict(steps=0, origins=NAN_ORIGIN)),
    "ray_spans empty range, nan origin": ("ray_spans", dict(t0=1.0, t1=1.0, origins=NAN_ORIGIN)),
    "ray_spans truncated shape, nan origin": ("ray_spans", dict(shape=TRUNCATED, origins=NAN_ORIGIN)),
    "ray_spans unknown type, empty range": ("ray_spans", dict(shape=NO_SUCH_TYPE, t0=1.0, t1=1.0)),
    "ray_spans no rays, truncated shape": ("ray_spans", dict(shape=TRUNCATED, n=0)),
    "ray_spans no rays, unknown type, null arrays": ("ray_spans", dict(shape=NO_SUCH_TYPE, n=0, origins=None, dirs=None)),
    "ray_spans no rays, steps 0": ("ray_spans", dict(n=0, steps=0)),
    "ray_spans no rays, empty range": ("ray_spans", dict(n=0, t0=1.0, t1=1.0)),
    # ---- the interval probes ----------------------------------------------------------------------
    "intervals null shape": ("intervals", dict(shape=None)),
    "intervals variant 3": ("intervals", dict(variant=3)),
    "intervals n -1": ("intervals", dict(n=-1)),
    "intervals null boxes": ("intervals", dict(boxes=None)),
    "intervals truncated shape": ("intervals", dict(shape=TRUNCATED)),
    "intervals unknown type": ("intervals", dict(shape=NO_SUCH_TYPE)),
    "eval_modes null shape": ("eval_modes", dict(shape=None)),
    "eval_modes n -1": ("eval_modes", dict(n=-1)),
    "eval_modes null modes": ("eval_modes", dict(modes=None)),
    "eval_modes truncated shape": ("eval_modes", dict(shape=TRUNCATED)),
    "eval_modes unknown type": ("eval_modes", dict(shape=NO_SUCH_TYPE)),
    # ---- host only --------------------------------------------------------------------------------
    "bounds_edges null search": ("bounds_edges", dict(search=None)),
    "bounds_edges null edges": ("bounds_edges", dict(edges=None)),
    "bounds_edges depth 2": ("bounds_edges", dict(depth=2)),
    "bounds_edges reversed box": ("bounds_edges", dict(search=REVERSED_BOX)),
    "fit_box null bounds": ("fit_box", dict(bounds=None)),
    "fit_box null out": ("fit_box", dict(out=None)),
    "fit_box resolution 4, margin 2": ("fit_box", dict(resolution=4)),
    "fit_box margin -1": ("fit_box", dict(margin=-1)),
    "slice_coords null rect": ("slice_coords", dict(rect=None)),
    "slice_coords null ys": ("slice_coords", dict(ys=None)),
    "slice_coords resolution 0": ("slice_coords", dict(resolution=0)),
    "slice_coords nan rect": ("slice_coords", dict(rect=F(-1, NAN, -1, 1))),
    "slice_loops null offsets": ("slice_loops", dict(offsets=None)),
    "slice_loops null keys": ("slice_loops", dict(keys=None)),
    "slice_loops n -1": ("slice_loops", dict(n=-1)),
    "slice_loops a key starts two segments": ("slice_loops", dict(keys=np.array([1, 2, 1, 3], np.uint32))),
    "raster_coords null rect": ("raster_coords", dict(rect=None)),
    "raster_coords null my": ("raster_coords", dict(my=None)),
    "raster_coords supersample 3": ("raster_coords", dict(supersample=3)),
    "raster_coords width 0": ("raster_coords", dict(width=0)),
    "ray_params null ts": ("ray_params", dict(ts=None)),
    "ray_params steps 0": ("ray_params", dict(steps=0)),
    "ray_params empty range": ("ray_params", dict(t0=2.0, t1=1.0)),
    "mass_mids null box": ("mass_mids", dict(box=None)),
    "mass_mids null mids": ("mass_mids", dict(mids=None)),
    "mass_mids depth 2": ("mass_mids", dict(depth=2)),
    "mass_physical null moments": ("mass_physical", dict(moments=None)),
    "mass_physical null out": ("mass_physical", dict(out=None)),
    "mass_physical depth 11": ("mass_physical", dict(depth=11)),
    "mass_physical reversed box": ("mass_physical", dict(box=REVERSED_BOX)),
}

# name -> (return value, implisolid_last_error()), as the library answered before the move
EXPECTED = {
    'bounds null shape': (-1, 'implisolid_bounds: bad arguments'),
    'bounds null search': (-1, 'implisolid_bounds: bad arguments'),
    'bounds null out': (-1, 'implisolid_bounds: bad arguments'),
    'bounds depth 2': (-1, 'implisolid_bounds: depth must be in [3, 10]'),
    'bounds depth 11': (-1, 'implisolid_bounds: depth must be in [3, 10]'),
    'bounds reversed box': (-1, 'bounds: the search box must be finite with min < max on every axis'),
    'bounds nan box': (-1, 'bounds: the search box must be finite with min < max on every axis'),
    'bounds truncated shape': (-1, 'JSON parse error: expected , or ]'),
    'bounds unknown type': (-1, 'Invalid object you asked for: "no_such_solid"'),
    'bounds truncated shape, depth 2': (-1, 'implisolid_bounds: depth must be in [3, 10]'),
    'bounds unknown type, reversed box': (-1, 'bounds: the search box must be finite with min < max on every axis'),
    'mass null shape': (-1, 'implisolid_mass: bad arguments'),
    'mass null box': (-1, 'implisolid_mass: bad arguments'),
    'mass null moments': (-1, 'implisolid_mass: bad arguments'),
    'mass depth 2': (-1, 'implisolid_mass: depth must be in [3, 10]'),
    'mass depth 11': (-1, 'implisolid_mass: depth must be in [3, 10]'),
    'mass reversed box': (-1, 'bounds: the search box must be finite with min < max on every axis'),
    'mass nan box': (-1, 'bounds: the search box must be finite with min < max on every axis'),
    'mass truncated shape': (-1, 'JSON parse error: expected , or ]'),
    'mass unknown type': (-1, 'Invalid object you asked for: "no_such_solid"'),
    'mass truncated shape, depth 11': (-1, 'implisolid_mass: depth must be in [3, 10]'),
    'mass unknown type, nan box': (-1, 'bounds: the search box must be finite with min < max on every axis'),
    'slice null shape': (-1, 'implisolid_slice: bad arguments'),
    'slice null rect': (-1, 'implisolid_slice: bad arguments'),
    'slice null z': (-1, 'implisolid_slice: bad arguments'),
    'slice null offsets': (-1, 'implisolid_slice: bad arguments'),
    'slice 0 layers': (-1, 'implisolid_slice: n_layers must be in [1, 65536]'),
    'slice 65537 layers': (-1, 'implisolid_slice: n_layers must be in [1, 65536]'),
    'slice inf z': (-1, 'implisolid_slice: every z must be finite'),
    'slice nan z': (-1, 'implisolid_slice: every z must be finite'),
    'slice resolution 0': (-1, 'slice: resolution must be in [1, 4096]'),
    'slice resolution 4097': (-1, 'slice: resolution must be in [1, 4096]'),
    'slice reversed rect': (-1, 'slice: the rect must be finite with min < max on both axes'),
    'slice truncated shape': (-1, 'JSON parse error: expected , or ]'),
    'slice unknown type': (-1, 'Invalid object you asked for: "no_such_solid"'),
    'slice truncated shape, 0 layers': (-1, 'implisolid_slice: n_layers must be in [1, 65536]'),
    'slice unknown type, resolution 4097': (-1, 'slice: resolution must be in [1, 4096]'),
    'slice truncated shape, nan z': (-1, 'implisolid_slice: every z must be finite'),
    'raster null shape': (-1, 'implisolid_raster: bad arguments'),
    'raster null rect': (-1, 'implisolid_raster: bad arguments'),
    'raster null z': (-1, 'implisolid_raster: bad arguments'),
    'raster null sums': (-1, 'implisolid_raster: bad arguments'),
    'raster 0 layers': (-1, 'implisolid_raster: n_layers must be in [1, 65536]'),
    'raster 65537 layers': (-1, 'implisolid_raster: n_layers must be in [1, 65536]'),
    'raster inf z': (-1, 'implisolid_raster: every z must be finite'),
    'raster nan z': (-1, 'implisolid_raster: every z must be finite'),
    'raster width 0': (-1, 'implisolid_raster: width and height must be in [1, 16384]'),
    'raster width 16385': (-1, 'implisolid_raster: width and height must be in [1, 16384]'),
    'raster height 0': (-1, 'implisolid_raster: width and height must be in [1, 16384]'),
    'raster height 16385': (-1, 'implisolid_raster: width and height must be in [1, 16384]'),
    'raster supersample 3': (-1, 'implisolid_raster: supersample must be 1, 2 or 4'),
    'raster supersample 0': (-1, 'implisolid_raster: supersample must be 1, 2 or 4'),
    'raster reversed rect': (-1, 'raster: the rect must be finite with min < max on both axes'),
    'raster truncated shape': (-1, 'JSON parse error: expected , or ]'),
    'raster unknown type': (-1, 'Invalid object you asked for: "no_such_solid"'),
    'raster truncated shape, supersample 3': (-1, 'implisolid_raster: supersample must be 1, 2 or 4'),
    'raster unknown type, width 0': (-1, 'implisolid_raster: width and height must be in [1, 16384]'),
    'raster truncated shape, 65537 layers': (-1, 'implisolid_raster: n_layers must be in [1, 65536]'),
    'raycast null shape': (-1, 'implisolid_raycast: bad arguments'),
    'raycast null origins': (-1, 'implisolid_raycast: bad arguments'),
    'raycast null dirs': (-1, 'implisolid_raycast: bad arguments'),
    'raycast null hit': (-1, 'implisolid_raycast: bad arguments'),
    'raycast null t': (-1, 'implisolid_raycast: bad arguments'),
    'raycast null f': (-1, 'implisolid_raycast: bad arguments'),
    'raycast n -1': (-1, 'implisolid_raycast: n must be in [0, 2^24]'),
    'raycast n 2^24 + 1': (-1, 'implisolid_raycast: n must be in [0, 2^24]'),
    'raycast steps 0': (-1, 'implisolid_raycast: steps must be in [1, 65536]'),
    'raycast steps 65537': (-1, 'implisolid_raycast: steps must be in [1, 65536]'),
    'raycast bisect -1': (-1, 'implisolid_raycast: bisect must be in [0, 32]'),
    'raycast bisect 33': (-1, 'implisolid_raycast: bisect must be in [0, 32]'),
    'raycast empty range': (-1, 'raycast: the range must be finite with t0 < t1'),
    'raycast nan origin': (-1, 'implisolid_raycast: every origin and direction must be finite'),
    'raycast inf direction': (-1, 'implisolid_raycast: every origin and direction must be finite'),
    'raycast truncated shape': (-1, 'JSON parse error: expected , or ]'),
    'raycast unknown type': (-1, 'Invalid object you asked for: "no_such_solid"'),
    'raycast truncated shape, bisect 33': (-1, 'implisolid_raycast: bisect must be in [0, 32]'),
    'raycast unknown type, steps 0': (-1, 'implisolid_raycast: steps must be in [1, 65536]'),
    'raycast truncated shape, nan origin': (-1, 'implisolid_raycast: every origin and direction must be finite'),
    'raycast unknown type, n -1': (-1, 'implisolid_raycast: n must be in [0, 2^24]'),
    'raycast no rays, truncated shape': (-1, 'JSON parse error: expected , or ]'),
    'raycast no rays, unknown type, null arrays': (-1, 'Invalid object you asked for: "no_such_solid"'),
    'raycast no rays, steps 0': (-1, 'implisolid_raycast: steps must be in [1, 65536]'),
    'intervals null shape': (-1, 'implisolid_debug_intervals: bad arguments'),
    'intervals variant 3': (-1, 'implisolid_debug_intervals: bad arguments'),
    'intervals n -1': (-1, 'implisolid_debug_intervals: bad arguments'),
    'intervals null boxes': (-1, 'implisolid_debug_intervals: bad arguments'),
    'intervals truncated shape': (-1, 'JSON parse error: expected , or ]'),
    'intervals unknown type': (-1, 'Invalid object you asked for: "no_such_solid"'),
    'eval_modes null shape': (-1, 'implisolid_debug_eval_modes: bad arguments'),
    'eval_modes n -1': (-1, 'implisolid_debug_eval_modes: bad arguments'),
    'eval_modes null modes': (-1, 'implisolid_debug_eval_modes: bad arguments'),
    'eval_modes truncated shape': (-1, 'JSON parse error: expected , or ]'),
    'eval_modes unknown type': (-1, 'Invalid object you asked for: "no_such_solid"'),
    'bounds_edges null search': (-1, 'implisolid_bounds_edges: bad arguments'),
    'bounds_edges null edges': (-1, 'implisolid_bounds_edges: bad arguments'),
    'bounds_edges depth 2': (-1, 'bounds: depth must be in [3, 10]'),
    'bounds_edges reversed box': (-1, 'bounds: the search box must be finite with min < max on every axis'),
    'fit_box null bounds': (-1, 'implisolid_fit_box: resolution - 2 margin must be >= 1 (margin >= 0)'),
    'fit_box null out': (-1, 'implisolid_fit_box: resolution - 2 margin must be >= 1 (margin >= 0)'),
    'fit_box resolution 4, margin 2': (-1, 'implisolid_fit_box: resolution - 2 margin must be >= 1 (margin >= 0)'),
    'fit_box margin -1': (-1, 'implisolid_fit_box: resolution - 2 margin must be >= 1 (margin >= 0)'),
    'slice_coords null rect': (-1, 'implisolid_slice_coords: bad arguments'),
    'slice_coords null ys': (-1, 'implisolid_slice_coords: bad arguments'),
    'slice_coords resolution 0': (-1, 'slice: resolution must be in [1, 4096]'),
    'slice_coords nan rect': (-1, 'slice: the rect must be finite with min < max on both axes'),
    'slice_loops null offsets': (-1, 'implisolid_slice_loops: bad arguments'),
    'slice_loops null keys': (-1, 'implisolid_slice_loops: bad arguments'),
    'slice_loops n -1': (-1, 'implisolid_slice_loops: bad arguments'),
    'slice_loops a key starts two segments': (-1, 'implisolid_slice_loops: a key starts two segments or ends two'),
    'raster_coords null rect': (-1, 'implisolid_raster_coords: bad arguments'),
    'raster_coords null my': (-1, 'implisolid_raster_coords: bad arguments'),
    'raster_coords supersample 3': (-1, 'raster: supersample must be 1, 2 or 4'),
    'raster_coords width 0': (-1, 'raster: width must be in [1, 16384]'),
    'ray_params null ts': (-1, 'implisolid_ray_params: bad arguments'),
    'ray_params steps 0': (-1, 'raycast: steps must be in [1, 65536]'),
    'ray_params empty range': (-1, 'raycast: the range must be finite with t0 < t1'),
    'mass_mids null box': (-1, 'implisolid_mass_mids: bad arguments'),
    'mass_mids null mids': (-1, 'implisolid_mass_mids: bad arguments'),
    'mass_mids depth 2': (-1, 'mass: depth must be in [3, 10]'),
    'mass_physical null moments': (-1, 'implisolid_mass_physical: bad arguments'),
    'mass_physical null out': (-1, 'implisolid_mass_physical: bad arguments'),
    'mass_physical depth 11': (-1, 'mass: depth must be in [3, 10]'),
    'mass_physical reversed box': (-1, 'mass: the box must be finite with min < max on every axis'),
    # recorded before the layer entries and the ray entries came to share their request checks
    'raster null rect, 0 layers': (-1, 'implisolid_raster: bad arguments'),
    'raster 0 layers, nan z': (-1, 'implisolid_raster: n_layers must be in [1, 65536]'),
    'raster nan z, width 0': (-1, 'implisolid_raster: every z must be finite'),
    'raster height 0, supersample 3': (-1, 'implisolid_raster: width and height must be in [1, 16384]'),
    'raster supersample 3, reversed rect': (-1, 'implisolid_raster: supersample must be 1, 2 or 4'),
    'raster unknown type, reversed rect': (-1, 'raster: the rect must be finite with min < max on both axes'),
    'islands null shape': (-1, 'implisolid_islands: bad arguments'),
    'islands null rect': (-1, 'implisolid_islands: bad arguments'),
    'islands null z': (-1, 'implisolid_islands: bad arguments'),
    'islands null offsets': (-1, 'implisolid_islands: bad arguments'),
    'islands 0 layers': (-1, 'implisolid_islands: n_layers must be in [1, 65536]'),
    'islands 65537 layers': (-1, 'implisolid_islands: n_layers must be in [1, 65536]'),
    'islands inf z': (-1, 'implisolid_islands: every z must be finite'),
    'islands nan z': (-1, 'implisolid_islands: every z must be finite'),
    'islands width 0': (-1, 'implisolid_islands: width and height must be in [1, 16384]'),
    'islands width 16385': (-1, 'implisolid_islands: width and height must be in [1, 16384]'),
    'islands height 0': (-1, 'implisolid_islands: width and height must be in [1, 16384]'),
    'islands height 16385': (-1, 'implisolid_islands: width and height must be in [1, 16384]'),
    'islands supersample 3': (-1, 'implisolid_islands: supersample must be 1, 2 or 4'),
    'islands supersample 0': (-1, 'implisolid_islands: supersample must be 1, 2 or 4'),
    'islands threshold 0': (-1, 'implisolid_islands: threshold must be in [1, supersample^2]'),
    'islands threshold 5': (-1, 'implisolid_islands: threshold must be in [1, supersample^2]'),
    'islands supersample 1, threshold 2': (-1, 'implisolid_islands: threshold must be in [1, supersample^2]'),
    'islands connectivity 6': (-1, 'implisolid_islands: connectivity must be 4 or 8'),
    'islands reversed rect': (-1, 'raster: the rect must be finite with min < max on both axes'),
    'islands nan rect': (-1, 'raster: the rect must be finite with min < max on both axes'),
    'islands truncated shape': (-1, 'JSON parse error: expected , or ]'),
    'islands unknown type': (-1, 'Invalid object you asked for: "no_such_solid"'),
    'islands null z, 0 layers': (-1, 'implisolid_islands: bad arguments'),
    'islands 0 layers, nan z': (-1, 'implisolid_islands: n_layers must be in [1, 65536]'),
    'islands nan z, width 0': (-1, 'implisolid_islands: every z must be finite'),
    'islands height 16385, supersample 3': (-1, 'implisolid_islands: width and height must be in [1, 16384]'),
    'islands supersample 3, threshold 0': (-1, 'implisolid_islands: supersample must be 1, 2 or 4'),
    'islands supersample 0, connectivity 6': (-1, 'implisolid_islands: supersample must be 1, 2 or 4'),
    'islands threshold 5, connectivity 6': (-1, 'implisolid_islands: threshold must be in [1, supersample^2]'),
    'islands threshold 0, reversed rect': (-1, 'implisolid_islands: threshold must be in [1, supersample^2]'),
    'islands connectivity 6, reversed rect': (-1, 'implisolid_islands: connectivity must be 4 or 8'),
    'islands unknown type, reversed rect': (-1, 'raster: the rect must be finite with min < max on both axes'),
    'islands truncated shape, connectivity 6': (-1, 'implisolid_islands: connectivity must be 4 or 8'),
    'islands truncated shape, threshold 0': (-1, 'implisolid_islands: threshold must be in [1, supersample^2]'),
    'islands unknown type, 65537 layers': (-1, 'implisolid_islands: n_layers must be in [1, 65536]'),
    'distance null shape': (-1, 'implisolid_layer_distance: bad arguments'),
    'distance null rect': (-1, 'implisolid_layer_distance: bad arguments'),
    'distance null z': (-1, 'implisolid_layer_distance: bad arguments'),
    'distance null rec': (-1, 'implisolid_layer_distance: bad arguments'),
    'distance 0 layers': (-1, 'implisolid_layer_distance: n_layers must be in [1, 65536]'),
    'distance 65537 layers': (-1, 'implisolid_layer_distance: n_layers must be in [1, 65536]'),
    'distance inf z': (-1, 'implisolid_layer_distance: every z must be finite'),
    'distance nan z': (-1, 'implisolid_layer_distance: every z must be finite'),
    'distance width 0': (-1, 'implisolid_layer_distance: width and height must be in [1, 16384]'),
    'distance width 16385': (-1, 'implisolid_layer_distance: width and height must be in [1, 16384]'),
    'distance height 0': (-1, 'implisolid_layer_distance: width and height must be in [1, 16384]'),
    'distance height 16385': (-1, 'implisolid_layer_distance: width and height must be in [1, 16384]'),
    'distance supersample 3': (-1, 'implisolid_layer_distance: supersample must be 1, 2 or 4'),
    'distance supersample 0': (-1, 'implisolid_layer_distance: supersample must be 1, 2 or 4'),
    'distance threshold 0': (-1, 'implisolid_layer_distance: threshold must be in [1, supersample^2]'),
    'distance threshold 5': (-1, 'implisolid_layer_distance: threshold must be in [1, supersample^2]'),
    'distance supersample 1, threshold 2': (-1, 'implisolid_layer_distance: threshold must be in [1, supersample^2]'),
    'distance reach2 -1': (-1, 'implisolid_layer_distance: reach2 must be in [0, 2^30)'),
    'distance reversed rect': (-1, 'raster: the rect must be finite with min < max on both axes'),
    'distance nan rect': (-1, 'raster: the rect must be finite with min < max on both axes'),
    'distance truncated shape': (-1, 'JSON parse error: expected , or ]'),
    'distance unknown type': (-1, 'Invalid object you asked for: "no_such_solid"'),
    'distance null z, 0 layers': (-1, 'implisolid_layer_distance: bad arguments'),
    'distance 0 layers, nan z': (-1, 'implisolid_layer_distance: n_layers must be in [1, 65536]'),
    'distance nan z, width 0': (-1, 'implisolid_layer_distance: every z must be finite'),
    'distance height 16385, supersample 3': (-1, 'implisolid_layer_distance: width and height must be in [1, 16384]'),
    'distance supersample 3, threshold 0': (-1, 'implisolid_layer_distance: supersample must be 1, 2 or 4'),
    'distance supersample 0, reach2 -1': (-1, 'implisolid_layer_distance: supersample must be 1, 2 or 4'),
    'distance threshold 5, reach2 -1': (-1, 'implisolid_layer_distance: threshold must be in [1, supersample^2]'),
    'distance threshold 0, reversed rect': (-1, 'implisolid_layer_distance: threshold must be in [1, supersample^2]'),
    'distance reach2 -1, reversed rect': (-1, 'implisolid_layer_distance: reach2 must be in [0, 2^30)'),
    'distance unknown type, reversed rect': (-1, 'raster: the rect must be finite with min < max on both axes'),
    'distance truncated shape, reach2 -1': (-1, 'implisolid_layer_distance: reach2 must be in [0, 2^30)'),
    'distance truncated shape, threshold 0': (-1, 'implisolid_layer_distance: threshold must be in [1, supersample^2]'),
    'distance unknown type, 65537 layers': (-1, 'implisolid_layer_distance: n_layers must be in [1, 65536]'),
    'raycast n -1, bisect 33': (-1, 'implisolid_raycast: n must be in [0, 2^24]'),
    'raycast bisect 33, steps 0': (-1, 'implisolid_raycast: bisect must be in [0, 32]'),
    'raycast steps 0, empty range': (-1, 'implisolid_raycast: steps must be in [1, 65536]'),
    'raycast empty range, nan origin': (-1, 'raycast: the range must be finite with t0 < t1'),
    'ray_spans null shape': (-1, 'implisolid_ray_spans: bad arguments'),
    'ray_spans null origins': (-1, 'implisolid_ray_spans: bad arguments'),
    'ray_spans null dirs': (-1, 'implisolid_ray_spans: bad arguments'),
    'ray_spans null offsets': (-1, 'implisolid_ray_spans: bad arguments'),
    'ray_spans n -1': (-1, 'implisolid_ray_spans: n must be in [0, 2^24]'),
    'ray_spans n 2^24 + 1': (-1, 'implisolid_ray_spans: n must be in [0, 2^24]'),
    'ray_spans bisect -1': (-1, 'implisolid_ray_spans: bisect must be in [0, 32]'),
    'ray_spans bisect 33': (-1, 'implisolid_ray_spans: bisect must be in [0, 32]'),
    'ray_spans steps 0': (-1, 'implisolid_ray_spans: steps must be in [1, 65536]'),
    'ray_spans steps 65537': (-1, 'implisolid_ray_spans: steps must be in [1, 65536]'),
    'ray_spans empty range': (-1, 'raycast: the range must be finite with t0 < t1'),
    'ray_spans nan t1': (-1, 'raycast: the range must be finite with t0 < t1'),
    'ray_spans nan origin': (-1, 'implisolid_ray_spans: every origin and direction must be finite'),
    'ray_spans inf direction': (-1, 'implisolid_ray_spans: every origin and direction must be finite'),
    'ray_spans truncated shape': (-1, 'JSON parse error: expected , or ]'),
    'ray_spans unknown type': (-1, 'Invalid object you asked for: "no_such_solid"'),
    'ray_spans null offsets, n -1': (-1, 'implisolid_ray_spans: bad arguments'),
    'ray_spans n -1, bisect 33': (-1, 'implisolid_ray_spans: n must be in [0, 2^24]'),
    'ray_spans bisect 33, steps 0': (-1, 'implisolid_ray_spans: bisect must be in [0, 32]'),
    'ray_spans steps 0, empty range': (-1, 'implisolid_ray_spans: steps must be in [1, 65536]'),
    'ray_spans steps 0, nan origin': (-1, 'implisolid_ray_spans: steps must be in [1, 65536]'),
    'ray_spans empty range, nan origin': (-1, 'raycast: the range must be finite with t0 < t1'),
    'ray_spans truncated shape, nan origin': (-1, 'implisolid_ray_spans: every origin and direction must be finite'),
    'ray_spans unknown type, empty range': (-1, 'raycast: the range must be finite with t0 < t1'),
    'ray_spans no rays, truncated shape': (-1, 'JSON parse error: expected , or ]'),
    'ray_spans no rays, unknown type, null arrays': (-1, 'Invalid object you asked for: "no_such_solid"'),
    'ray_spans no rays, steps 0': (-1, 'implisolid_ray_spans: steps must be in [1, 65536]'),
    'ray_spans no rays, empty range': (-1, 'raycast: the range must be finite with t0 < t1'),
}


def observe(L, name):
    entry, changed = CASES[name]
    rc = ENTRY[entry](L, **changed)
    return rc, L.implisolid_last_error().decode()


def next_call_works(impli):
    L = impli.lib()
    ts = F(*[9] * 5)
    assert ENTRY["ray_params"](L, ts=ts) == 0 and impli.last_error() == ""
    assert ts.tolist() == [0, 0.25, 0.5, 0.75, 1]
    assert ENTRY["fit_box"](L) == 0 and impli.last_error() == ""


def test_every_case_is_recorded():
    assert set(CASES) == set(EXPECTED)


@pytest.mark.parametrize("name", list(CASES))
def test_refusal(impli, name):
    rc, msg = observe(impli.lib(), name)
    assert (rc, msg) == EXPECTED[name]
    assert rc == -1 and msg, "every case here is a refusal"
    next_call_works(impli)


def test_a_bad_request_wins_over_a_bad_shape(impli):
    # the request is validated before the shape is compiled: both wrong, the request's message
    L = impli.lib()
    for name, (entry, changed) in CASES.items():
        if "shape" not in changed or len(changed) == 1 or changed.get("n") == 0:
            continue
        request_only = {k: v for k, v in changed.items() if k != "shape"}
        assert ENTRY[entry](L, **request_only) == -1
        assert impli.last_error() == EXPECTED[name][1], name
        assert ENTRY[entry](L, shape=changed["shape"]) == -1
        assert impli.last_error() != EXPECTED[name][1], name


def test_raycast_without_rays_compiles_the_shape_and_zeroes_the_stats(impli):
    L = impli.lib()
    stats = np.full(6, 7, np.int64)
    assert ENTRY["raycast"](L, n=0, stats=stats) == 0 and impli.last_error() == ""
    assert stats.tolist() == [0] * 6
    stats[:] = 7
    assert ENTRY["raycast"](L, n=0, origins=None, dirs=None, hit=None, t=None, f=None, normals=None, stats=stats) == 0
    assert impli.last_error() == "" and stats.tolist() == [0] * 6
    assert ENTRY["raycast"](L, n=0, stats=None) == 0 and impli.last_error() == ""
    stats[:] = 7
    rc, msg = observe(L, "raycast no rays, truncated shape")
    assert (rc, msg) == EXPECTED["raycast no rays, truncated shape"]
    assert ENTRY["raycast"](L, n=0, shape=TRUNCATED, stats=stats) == -1 and stats.tolist() == [7] * 6, "stats untouched"
    next_call_works(impli)


def test_ray_spans_without_rays_compiles_the_shape_zeroes_the_stats_and_fills_the_slot(impli):
    L = impli.lib()
    stats, offs = np.full(8, 7, np.int64), np.full(1, 7, np.int64)
    assert ENTRY["ray_spans"](L, n=0, origins=None, dirs=None, offsets=offs, stats=stats) == 0 and impli.last_error() == ""
    assert stats.tolist() == [0] * 8 and offs.tolist() == [0]
    assert L.implisolid_ray_spans_copy(None, None, None, None) == 0, "an empty result is a result"
    stats[:], offs[:] = 7, 7
    assert ENTRY["ray_spans"](L, n=0, shape=TRUNCATED, offsets=offs, stats=stats) == -1
    assert stats.tolist() == [7] * 8 and offs.tolist() == [7], "stats and offsets untouched"
    assert L.implisolid_ray_spans_copy(None, None, None, None) == -1, "and the slot is empty"
    next_call_works(impli)


SLICE_COPY = (-1, "implisolid_slice_copy: no slice to copy (the last implisolid_slice failed, or none ran)")


@pytest.mark.parametrize("name", [n for n, (e, _) in CASES.items() if e == "slice"])
def test_no_slice_to_copy_after_a_refused_slice(impli, name):
    L = impli.lib()
    assert observe(L, name)[0] == -1
    assert (ENTRY["slice_copy"](L), impli.last_error()) == SLICE_COPY
    assert (ENTRY["slice_copy"](L, xy=None, keys=None), impli.last_error()) == SLICE_COPY
    next_call_works(impli)


# ---- the result slots and the pass timers ---------------------------------------------------------------------------
# What the four copy entries and the six timer entries answer, recorded from the library before the queries came
# to share their result slot and their pass timer: in a process that has run no query, and after a refused one.
ENTRY["runs"] = Args("implisolid_layer_runs", shape=SPHERE, irm=0, rect=RECT, width=8, height=8, supersample=2, z=Z2, n_layers=2,
                     threshold=0, offsets=i64(3), sums=i64(2), stats=i64(7))
COPY = {
    "slice": Args("implisolid_slice_copy", xy=F(*[0] * 4), keys=np.zeros(2, np.uint32)),
    "islands": Args("implisolid_islands_copy", comps=np.zeros(8, np.int32)),
    "runs": Args("implisolid_layer_runs_copy", start=np.zeros(1, np.uint32), value=np.zeros(1, np.uint8)),
    "ray_spans": Args("implisolid_ray_spans_copy", k=np.zeros(2, np.int32), t=F(0, 0), f=F(0, 0), normals=F(*[0] * 6)),
}
NOTHING_TO_COPY = {
    "slice": SLICE_COPY,
    "islands": (-1, "implisolid_islands_copy: no records to copy (the last implisolid_islands failed, or none ran)"),
    "runs": (-1, "implisolid_layer_runs_copy: no runs to copy (the last implisolid_layer_runs failed, or none ran)"),
    "ray_spans": (-1, "implisolid_ray_spans_copy: no spans to copy (the last implisolid_ray_spans failed, or none ran)"),
}
REFUSED = {"slice": dict(n_layers=0), "islands": dict(connectivity=6), "runs": dict(threshold=5), "ray_spans": dict(steps=0)}


def _copies(L, last_error):
    """each copy entry's answer with its valid pointers, then with null ones"""
    out = {}
    for name, copy in COPY.items():
        with_pointers = (copy(L), last_error())
        out[name] = [with_pointers, (copy(L, **{k: None for k in copy.valid}), last_error())]
    return out


def test_before_any_query_the_timers_read_minus_one_and_nothing_is_there_to_copy():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import json, sys; sys.path.insert(0, 'tests'); import implisolid_amd as I, test_cpu_query_refusals as t; L = I.lib(); "
            "ms = [I.debug_bounds_ms(False), I.islands_kernel_ms(False), I.layer_distance_kernel_ms(False), "
            "I.layer_runs_kernel_ms(False), I.raycast_kernel_ms(False), I.ray_spans_kernel_ms(False)]; "
            "print('RESULT', json.dumps([ms, t._copies(L, I.last_error)]))")
    out = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True, timeout=120)
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
    assert len(lines) == 1, (out.stdout, out.stderr)
    ms, copies = json.loads(lines[0][len("RESULT "):])
    # bounds (one figure, returned), islands, layer distance, layer runs, raycast, ray spans
    assert ms == [-1.0] + [[-1.0] * n for n in (5, 3, 3, 2, 3)]
    for name, want in NOTHING_TO_COPY.items():
        assert [tuple(c) for c in copies[name]] == [want, want], name


@pytest.mark.parametrize("name", list(REFUSED))
def test_nothing_to_copy_after_a_refused_query(impli, name):
    L = impli.lib()
    assert ENTRY[name](L, **REFUSED[name]) == -1 and impli.last_error()
    assert _copies(L, impli.last_error)[name] == [NOTHING_TO_COPY[name]] * 2
    next_call_works(impli)
