"""GPU: per-vertex normals from object streams (the "normals" settings key on implisolid_batch_*,
merged launches and per-object graphs) against the reference rule mcc2.cpp:852-871 applied to the
oracle's gradients (np_normals.normals_ref) -- bit for bit, every row, NaN rows by position; R = 24
on the +-1 box."""
import json
import os

import numpy as np
import pytest

from np_normals import normals_ref, same_bits
from test_gpu_normals import _general_matrix_tree
from test_gpu_parity import TREES, _depth_class_objects

pytestmark = pytest.mark.gpu

R = 24


def _mc():
    from implisolid_amd import scenes
    return scenes.mc_settings(R, 1.0)


def _far():   # outside the box: no vertex
    from implisolid_amd import scenes
    return {"type": "iellipsoid", "matrix": scenes.st(0.25, 3.0, 0, 0)}


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _stream_objects():
    """Deep (its own depth class: the last row of the merged batch, though the caller's object 0),
    then shallow objects with the two empty ones between and after them."""
    from implisolid_amd import scenes
    deep = _depth_class_objects()[3]   # the 14-deep chain: 15 stack slots, the 16-slot class
    assert scenes.tree_stats(deep)[2] + 1 > 12
    return [deep, TREES["sphere"], TREES["intersection"], TREES["twist_tbb"], TREES["extrusion_tri"],
            _general_matrix_tree(), _far()]


_REF = {}


def _reference(oracle, shape):
    """(verts, faces, normals, -42 rows) of one object at R, computed once per object and shared."""
    key = json.dumps(shape, sort_keys=True)
    if key not in _REF:
        tree = oracle.mp5_to_nodes(json.dumps(shape))
        v, f = oracle.marching_cubes(tree, R, [-1, 1] * 3)
        n, bad = normals_ref(oracle, tree, v)
        for a in (v, f, n):
            a.setflags(write=False)
        _REF[key] = (v, f, n, bad)
    return _REF[key]


def _check_object(b, i, shape, oracle, plain=None, tag=None):
    vr, fr, nr, bad = _reference(oracle, shape)
    v, f, n = b.download(i, normals=True)
    assert np.array_equal(f, fr) and np.array_equal(_u32(v), _u32(vr)), (tag, i)
    if plain is not None:   # the mesh of the same batch created without the key
        assert np.array_equal(f, plain[1]) and np.array_equal(_u32(v), _u32(plain[0])), (tag, i)
    assert n.shape == v.shape and n.dtype == np.float32, (tag, i)
    assert same_bits(n, nr), (tag, i, np.flatnonzero((_u32(n) != _u32(nr)).any(1))[:10])
    n2, problems = b.normals(i, return_problems=True)
    assert same_bits(n2, n) and problems == bad, (tag, i, problems, bad)
    return v, n


@pytest.mark.parametrize("n_streams", [0, 2])
def test_batch_normals_match_reference(impli, oracle, n_streams):
    shapes, mc = _stream_objects(), _mc()
    before = json.dumps(mc, sort_keys=True)
    with impli.Batch(shapes, mc, n_streams=n_streams) as b0:
        assert not b0.has_normals
        b0.run()
        plain = [b0.download(i) for i in range(len(shapes))]
    with impli.Batch(shapes, mc, n_streams=n_streams, normals=True) as b:
        assert json.dumps(mc, sort_keys=True) == before
        assert b.has_normals and b.n == len(shapes) and b.merged == (n_streams == 0)
        counts = []
        for rep in range(2):   # the second run: the same normals, and problem counts that did not accumulate
            b.run()
            for i, sh in enumerate(shapes):
                v, n = _check_object(b, i, sh, oracle, plain[i], rep)
                if rep == 0:
                    counts.append(len(v))
                    # ... and the normals build_geometry gives the same object
                    n1 = impli.make_geometry(sh, mc, normals=True)[2]
                    assert same_bits(n, n1), i
    # no wave of the merged pass may straddle objects: partial last waves, non-empty neighbours, and
    # empty objects between and behind them
    assert any(c % 64 for c in counts), counts
    assert any(a > 0 and c > 0 for a, c in zip(counts, counts[1:])), counts
    assert counts[2] == 0 and counts[-1] == 0 and counts[0] > 0, counts


def test_batch_normals_direct_launches(impli, oracle):
    shapes, mc = [TREES["twist_tbb"], _far(), TREES["union_sphere_cube"]], _mc()
    old = os.environ.get("IMPLISOLID_NO_GRAPH")
    os.environ["IMPLISOLID_NO_GRAPH"] = "1"
    try:
        b = impli.Batch(shapes, mc, n_streams=2, normals=True)
    finally:
        if old is None:
            del os.environ["IMPLISOLID_NO_GRAPH"]
        else:
            os.environ["IMPLISOLID_NO_GRAPH"] = old
    with b:
        assert b.graphs is False and b.has_normals and not b.merged
        for rep in range(2):
            b.run()
            for i, sh in enumerate(shapes):
                _check_object(b, i, sh, oracle, tag=rep)


@pytest.mark.parametrize("n_streams", [0, 2])
def test_batch_without_key_has_no_normals(impli, oracle, n_streams):
    shapes, mc = [TREES["sphere"], TREES["difference"]], _mc()
    with impli.Batch(shapes, mc, n_streams=n_streams, normals=True) as b:   # one with the key, closed just before
        b.run()
        assert b.has_normals
    for settings in (mc, dict(mc, normals={"enabled": True})):   # true is no int: the default, off
        with impli.Batch(shapes, settings, n_streams=n_streams) as b:
            b.run()
            assert b.has_normals is False
            with pytest.raises(impli.ImplisolidError, match="normals"):
                b.normals(0)
            with pytest.raises(impli.ImplisolidError, match="normals"):
                b.download(0, normals=True)
            L = impli.lib()
            assert L.implisolid_batch_download_normals(b.h, 0, None, None) == -1 and '"normals"' in impli.last_error()
            for i, sh in enumerate(shapes):
                vr, fr, _, _ = _reference(oracle, sh)
                v, f = b.download(i)
                assert np.array_equal(f, fr) and np.array_equal(_u32(v), _u32(vr)), i
    with impli.Batch(shapes, mc, n_streams=n_streams, normals=True) as b:   # a bad index is an error too
        b.run()
        with pytest.raises(impli.ImplisolidError, match="bad index"):
            b.normals(len(shapes))


def _sphere_lattice(k, r):
    """k^3 spheres of radius r on a lattice filling the box, under a balanced tree of unions."""
    from implisolid_amd import scenes
    step = 2.0 / k
    nodes = [{"type": "iellipsoid", "matrix": scenes.st(2 * r, -1 + step * (i + 0.5), -1 + step * (j + 0.5), -1 + step * (l + 0.5))}
             for i in range(k) for j in range(k) for l in range(k)]
    while len(nodes) > 1:
        nodes = [{"type": "Union", "matrix": list(scenes.EYE), "children": nodes[a:a + 2]} if a + 1 < len(nodes) else nodes[a]
                 for a in range(0, len(nodes), 2)]
    return nodes[0]


def test_batch_normals_after_capacity_growth(impli, oracle):
    """A fresh engine's vertex buffer holds 6 (R + 2)^2 + 1 vertices rounded up to 1024 2^k
    (Engine::set_slab): 4096 at R = 24, where the largest mesh of TREES (leaf_cube) has 3494 vertices
    and fits, as does every other object of the existing suites.  A 3 x 3 x 3 lattice of spheres of
    radius 0.26 (two cells apart) has more than 4400 there and more than the 8192 faces, so the merged
    create's first pass finds that it does not fit, grows the buffers -- the normals with the
    vertices -- re-uploads the rows and runs again.  (Lattices of this kind outgrow the buffers at
    lower resolutions too -- 27 spheres of radius 0.32 from R = 10 on -- but R = 24 is this suite's
    resolution.)  Beside it an object that fits, on either side.

    The lattice's mesh is compared with the same batch created without the key, not with the oracle:
    the library's mesh of this object (4460 vertices, 8816 faces, the same from build_geometry, the
    merged stream and the per-object graphs, and the same before this feature) is not the oracle's
    (4698 / 9288).  That difference is the marching cubes' and older than the normals; the normals
    are checked against the reference rule at the vertices the stream returned."""
    lattice = _sphere_lattice(3, 0.26)
    shapes, mc = [TREES["sphere"], lattice, TREES["leaf_itorus"]], _mc()
    cap = 1024
    while cap < 6 * (R + 2) ** 2 + 1:
        cap *= 2
    assert cap > len(_reference(oracle, TREES["leaf_cube"])[0]) + 1
    with impli.Batch(shapes, mc, n_streams=0) as b0:
        b0.run()
        plain = [b0.download(i) for i in range(len(shapes))]
    assert len(plain[1][0]) + 1 > cap and len(plain[1][0]) % 64 != 0
    tree = oracle.mp5_to_nodes(json.dumps(lattice))
    with impli.Batch(shapes, mc, n_streams=0, normals=True) as b:
        assert b.merged and b.has_normals
        for rep in range(2):
            b.run()
            for i in (0, 2):
                _check_object(b, i, shapes[i], oracle, plain[i], rep)
            v, f, n = b.download(1, normals=True)
            assert np.array_equal(f, plain[1][1]) and np.array_equal(_u32(v), _u32(plain[1][0])), rep
            ref, bad = normals_ref(oracle, tree, v)
            assert same_bits(n, ref), (rep, np.flatnonzero((_u32(n) != _u32(ref)).any(1))[:10])
            assert b.normals(1, return_problems=True)[1] == bad, rep


def test_batch_create_destroy_keeps_pool_flat(impli, oracle):
    """Creating and closing the same merged batch with the key returns every device block it took
    (the engines' normals buffers and the batch's own blocks): the device memory in use after the 20th
    round is that after the 2nd.  The batch's deepest object has 10 stack slots, so its deep class runs
    the 12-slot kernels: checked once against the reference, on the first round."""
    import torch
    shapes, mc = [TREES["sphere"], _depth_class_objects()[1], TREES["intersection"], TREES["lid"]], _mc()
    used = []
    for rep in range(20):
        with impli.Batch(shapes, mc, n_streams=0, normals=True) as b:
            b.run()
            if rep == 0:
                for i, sh in enumerate(shapes):
                    _check_object(b, i, sh, oracle)
            else:
                b.counts(0)
        torch.cuda.synchronize()
        free, total = torch.cuda.mem_get_info()
        used.append(total - free)
    assert used[19] == used[1], used
