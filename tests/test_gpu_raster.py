"""Layer images of a solid (implisolid_raster) on the GPU.

The reference is tests/np_raster.py's restatement of the definition on field values that do not come
from the raster kernels: the oracle's (eval_implicit) at the sample points, or ImplicitService.eval /
np_sdf3d.evaluate for the sdf_3d shapes, which the oracle does not have.  Coverage bytes and layer sums
are integers and must equal it exactly, whatever the pruning level skips or fills and however the
layers are chunked.  40 x 40 gives tiles of 16, 16 and 8 pixels; 33 x 17 gives border tiles one pixel
wide and one pixel high, an image pitch (48) that is not the width, and a width that is no multiple
of 4.
"""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_raster   # noqa: E402
import np_sdf3d   # noqa: E402
import test_gpu_mass as gm   # noqa: E402  (its shapes and boxes; its tests are not collected from here)

pytestmark = pytest.mark.gpu

EYE = gm.EYE
SHAPES, NAMES = gm.SHAPES, gm.NAMES
RECTS = {"unit": gm.UNIT[:4], "non_dyadic": gm.NON_DYADIC[:4]}
GRIDS = [(40, 40, 1), (40, 40, 2), (33, 17, 4)]
# a plane that misses every shape, a repeated plane and an unsorted order; the shapes sit around z = -0.3 .. 0
Z = np.array([-0.9, -0.3, 0.05, -0.3, -0.125, -0.55], np.float32)

_REF = {}


def _field(impli, oracle, name, shape, pts, ignore_root_matrix=False):
    if name == "sdf3d":
        with impli.ImplicitService(shape) as svc:
            return np.asarray(svc.eval(pts), np.float32)
    return np.asarray(oracle.eval_implicit(oracle.mp5_to_nodes(json.dumps(shape), ignore_root_matrix), pts), np.float32)


def _ref(impli, oracle, name, shape, rect, W, H, s, z=Z, ignore_root_matrix=False):
    """np_raster.coverage of the independent field values; computed once per case"""
    key = (name, tuple(rect), W, H, s, tuple(float(v) for v in z), ignore_root_matrix)
    if key not in _REF:
        mx, my = np_raster.coords(rect, W, H, s)
        F = _field(impli, oracle, name, shape, np_raster.points(mx, my, z), ignore_root_matrix)
        _REF[key] = np_raster.coverage(F.reshape(len(z), H * s, W * s), s)
    return _REF[key]


def _at_level(impli, level, *a, **kw):
    impli.set_pruning(level)
    try:
        return impli.raster_layers(*a, return_stats=True, **kw)
    finally:
        impli.set_pruning(2)


def _check_bits(got, want, W, H, s):
    cov, sums, stats = got
    rc, rs = want
    assert cov.dtype == np.uint8 and cov.shape == rc.shape == (len(rs), H, W) and sums.dtype == np.int64 and sums.shape == rs.shape
    bad = np.argwhere(cov != rc)
    assert len(bad) == 0, ("first differing [l, py, px]", bad[:5].tolist(), len(bad))
    assert np.array_equal(sums, rs), (sums.tolist(), rs.tolist())
    assert int(cov.max()) <= s * s and np.array_equal(cov.reshape(len(rs), -1).sum(axis=1, dtype=np.int64), sums)
    ntx, nty = (W + 15) // 16, (H + 15) // 16
    assert stats[0] == len(rs) * ntx * nty and stats[1] + stats[2] <= stats[0] and stats[3] <= stats[1] * 256 * s * s


def test_the_deep_tree_runs_the_16_slot_stacks(impli):
    assert impli.program_info(SHAPES["tree_deep"])[1] > 12
    assert impli.program_info(SHAPES["csg"])[1] <= 12, "and the others the smaller ones"


@pytest.mark.parametrize("level", [0, 2])
@pytest.mark.parametrize("rect", sorted(RECTS))
@pytest.mark.parametrize("W, H, s", GRIDS)
@pytest.mark.parametrize("name", NAMES)
def test_images_equal_the_restatement(impli, oracle, name, W, H, s, rect, level):
    want = _ref(impli, oracle, name, SHAPES[name], RECTS[rect], W, H, s)
    got = _at_level(impli, level, SHAPES[name], RECTS[rect], W, H, Z, s)
    print(name, (W, H, s), rect, level, "sums", got[1].tolist(), "stats", got[2])
    assert 0 < want[1].sum() < len(Z) * W * H * s * s, "the case holds solid and empty samples"
    _check_bits(got, want, W, H, s)
    assert got[2][4] == 1
    if level == 0:
        assert got[2][1] == got[2][0] and got[2][2] == 0 and got[2][3] == len(Z) * W * H * s * s
    # the repeated plane repeats its image
    assert np.array_equal(got[0][1], got[0][3]) and got[1][1] == got[1][3]


@pytest.mark.parametrize("H", [1, 15, 16, 17])
@pytest.mark.parametrize("W", [1, 15, 16, 17])
def test_tile_edges(impli, oracle, W, H):
    z = Z[1:3]
    want = _ref(impli, oracle, "csg", SHAPES["csg"], RECTS["unit"], W, H, 2, z)
    for level in (0, 2):
        got = _at_level(impli, level, SHAPES["csg"], RECTS["unit"], W, H, z, 2)
        _check_bits(got, want, W, H, 2)


# ---- -0.0 is solid ------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [0, 2])
@pytest.mark.parametrize("W, s", [(32, 1), (16, 2)])
def test_negative_zero_samples_are_solid(impli, W, s, level):
    # gm.zero_node(): the table's nodes are the samples of +-1 at 32 per axis, its +0.0 entries give -0.0
    # there (asserted without a GPU in test_cpu_raster.py)
    node, zeros = gm.zero_node()
    mx, my = np_raster.coords(RECTS["unit"], W, W, s)
    z = mx if s == 1 else np_raster.coords(RECTS["unit"], 32, 32, 1)[0]
    F = np_sdf3d.evaluate(node, *np_raster.points(mx, my, z).T).reshape(32, 32, 32)
    assert np.array_equal(F == 0, zeros) and zeros.sum() >= 100 and np.signbit(F[zeros]).all()
    want = np_raster.coverage(F, s)
    got = _at_level(impli, level, node, RECTS["unit"], W, W, z, s)
    print("level", level, "solid samples", int(got[1].sum()), "of which -0.0", int(zeros.sum()), "stats", got[2])
    _check_bits(got, want, W, W, s)
    assert int(got[1].sum()) == int((F > 0).sum() + zeros.sum()), "every -0.0 sample is counted"


# ---- the fill path and the empty path --------------------------------------------------------------------
@pytest.mark.parametrize("W, H, s", GRIDS)
def test_a_solid_rect_is_filled_without_a_sample(impli, W, H, s):
    cov, sums, stats = impli.raster_layers(gm.BIG, RECTS["unit"], W, H, Z, s, return_stats=True)
    print("stats", stats)
    assert cov.shape == (len(Z), H, W) and (cov == s * s).all() and (sums == W * H * s * s).all()
    assert stats[1] == 0 and stats[3] == 0 and stats[2] == stats[0] == len(Z) * ((W + 15) // 16) * ((H + 15) // 16)


@pytest.mark.parametrize("W, H, s", GRIDS)
def test_an_empty_rect_gives_zeros(impli, W, H, s):
    cov, sums, stats = impli.raster_layers(gm.AWAY, RECTS["unit"], W, H, Z, s, return_stats=True)
    # every work figure is zero: tiles evaluated, tiles filled, samples ([4] counts the chunk the layers went through)
    assert (cov == 0).all() and (sums == 0).all() and stats[1:4] == [0, 0, 0] and stats[0] > 0 and stats[4] == 1


# ---- pruning does work --------------------------------------------------------------------------------------
def test_pruning_fills_and_skips_tiles_on_a_sphere(impli, oracle):
    W = 128
    mx, my = np_raster.coords(RECTS["unit"], W, W, 1)

    def tile_box(tx, ty):
        return [mx[16 * tx], mx[16 * tx + 15], my[16 * ty], my[16 * ty + 15], 0, 0]
    iv, _ = impli.debug_intervals(gm.SPHERE, [tile_box(4, 4), tile_box(0, 0)])
    print("central tile", iv[0].tolist(), "corner tile", iv[1].tolist())
    assert iv[0][0] >= 0, "the evaluator proves the central tile solid"
    assert iv[1][1] < 0, "and the corner tile outside"
    z = np.zeros(1, np.float32)
    want = _ref(impli, oracle, "sphere", gm.SPHERE, RECTS["unit"], W, W, 1, z)
    got0 = _at_level(impli, 0, gm.SPHERE, RECTS["unit"], W, W, z, 1)
    got2 = _at_level(impli, 2, gm.SPHERE, RECTS["unit"], W, W, z, 1)
    print("level 0", got0[2], "level 2", got2[2])
    _check_bits(got0, want, W, W, 1)
    _check_bits(got2, want, W, W, 1)
    pairs = 64
    assert got0[2][:4] == [pairs, pairs, 0, W * W]
    assert got2[2][0] == pairs and got2[2][2] > 0 and 0 < got2[2][1] < pairs
    assert np.array_equal(got0[0], got2[0]) and np.array_equal(got0[1], got2[1])
    # the disc's area, within the pixels its outline can cross: a ring one pixel diagonal wide
    h = 2.0 / W
    assert abs(int(got2[1][0]) * h * h - np.pi * 0.25) <= 2 * np.pi * 0.5 * np.sqrt(2.0) * h


@pytest.mark.parametrize("s", [1, 2])
def test_pruned_tiles_of_a_tree_of_more_than_sixteen_csg_nodes(impli, oracle, s):
    # the comb (tests/run_inputs.py) has 33 Unions: the modes of the nodes 16 .. 31 stand in the high half of a
    # listed tile's modes word, and in its tiles node 15 keeps its right operand, which sets the low half's bit 31
    import run_inputs as ri
    W, H, z = ri.COMB_W, ri.COMB_H, ri.COMB_Z
    want = _ref(impli, oracle, "comb", ri.COMB, ri.COMB_RECT, W, H, s, z)
    solid_tiles = int((np.pad(want[0], ((0, 0), (0, 0), (0, 1040 - W))).reshape(len(z), H, 65, 16).max(axis=(1, 3)) > 0).sum())
    for level in (0, 1, 2):
        got = _at_level(impli, level, ri.COMB, ri.COMB_RECT, W, H, z, s)
        print("comb", s, level, got[2])
        _check_bits(got, want, W, H, s)
        # a bound may list more tiles than hold a solid sample, never fewer; most of the image is empty
        assert got[2][0] == 130 and (got[2][1] == 130 if level == 0 else solid_tiles <= got[2][1] + got[2][2] < 130), (solid_tiles, got[2])


# ---- the mass sums: two independent kernel families ----------------------------------------------------------
@pytest.mark.parametrize("box", sorted(gm.BOXES))
@pytest.mark.parametrize("name", NAMES)
def test_layer_sums_equal_the_mass_layer_cells(impli, name, box):
    b = gm.BOXES[box]
    z = impli.mass_mids(b, 5)[2]
    mom, layers = impli.mass_moments(SHAPES[name], b, 5)
    assert layers.sum() > 0
    cov1, sums1 = impli.raster_layers(SHAPES[name], b[:4], 32, 32, z, 1)
    cov2, sums2 = impli.raster_layers(SHAPES[name], b[:4], 16, 16, z, 2)
    print(name, box, "layer cells", layers.tolist())
    assert np.array_equal(sums1, layers), (sums1.tolist(), layers.tolist())
    assert np.array_equal(sums2, layers), (sums2.tolist(), layers.tolist())
    # the 2 x 2 sums of the one-sample image are the two-sample image
    assert np.array_equal(cov1.reshape(32, 16, 2, 16, 2).sum(axis=(2, 4)), cov2)


# ---- chunks, cov = NULL, reruns ------------------------------------------------------------------------------
Z12 = np.concatenate([Z, Z[::-1] + np.float32(0.03125)]).astype(np.float32)


@pytest.mark.parametrize("name", ["egg", "tree_deep"])
def test_three_chunks_give_the_same_bits(impli, oracle, name, monkeypatch):
    want = _ref(impli, oracle, name, SHAPES[name], RECTS["non_dyadic"], 40, 40, 2, Z12)
    one = impli.raster_layers(SHAPES[name], RECTS["non_dyadic"], 40, 40, Z12, 2, return_stats=True)
    monkeypatch.setenv("IMPLISOLID_RASTER_CHUNK", "36")   # four layers of nine tiles
    got = impli.raster_layers(SHAPES[name], RECTS["non_dyadic"], 40, 40, Z12, 2, return_stats=True)
    monkeypatch.setenv("IMPLISOLID_RASTER_CHUNK", "1")    # below one layer's tiles: a layer per chunk
    each = impli.raster_layers(SHAPES[name], RECTS["non_dyadic"], 40, 40, Z12, 2, return_stats=True)
    monkeypatch.delenv("IMPLISOLID_RASTER_CHUNK")
    assert one[2][4] == 1 and got[2][4] == 3 and each[2][4] == 12
    for r in (one, got, each):
        _check_bits(r, want, 40, 40, 2)
        assert r[2][:4] == one[2][:4]


@pytest.mark.parametrize("chunk", [None, "36"])
def test_without_an_image_the_sums_are_the_same(impli, oracle, chunk, monkeypatch):
    want = _ref(impli, oracle, "csg", SHAPES["csg"], RECTS["unit"], 40, 40, 2, Z12)
    if chunk:
        monkeypatch.setenv("IMPLISOLID_RASTER_CHUNK", chunk)
    cov, sums, stats = impli.raster_layers(SHAPES["csg"], RECTS["unit"], 40, 40, Z12, 2, return_stats=True, want_cov=False)
    full = impli.raster_layers(SHAPES["csg"], RECTS["unit"], 40, 40, Z12, 2, return_stats=True)
    assert cov is None and np.array_equal(sums, want[1]) and stats == full[2] and stats[4] == (3 if chunk else 1)
    _check_bits(full, want, 40, 40, 2)


def test_two_calls_give_identical_bits(impli):
    a = impli.raster_layers(SHAPES["tree_deep"], RECTS["non_dyadic"], 33, 17, Z, 4, return_stats=True)
    # another shape and size in between: nothing of it may stay behind in the scratch
    impli.raster_layers(gm.BIG, RECTS["unit"], 40, 40, Z12, 1)
    b = impli.raster_layers(SHAPES["tree_deep"], RECTS["non_dyadic"], 33, 17, Z, 4, return_stats=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


@pytest.mark.parametrize("level", [0, 2])
def test_ignore_root_matrix(impli, oracle, level):
    shape = SHAPES["csg"]
    moved = dict(shape, matrix=[1, 0, 0, 0.3, 0, 1, 0, -0.2, 0, 0, 1, 0.1])
    want = _ref(impli, oracle, "csg_ignored", moved, RECTS["unit"], 40, 40, 2, Z, True)
    plain = _ref(impli, oracle, "csg", shape, RECTS["unit"], 40, 40, 2)
    kept = _ref(impli, oracle, "csg_moved", moved, RECTS["unit"], 40, 40, 2)
    assert np.array_equal(want[0], plain[0]) and not np.array_equal(kept[0], plain[0]), "the root matrix moves the solid"
    _check_bits(_at_level(impli, level, moved, RECTS["unit"], 40, 40, Z, 2, ignore_root_matrix=True), want, 40, 40, 2)
    _check_bits(_at_level(impli, level, moved, RECTS["unit"], 40, 40, Z, 2), kept, 40, 40, 2)


# ---- errors ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(W=0), dict(H=16385), dict(s=3), dict(z=[]), dict(z=[0.0, np.nan]), dict(rect=[1, -1, -1, 1]),
                                dict(rect=[-1, 1, -np.inf, 1]), dict(shape={"type": "rawjscode", "matrix": EYE})])
def test_bad_input_is_an_error(impli, kw):
    with pytest.raises(impli.ImplisolidError) as e:
        impli.raster_layers(kw.get("shape", SHAPES["egg"]), kw.get("rect", RECTS["unit"]), kw.get("W", 40), kw.get("H", 40),
                            kw.get("z", Z), kw.get("s", 2))
    assert str(e.value), "with a message"
    assert impli.raster_layers(SHAPES["egg"], RECTS["unit"], 40, 40, Z, 2)[1].sum() > 0, "and the next call works"
