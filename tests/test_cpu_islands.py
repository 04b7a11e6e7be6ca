"""Host side of the islands query (implisolid_islands' argument checks, implisolid_islands_copy, islands_of),
the restatement tests/np_islands.py against a plain flood fill, and the preconditions of the cases of
test_gpu_islands.py.  No GPU."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import island_inputs as ii   # noqa: E402
import np_islands   # noqa: E402
import np_raster   # noqa: E402
import np_sdf3d   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE = ii.EYE


def st(k, x, y, z):
    return [k, 0, 0, x, 0, k, 0, y, 0, 0, k, z]


# two spheres of radius 0.25 stacked on the z axis (centres -0.4 and 0.2, a gap between z = -0.15 and -0.05)
# and one of radius 0.09 beside the lower one, which only the plane z = -0.4 meets.  The planes: three through the lower sphere, one in the gap,
# then the upper sphere's lowest plane -- an island, the layer before it is empty -- and two it rests on
PAIR = {"type": "Union", "matrix": EYE, "children": [
    {"type": "iellipsoid", "matrix": st(0.5, 0, 0, -0.4)}, {"type": "iellipsoid", "matrix": st(0.5, 0, 0, 0.2)},
    {"type": "iellipsoid", "matrix": st(0.18, 0.6, 0.6, -0.4)}]}
PAIR_Z = np.array([-0.5, -0.4, -0.3, -0.1, -0.04, 0.1, 0.2], np.float32)
UNIT = [-1, 1, -1, 1]


def flood(solid, connectivity):
    """labels by a plain flood fill in increasing pixel order: the first pixel reached is the seed"""
    L, H, W = solid.shape
    lab = np.full(solid.shape, -1, np.int32)
    st8 = np_islands.steps(connectivity)
    for l in range(L):
        for p in range(H * W):
            y, x = divmod(p, W)
            if not solid[l, y, x] or lab[l, y, x] >= 0:
                continue
            lab[l, y, x] = p
            todo = [(y, x)]
            while todo:
                cy, cx = todo.pop()
                for dy, dx in st8:
                    ny, nx = cy + dy, cx + dx
                    if 0 <= ny < H and 0 <= nx < W and solid[l, ny, nx] and lab[l, ny, nx] < 0:
                        lab[l, ny, nx] = p
                        todo.append((ny, nx))
    return lab


def flood_records(solid, lab):
    L, H, W = solid.shape
    offs, rows = [0], []
    for l in range(L):
        acc = {}
        for y in range(H):
            for x in range(W):
                s = int(lab[l, y, x])
                if s < 0:
                    continue
                r = acc.setdefault(s, [s, 0, 0, x, y, x, y, l])
                r[1] += 1
                r[2] += 1 if l == 0 or solid[l - 1, y, x] else 0
                r[3], r[4], r[5], r[6] = min(r[3], x), min(r[4], y), max(r[5], x), max(r[6], y)
        rows += [acc[s] for s in sorted(acc)]
        offs.append(len(rows))
    return np.array(offs, np.int64), np.array(rows, np.int32).reshape(-1, 8)


_REST = {}


def restated(name, connectivity):
    key = (name, connectivity)
    if key not in _REST:
        bits = ii.PAINTED[name]()
        _REST[key] = (bits,) + np_islands.islands(bits.astype(np.uint8), 1, connectivity)
    return _REST[key]


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", sorted(ii.PAINTED))
def test_the_restatement_equals_a_flood_fill(name, connectivity):
    bits, offs, comps, lab = restated(name, connectivity)
    want = flood(bits, connectivity)
    assert np.array_equal(lab, want)
    fo, fc = flood_records(bits, want)
    assert np.array_equal(offs, fo) and np.array_equal(comps, fc)
    assert comps[:, 1].sum() == bits.sum() and (comps[:, 2] <= comps[:, 1]).all()


@pytest.mark.parametrize("connectivity", [4, 8])
def test_the_restatement_equals_a_flood_fill_at_the_tile_sizes(connectivity):
    for W in ii.SIZES:
        for H in ii.SIZES:
            bits = ii.sized(W, H)
            offs, comps, lab = np_islands.islands(bits.astype(np.uint8), 1, connectivity)
            want = flood(bits, connectivity)
            assert np.array_equal(lab, want), (W, H)
            fo, fc = flood_records(bits, want)
            assert np.array_equal(offs, fo) and np.array_equal(comps, fc), (W, H)
            assert bits.any() and not bits.all()


def test_a_threshold_selects_the_pixels():
    cov = np.array([[[0, 1, 2, 4], [4, 3, 0, 4]]], np.uint8)
    for thr, n, c4 in ((1, 6, 1), (3, 4, 2), (4, 3, 2)):
        offs, comps, lab = np_islands.islands(cov, thr, 4)
        assert (lab >= 0).sum() == n and len(comps) == c4 and np.array_equal((lab >= 0), cov >= thr)


# ---- the painted stacks are what they say ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["diagonals", "supports", "serpentine"])
def test_a_painted_stack_is_its_bit_pattern(name):
    bits = ii.PAINTED[name]()
    L, H, W = bits.shape
    node, rect, z = ii.painted(bits)
    mx, my = np_raster.coords(rect, W, H, 1)
    T = np_sdf3d.Table.from_node(node)
    assert np.array_equal(mx, (T.ox + T.gs * np.arange(W, dtype=np.float32)).astype(np.float32)), "the samples are the table's nodes"
    assert np.array_equal(my, (T.oy + T.gs * np.arange(H, dtype=np.float32)).astype(np.float32))
    assert np.array_equal(z, (T.oz + T.gs * np.arange(L, dtype=np.float32)).astype(np.float32))
    F = np_sdf3d.evaluate(node, *np_raster.points(mx, my, z).T).reshape(L, H, W)
    assert np.array_equal(np.abs(F), np.ones_like(F))
    assert np.array_equal(np_raster.coverage(F, 1)[0] == 1, bits)


def test_every_painted_stack_fits_the_table_limits():
    for name, make in ii.PAINTED.items():
        ii.painted(make())
    for W in ii.SIZES:
        for H in ii.SIZES:
            node, rect, z = ii.painted(ii.sized(W, H))
            assert node["size_x"] >= 2 and node["size_y"] >= 2 and len(z) == 2


# ---- the preconditions of the GPU cases -------------------------------------------------------------------
def test_the_checkerboard_has_8321_components_under_4_and_one_under_8():
    _, offs, comps, lab = restated("checkerboard", 4)
    assert offs.tolist() == [0, 8321] and (comps[:, 1] == 1).all() and 8321 > 4096, "more than one tile of the scan"
    _, offs8, comps8, _ = restated("checkerboard", 8)
    assert offs8.tolist() == [0, 1] and comps8[0].tolist() == [0, 8321, 8321, 0, 0, 128, 128, 0]


@pytest.mark.parametrize("connectivity", [4, 8])
def test_the_serpentine_and_the_u_are_one_component_each(connectivity):
    bits, offs, comps, lab = restated("serpentine", connectivity)
    assert len(comps) == 1 and comps[0, 0] == 0 and comps[0, 1] == bits.sum() and comps[0, 3:7].tolist() == [0, 0, 64, 32]
    bits, offs, comps, lab = restated("u_shape", connectivity)
    assert len(comps) == 1 and comps[0, 0] == 2, "the seed is the left arm's top"
    # the arms join in row 39 between columns 2 and 67: another tile (64 x 32 pixels) than the seed's
    assert not bits[0, :39, 3:67].any() and 39 // 32 != 0


@pytest.mark.parametrize("connectivity", [4, 8])
def test_the_rings_nest_without_merging(connectivity):
    _, offs, comps, lab = restated("rings", connectivity)
    assert len(comps) == 11
    for a, b in zip(comps[:-1], comps[1:]):
        assert a[3] < b[3] and a[4] < b[4] and a[5] > b[5] and a[6] > b[6], "each box lies inside the one before"


def test_the_diagonal_pairs_split_under_4_and_join_under_8():
    bits, offs4, comps4, _ = restated("diagonals", 4)
    _, offs8, comps8, _ = restated("diagonals", 8)
    assert offs4.tolist() == [0, 6, 12] and offs8.tolist() == [0, 3, 6] and (comps8[:, 1] == 2).all()
    assert bits[0, 31, 63] and bits[0, 32, 64] and bits[1, 31, 64] and bits[1, 32, 63], "the corner of tiles (64, 32)"


def test_the_support_stack_holds_below_0_1_partial_and_full():
    _, offs, comps, _ = restated("supports", 8)
    layer1 = {tuple(r[3:7]): r for r in comps[offs[1]:offs[2]]}
    assert layer1[(20, 20, 24, 24)][1:3].tolist() == [25, 0], "the island"
    assert layer1[(9, 9, 14, 14)][1:3].tolist() == [36, 1]
    assert layer1[(33, 2, 38, 7)][1:3].tolist() == [36, 18]
    layer2 = comps[offs[2]:offs[3]]
    assert len(layer2) == 1 and layer2[0][1:3].tolist() == [25, 25]
    assert (comps[offs[0]:offs[1], 1] == comps[offs[0]:offs[1], 2]).all(), "layer 0 stands on the build plate"
    assert offs[2] - offs[1] == 3, "a layer with several components"
    below = comps[offs[3]:offs[4], 2]
    assert (below == 0).any() and (below == 1).any()


def test_the_chunked_stack_has_an_island_and_a_supported_component_on_a_chunk_s_first_layer():
    _, offs, comps, _ = restated("chunked", 8)
    for l in (4, 8):
        c = comps[offs[l]:offs[l + 1]]
        assert (c[:, 2] == 0).any() and (c[:, 2] == c[:, 1]).any(), l
        sq = [r for r in c if r[0] == 2 * 40 + 2][0]
        assert sq[1] == sq[2] == 100, "the square rests on the last layer of the chunk before"
    isl = {4: 20 * 40 + 20, 8: 5 * 40 + 30}
    for l, seed in isl.items():
        assert [r for r in comps[offs[l]:offs[l + 1]] if r[0] == seed][0][2] == 0
        assert [r for r in comps[offs[l + 1]:offs[l + 2]] if r[0] == seed][0][2] == 36 - 11 * (l == 8)


def test_the_sphere_pair_has_an_island_and_rests_on_it(oracle):
    W = H = 40
    mx, my = np_raster.coords(UNIT, W, H, 1)
    F = oracle.eval_implicit(oracle.mp5_to_nodes(json.dumps(PAIR)), np_raster.points(mx, my, PAIR_Z))
    cov = np_raster.coverage(np.asarray(F, np.float32).reshape(len(PAIR_Z), H, W), 1)[0]
    offs, comps, lab = np_islands.islands(cov, 1, 8)
    per = np.diff(offs).tolist()
    assert per == [1, 2, 1, 0, 1, 1, 1], per
    assert comps[offs[4], 2] == 0 and comps[offs[4], 1] > 0, "the upper sphere's lowest plane is an island"
    assert comps[offs[5], 2] == comps[offs[4], 1] and comps[offs[6], 2] == comps[offs[5], 1] > 0, "and the later ones rest on it"
    assert (comps[offs[1]:offs[2], 2] > 0).tolist() == [True, False], "the small sphere appears beside the lower one"


# ---- the ABI ---------------------------------------------------------------------------------------------------
def test_abi_declares_the_island_entries(impli):
    L = impli.lib()
    header = open(os.path.join(ROOT, "include", "implisolid.h")).read()
    for name, decl in (("implisolid_islands", "int64_t implisolid_islands("), ("implisolid_islands_copy", "int implisolid_islands_copy("),
                       ("implisolid_debug_islands_ms", "int implisolid_debug_islands_ms(")):
        assert hasattr(L, name) and name in impli.ABI_SYMBOLS and decl in header, name
    for word in ("threshold", "connectivity", "seed", "below == 0", "comp_offsets", "IMPLISOLID_ISLANDS_CHUNK"):
        assert word in header, word
    assert impli.COMP_DTYPE.names == np_islands.FIELDS and impli.COMP_DTYPE.itemsize == 32


fp = ctypes.POINTER(ctypes.c_float)
lp = ctypes.POINTER(ctypes.c_int64)
SPHERE = json.dumps({"type": "iellipsoid", "matrix": EYE}).encode()
NO_COPY = "implisolid_islands_copy: no records to copy (the last implisolid_islands failed, or none ran)"
REFUSALS = [
    (dict(threshold=0), "implisolid_islands: threshold must be in [1, supersample^2]"),
    (dict(threshold=5), "implisolid_islands: threshold must be in [1, supersample^2]"),
    (dict(s=1, threshold=2), "implisolid_islands: threshold must be in [1, supersample^2]"),
    (dict(connectivity=6), "implisolid_islands: connectivity must be 4 or 8"),
    (dict(n=0), "implisolid_islands: n_layers must be in [1, 65536]"),
    (dict(n=65537), "implisolid_islands: n_layers must be in [1, 65536]"),
    (dict(z=[0.0, np.nan]), "implisolid_islands: every z must be finite"),
    (dict(W=0), "implisolid_islands: width and height must be in [1, 16384]"),
    (dict(H=16385), "implisolid_islands: width and height must be in [1, 16384]"),
    (dict(s=3), "implisolid_islands: supersample must be 1, 2 or 4"),
    (dict(rect=[1, -1, -1, 1]), "raster: the rect must be finite with min < max on both axes"),
    (dict(rect=[-1, 1, -np.inf, 1]), "raster: the rect must be finite with min < max on both axes"),
    (dict(shape=b'{"type": "iellipsoid", "matrix": [1, 0'), "JSON parse error: expected , or ]"),
    (dict(shape=json.dumps({"type": "no_such_solid", "matrix": EYE}).encode()), 'Invalid object you asked for: "no_such_solid"'),
    (dict(shape=None), "implisolid_islands: bad arguments"),
    (dict(offsets=None), "implisolid_islands: bad arguments"),
    # the request is validated before the shape is compiled
    (dict(shape=b"{", connectivity=5), "implisolid_islands: connectivity must be 4 or 8"),
]


def _call(L, kw):
    n = kw.get("n", 2)
    z = np.zeros(max(n, 2), np.float32) if "z" not in kw else np.array(kw["z"], np.float32)
    rect = np.array(kw.get("rect", UNIT), np.float32)
    offs = np.zeros(max(n, 2) + 1, np.int64)
    return L.implisolid_islands(kw.get("shape", SPHERE), 0, rect.ctypes.data_as(fp), kw.get("W", 8), kw.get("H", 8), kw.get("s", 2),
                                z.ctypes.data_as(fp), n, kw.get("threshold", 1), kw.get("connectivity", 8),
                                None if "offsets" in kw else offs.ctypes.data_as(lp), None, None)


@pytest.mark.parametrize("kw, message", REFUSALS)
def test_bad_input_is_refused_before_a_device_and_empties_the_slot(impli, kw, message):
    L = impli.lib()
    assert _call(L, kw) == -1
    assert impli.last_error() == message
    out = np.zeros(8, np.int32)
    assert L.implisolid_islands_copy(out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))) == -1 and impli.last_error() == NO_COPY
    assert L.implisolid_islands_copy(None) == -1 and impli.last_error() == NO_COPY
    assert impli.raster_coords(UNIT, 8, 8, 2)[0].shape == (16,) and impli.last_error() == "", "and the next call works"


@pytest.mark.parametrize("kw", [dict(width=0), dict(height=16385), dict(z=[]), dict(z=[np.inf]), dict(supersample=3), dict(threshold=0),
                                dict(supersample=2, threshold=5), dict(connectivity=6), dict(rect=[1, -1, -1, 1])])
def test_the_python_entry_refuses_them_too(impli, kw):
    a = dict(shape=json.loads(SPHERE), rect=UNIT, width=8, height=8, z=[0.0, 0.1])
    a.update(kw)
    with pytest.raises(impli.ImplisolidError) as e:
        impli.layer_islands(**a)
    assert str(e.value)
    with pytest.raises(ValueError):
        impli.layer_islands(json.loads(SPHERE), [0, 1, 2], 8, 8, [0.0])


def test_the_timer_answers_without_a_call(impli):
    ms = impli.islands_kernel_ms(False)
    assert len(ms) == 5


def test_islands_of(impli):
    rows = np.array([[0, 5, 5, 0, 0, 4, 0, 0], [9, 3, 0, 1, 1, 3, 1, 1], [40, 7, 2, 0, 4, 6, 4, 1], [3, 1, 0, 3, 0, 3, 0, 2]], np.int32)
    comps = np.ascontiguousarray(rows).view(impli.COMP_DTYPE).reshape(-1)
    assert comps["seed"].tolist() == [0, 9, 40, 3] and comps["layer"].tolist() == [0, 1, 1, 2]
    isl = impli.islands_of(comps)
    assert isl.dtype == impli.COMP_DTYPE and isl["seed"].tolist() == [9, 3] and isl["area"].tolist() == [3, 1]
    assert len(impli.islands_of(comps[:1])) == 0
    assert np.array_equal(np_islands.as_rows(comps), rows)
