"""Host side of the hollowing query (implisolid_layer_hollow's argument checks in their order, implisolid_hollow_wall2),
the restatement tests/np_hollow.py against hand-written expectations, and the preconditions of the cases of
test_gpu_hollow.py.  No GPU."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hollow_inputs as hi   # noqa: E402
import np_hollow   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE = hi.ii.EYE
UNIT = [-1, 1, -1, 1]

_REST = {}


def restated(name, wall2, ends):
    """(bits, core) of a stack of hollow_inputs, computed once per table and ends"""
    key = (name, tuple(int(v) for v in wall2), ends)
    if key not in _REST:
        bits = hi.PAINTED[name]() if name in hi.PAINTED else getattr(hi, name)()
        _REST[key] = (bits, np_hollow.core(bits, wall2, ends))
    return _REST[key]


# ---- the restatement by hand ---------------------------------------------------------------------------------
def test_one_layer_is_the_erosion_by_the_disc():
    b = np.ones((1, 5, 5), bool)
    b[0, 0, 0] = False
    # the empty corner reaches (1, 0) and (0, 1) at 1, (1, 1) at 2, (2, 0) and (0, 2) at 4
    assert np_hollow.core(b, [0], 0).sum() == 24 and np.array_equal(np_hollow.core(b, [0], 0), b)
    c1 = np_hollow.core(b, [1], 0)[0]
    assert c1.sum() == 22 and not c1[0, 1] and not c1[1, 0] and c1[1, 1]
    c2 = np_hollow.core(b, [2], 0)[0]
    assert c2.sum() == 21 and not c2[1, 1] and c2[0, 2]
    c4 = np_hollow.core(b, [4], 0)[0]
    assert c4.sum() == 19 and not c4[0, 2] and not c4[2, 0] and c4[1, 2]


def test_a_column_of_voxels_and_the_ends():
    b = np.ones((5, 1, 1), bool)
    assert np_hollow.core(b, [0, 0], 0).reshape(-1).tolist() == [1, 1, 1, 1, 1], "nothing exists beyond the stack"
    assert np_hollow.core(b, [0, 0], 1).reshape(-1).tolist() == [0, 1, 1, 1, 1], "a floor skin of one layer"
    assert np_hollow.core(b, [0, 0], 2).reshape(-1).tolist() == [1, 1, 1, 1, 0]
    assert np_hollow.core(b, [0, 0, 0], 3).reshape(-1).tolist() == [0, 0, 1, 0, 0]
    assert np_hollow.core(b, [0] * 4, 3).sum() == 0 and np_hollow.core(b, [0] * 9, 0).sum() == 5
    b[2] = False
    assert np_hollow.core(b, [0, 0], 0).reshape(-1).tolist() == [1, 0, 0, 0, 1]
    assert np_hollow.core(b, [0], 3).reshape(-1).tolist() == [1, 1, 0, 1, 1], "reach 0 looks at no other layer"


def test_the_lens_narrows_with_the_layer_offset():
    b = np.ones((3, 1, 7), bool)
    b[0, 0, 3] = False
    c = np_hollow.core(b, [9, 4, 1], 0)
    assert c[0, 0].tolist() == [0] * 7, "within 3 pixels in its own layer"
    assert c[1, 0].tolist() == [1, 0, 0, 0, 0, 0, 1], "within 2 one layer off"
    assert c[2, 0].tolist() == [1, 1, 0, 0, 0, 1, 1], "within 1 two layers off"


def test_grey_levels_stay_in_the_shell():
    cov = np.full((1, 5, 5), 4, np.uint8)
    cov[0, 0, :] = [0, 1, 2, 3, 4]
    out, rec = np_hollow.hollow(cov, 3, [1], 0)
    # solid from 3 up: the row's first three pixels are empty; they reach (3, 0) and the three pixels below them
    assert rec.tolist() == [[22, 18]] and out.dtype == np.uint8
    assert out[0, 0].tolist() == [0, 1, 2, 3, 0] and out[0, 1].tolist() == [4, 4, 4, 0, 0] and (out[0, 2:] == 0).all()


def test_the_box_in_closed_form():
    w2 = np_hollow.wall2_table(*hi.BOX_WALL)
    assert w2 == [9, 8, 5, 0]
    bits = hi.box()
    c = np_hollow.core(bits, w2, 0)
    assert np.array_equal(c, hi.box_core(3)) and c.sum() == 34 * 34 * 6
    assert np.array_equal(np_hollow.core(bits, w2, 3), c), "the block's own margin already makes the skins"
    touching = hi.box_touching()
    got = [np_hollow.core(touching, w2, e) for e in range(4)]
    want_layers = {0: range(0, 14), 1: range(3, 14), 2: range(0, 11), 3: range(3, 11)}
    for e in range(4):
        want = np.zeros_like(touching)
        want[list(want_layers[e]), 7:41, 7:41] = True
        assert np.array_equal(got[e], want), e
    assert len({g.tobytes() for g in got}) == 4


# ---- implisolid_hollow_wall2 -----------------------------------------------------------------------------------
def test_wall2_examples(impli):
    assert impli.hollow_wall2(3, 1).tolist() == [9, 8, 5, 0] and impli.hollow_wall2(2.5, 2).tolist() == [6, 2]
    assert impli.hollow_wall2(0, 1).tolist() == [0] and impli.hollow_wall2(8, 2).tolist() == [64, 60, 48, 28, 0]
    assert impli.hollow_wall2(4, 2.5).tolist() == [16, 9] == np_hollow.wall2_table(4, 2.5)
    assert impli.hollow_wall2(3, 1).dtype == np.int64
    rng = np.random.default_rng(5)
    for wall, pitch in zip(rng.uniform(0, 40, 50), rng.uniform(0.3, 9, 50)):
        assert impli.hollow_wall2(wall, pitch).tolist() == np_hollow.wall2_table(wall, pitch), (wall, pitch)
    assert len(impli.hollow_wall2(1024, 1)) == 1025 and impli.hollow_wall2(32767.9, 1e9).tolist() == [int(np.floor(32767.9 * 32767.9))]


@pytest.mark.parametrize("wall, pitch, cap", [(np.nan, 1, 8), (np.inf, 1, 8), (-1, 1, 8), (3, np.nan, 8), (3, np.inf, 8), (3, 0, 8), (3, -2, 8),
                                              (32768, 1, 2000), (1e200, 1, 8), (1025, 1, 2000), (3, 1e-3, 5000), (3, 1, 3), (3, 1, 0),
                                              (0, 1, 0)])
def test_wall2_refusals_write_nothing(impli, wall, pitch, cap):
    L = impli.lib()
    buf = np.full(max(cap, 8), 77, np.int64)
    assert L.implisolid_hollow_wall2(wall, pitch, buf.ctypes.data_as(lp), cap) == -1
    assert impli.last_error().startswith("implisolid_hollow_wall2: ") and (buf == 77).all()
    assert np_hollow.wall2_table(wall, pitch) is None or len(np_hollow.wall2_table(wall, pitch)) > cap
    assert L.implisolid_hollow_wall2(3.0, 1.0, buf.ctypes.data_as(lp), 4) == 3 and impli.last_error() == "" and buf[:5].tolist() == [9, 8, 5, 0, 77]
    assert L.implisolid_hollow_wall2(3.0, 1.0, None, 4) == -1
    with pytest.raises(impli.ImplisolidError):
        impli.hollow_wall2(wall, pitch if cap >= 8 else -1)


# ---- the ABI ---------------------------------------------------------------------------------------------------
def test_abi_declares_the_hollow_entries(impli):
    L = impli.lib()
    header = open(os.path.join(ROOT, "include", "implisolid.h")).read()
    for name in ("implisolid_layer_hollow", "implisolid_hollow_wall2", "implisolid_debug_layer_hollow_ms"):
        assert hasattr(L, name) and name in impli.ABI_SYMBOLS and ("int %s(" % name) in header, name
    for word in ("wall2", "reach", "ends", "core", "IMPLISOLID_HOLLOW_CHUNK", "no skin at the image's sides"):
        assert word in header, word
    assert impli.HOLLOW_DTYPE.names == np_hollow.FIELDS and impli.HOLLOW_DTYPE.itemsize == 16


fp = ctypes.POINTER(ctypes.c_float)
lp = ctypes.POINTER(ctypes.c_int64)
SPHERE = json.dumps({"type": "iellipsoid", "matrix": EYE}).encode()
WHO = "implisolid_layer_hollow: "
# in the order of the checks: each entry's message wins over every later entry's
ORDER = [
    ("null shape", dict(shape=None), WHO + "bad arguments"),
    ("0 layers", dict(n=0), WHO + "n_layers must be in [1, 65536]"),
    ("nan z", dict(z=[0.0, np.nan]), WHO + "every z must be finite"),
    ("height 16385", dict(H=16385), WHO + "width and height must be in [1, 16384]"),
    ("supersample 3", dict(s=3), WHO + "supersample must be 1, 2 or 4"),
    ("threshold 5", dict(threshold=5), WHO + "threshold must be in [1, supersample^2]"),
    ("reach 1025", dict(reach=1025), WHO + "reach must be in [0, 1024]"),
    ("wall2 rising", dict(wall2=[1, 2], reach=1), WHO + "wall2 must be in [0, 2^30) and non-increasing"),
    ("ends 4", dict(ends=4), WHO + "ends must be in [0, 3]"),
    ("reversed rect", dict(rect=[1, -1, -1, 1]), "raster: the rect must be finite with min < max on both axes"),
    ("truncated shape", dict(shape=b'{"type": "iellipsoid", "matrix": [1, 0'), "JSON parse error: expected , or ]"),
]
ALONE = [
    (dict(rect=None), WHO + "bad arguments"),
    (dict(z=None), WHO + "bad arguments"),
    (dict(wall2=None), WHO + "bad arguments"),
    (dict(rec=None), WHO + "bad arguments"),
    (dict(n=65537), WHO + "n_layers must be in [1, 65536]"),
    (dict(z=[np.inf, 0.0]), WHO + "every z must be finite"),
    (dict(W=0), WHO + "width and height must be in [1, 16384]"),
    (dict(s=0), WHO + "supersample must be 1, 2 or 4"),
    (dict(threshold=0), WHO + "threshold must be in [1, supersample^2]"),
    (dict(s=1, threshold=2), WHO + "threshold must be in [1, supersample^2]"),
    (dict(reach=-1), WHO + "reach must be in [0, 1024]"),
    # 1024 x 1024 tiles a layer: one layer fills the window budget, three do not fit
    (dict(W=16384, H=16384, reach=1, wall2=[1, 1]), WHO + "(2 reach + 1) layers must hold at most 2^20 tiles"),
    (dict(W=16384, H=16, reach=512, wall2=[0] * 513), WHO + "(2 reach + 1) layers must hold at most 2^20 tiles"),
    (dict(wall2=[-1]), WHO + "wall2 must be in [0, 2^30) and non-increasing"),
    (dict(wall2=[1 << 30]), WHO + "wall2 must be in [0, 2^30) and non-increasing"),
    (dict(wall2=[5, 5, 4, 6], reach=3), WHO + "wall2 must be in [0, 2^30) and non-increasing"),
    (dict(ends=-1), WHO + "ends must be in [0, 3]"),
    (dict(rect=[-1, 1, -np.inf, 1]), "raster: the rect must be finite with min < max on both axes"),
    (dict(shape=json.dumps({"type": "no_such_solid", "matrix": EYE}).encode()), 'Invalid object you asked for: "no_such_solid"'),
]


def _call(L, kw):
    n = kw.get("n", 2)
    z = None if "z" in kw and kw["z"] is None else np.zeros(max(n, 2), np.float32) if "z" not in kw else np.array(kw["z"], np.float32)
    rect = None if "rect" in kw and kw["rect"] is None else np.array(kw.get("rect", UNIT), np.float32)
    wall2 = None if "wall2" in kw and kw["wall2"] is None else np.array(kw.get("wall2", [1]), np.int64)
    rec = np.full(2 * max(n, 2), 77, np.int64)
    out = np.full(8, 77, np.uint8)
    stats = np.full(8, 77, np.int64)
    rc = L.implisolid_layer_hollow(kw.get("shape", SPHERE), 0, None if rect is None else rect.ctypes.data_as(fp), kw.get("W", 8),
                                   kw.get("H", 8), kw.get("s", 2), None if z is None else z.ctypes.data_as(fp), n, kw.get("threshold", 1),
                                   None if wall2 is None else wall2.ctypes.data_as(lp), kw.get("reach", 0), kw.get("ends", 0),
                                   out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), None if "rec" in kw else rec.ctypes.data_as(lp),
                                   stats.ctypes.data_as(lp))
    assert (rec == 77).all() and (out == 77).all() and (stats == 77).all(), "a refused call writes nothing"
    return rc


@pytest.mark.parametrize("kw, message", [(kw, m) for _, kw, m in ORDER] + ALONE)
def test_bad_input_is_refused_before_a_device(impli, kw, message):
    L = impli.lib()
    assert _call(L, kw) == -1
    assert impli.last_error() == message
    assert impli.raster_coords(UNIT, 8, 8, 2)[0].shape == (16,) and impli.last_error() == "", "and the next call works"


@pytest.mark.parametrize("first", range(len(ORDER) - 1))
def test_the_refusals_come_in_order(impli, first):
    L = impli.lib()
    name, kw, message = ORDER[first]
    for later, kw2, _ in ORDER[first + 1:]:
        both = dict(kw2)
        both.update(kw)
        if set(kw) & set(kw2):
            continue   # both mistakes in one argument: one of them cannot be made
        assert _call(L, both) == -1 and impli.last_error() == message, (name, later)


@pytest.mark.parametrize("kw", [dict(width=0), dict(height=16385), dict(z=[]), dict(z=[np.inf]), dict(supersample=3), dict(threshold=0),
                                dict(supersample=2, threshold=5), dict(wall2=[]), dict(wall2=[1.5]), dict(wall2=[-1]), dict(wall2=[1 << 30]),
                                dict(wall2=[1 << 70]), dict(wall2=[1, 2]), dict(wall2=[0] * 1026), dict(ends=4), dict(ends=-1),
                                dict(rect=[1, -1, -1, 1])])
def test_the_python_entry_refuses_them_too(impli, kw):
    a = dict(shape=json.loads(SPHERE), rect=UNIT, width=8, height=8, z=[0.0, 0.1], wall2=[1])
    a.update(kw)
    with pytest.raises(impli.ImplisolidError) as e:
        impli.layer_hollow(**a)
    assert str(e.value)


def test_the_timer_answers_without_a_call(impli):
    assert len(impli.layer_hollow_kernel_ms(False)) == 4


# ---- the preconditions of the GPU cases ----------------------------------------------------------------------------
def test_the_hole_s_shell_is_the_ellipsoid():
    bits = hi.one_hole()
    hx, hy, hl = hi.HOLE
    l, y, x = np.mgrid[0:9, 0:70, 0:70]
    for name, (wall, pitch) in hi.HOLE_WALLS.items():
        w2 = np_hollow.wall2_table(wall, pitch)
        c = np_hollow.core(bits, w2, 0)
        dl = np.abs(l - hl)
        lens = (dl < len(w2)) & ((x - hx) ** 2 + (y - hy) ** 2 <= np.array(w2 + [-1] * 9)[np.minimum(dl, len(w2))])
        assert np.array_equal(~c, lens), name
        assert lens.sum() > 1 and {int(v) for v in dl[lens]} == set(range(len(w2))), "the shell spans every layer within reach"
    assert np_hollow.wall2_table(4, 1) == [16, 15, 12, 7, 0] and np_hollow.wall2_table(4, 2.5) == [16, 9]
    # the shell crosses a tile border, and every tile of the 5 x 5 holds core voxels that look at the hole's layer
    own = np_hollow.core(bits, [16], 0)[hl]
    assert len({(int(py) // 16, int(px) // 16) for py, px in np.argwhere(~own)}) == 2
    assert len({(int(py) // 16, int(px) // 16) for py, px in np.argwhere(own)}) == 25


@pytest.mark.parametrize("reach", sorted(hi.WALLS))
@pytest.mark.parametrize("name", sorted(hi.PAINTED))
def test_the_painted_stacks_hold_core_and_shell(name, reach):
    w2 = hi.WALLS[reach]
    assert len(w2) == reach + 1
    bits, c = restated(name, w2, 3)
    shell = bits & ~c
    if name == "random_50":
        assert shell.any() and (reach > 0 or c.any()), "half full: hardly any core, none beyond its own layer"
    elif name == "one_class":
        # layers 0 and 2 .. 5 are solid without a distance; only the empty layer 1 and the ends make a shell
        want = {0: [0, 2, 3, 4, 5], 1: [3, 4], 4: []}[reach]
        assert [l for l in range(6) if c[l].any()] == want and all(c[l].all() for l in want)
        open_ends = np_hollow.core(bits, w2, 0)
        assert [l for l in range(6) if open_ends[l].any()] == {0: [0, 2, 3, 4, 5], 1: [3, 4, 5], 4: []}[reach]
    else:
        assert shell.any() and (c.any() or (name, reach) == ("random_95", 4)), (name, reach)   # nine dense layers: no core left
    for e in (0, 3):
        assert (np_hollow.core(bits, w2, e) <= bits).all()
    if reach:   # the other layers decide something: the window is not the layer's own erosion
        alone = np_hollow.core(bits, w2[:1], 0)
        assert not np.array_equal(np_hollow.core(bits, w2, 0), alone) or name == "random_50"
        # ... and both directions do: looking only ahead (offsets j >= 0) gives another core
        ahead = alone.copy()
        for l in range(len(bits)):
            for j in range(1, reach + 1):
                if l + j < len(bits):
                    ahead[l] &= ~np_hollow.reached(~bits[l + j], w2[j])
        assert not np.array_equal(np_hollow.core(bits, w2, 0), ahead) or name in ("random_50", "one_class"), name


def test_a_threshold_hit_exactly_decides():
    # > and >= differ where a distance equals its threshold: the staircase holds such voxels at every reach
    bits = hi.PAINTED["staircase"]()
    for reach, w2 in hi.WALLS.items():
        strict = np_hollow.core(bits, w2, 0)
        loose = np_hollow.core(bits, [max(v - 1, 0) for v in w2], 0)
        assert strict.sum() < loose.sum(), reach


def test_the_sized_and_deep_stacks():
    some = 0
    for W in hi.SIZES:
        for H in hi.SIZES:
            bits = hi.sized(W, H)
            assert bits.shape == (3, H, W) and bits.any()
            c = np_hollow.core(bits, hi.SIZED_WALL, 0)
            if W >= 15 and H >= 15:
                assert c.any() and (bits & ~c).any() and not bits.all(), (W, H)
            some += int(c.any())
    assert some >= 40
    assert hi.DEPTHS == [1, 2, 3, 4, 7, 8] and len(hi.DEPTH_WALL) == hi.DEPTH_REACH + 1
    for n in hi.DEPTHS:
        bits = hi.deep(n)
        for ends in (0, 3):
            c = np_hollow.core(bits, hi.DEPTH_WALL, ends)
            assert (bits & ~c).any() and (c.any() or (ends == 3 and n < 2 * hi.DEPTH_REACH + 1)), (n, ends)
    bits = hi.shallow()
    assert len(hi.FAR_REACH_WALL) - 1 > len(bits)
    c = np_hollow.core(bits, hi.FAR_REACH_WALL, 0)
    assert c.any() and (bits & ~c).any() and not np_hollow.core(bits, hi.FAR_REACH_WALL, 1).any()
