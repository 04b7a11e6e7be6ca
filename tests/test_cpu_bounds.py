"""Host side of the bounds of a solid (no GPU): the edge table, the fitted-box formula, the "fit_box"
settings key, and the callers that refuse it -- against tests/np_bounds.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_bounds   # noqa: E402

EYE = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
SPHERE = {"type": "iellipsoid", "matrix": EYE}

BOXES = {
    "unit": [-1, 1, -1, 1, -1, 1],
    "asymmetric": [-0.3, 1.7, 0.125, 0.9, -2.5, -0.1],
    "large_offsets": [1000.1, 1003.7, -5000.3, -4999.2, 123456.0, 123457.5],
    "thirds": [-1 / 3, 2 / 3, -0.7, 0.1, 0.001, 0.0123],
}


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("depth", [3, 7, 10])
@pytest.mark.parametrize("name", sorted(BOXES))
def test_edges_equal_the_restatement(impli, name, depth):
    s = np.array(BOXES[name], np.float32)
    e = impli.bounds_edges(s, depth)
    N = 1 << depth
    assert e.shape == (3, N + 1) and e.dtype == np.float32
    assert np.array_equal(_u32(e), _u32(np_bounds.edges(s, depth)))
    assert np.array_equal(_u32(e[:, N]), _u32(s[1::2])) and np.array_equal(_u32(e[:, 0]), _u32(s[0::2]))
    assert (np.diff(e.astype(np.float64), axis=1) >= 0).all(), "the edges are monotone"
    assert (e[:, 0] < e[:, N]).all()


def test_edges_nest_across_levels(impli):
    """Box i of level l spans edge[i << (depth - l)] .. edge[(i + 1) << (depth - l)] of the one
    table: a child's ends are its parent's ends or the edge between them."""
    e = impli.bounds_edges(BOXES["asymmetric"], 10)[0]
    for level in range(3, 10):
        sh = 10 - level
        i = np.arange(1 << level)
        p0, p1 = e[i << sh], e[(i + 1) << sh]
        c = e[(2 * i + 1) << (sh - 1)]
        assert (p0 <= c).all() and (c <= p1).all()


@pytest.mark.parametrize("bad", [[-1, 1, -1, 1, 1, -1], [0, 0, -1, 1, -1, 1], [-1, np.inf, -1, 1, -1, 1],
                                 [np.nan, 1, -1, 1, -1, 1], [-3e38, 3e38, -1, 1, -1, 1]])
def test_edges_refuse_bad_boxes(impli, bad):
    with pytest.raises(impli.ImplisolidError):
        impli.bounds_edges(bad, 5)


@pytest.mark.parametrize("depth", [2, 11, -1])
def test_edges_refuse_bad_depths(impli, depth):
    with pytest.raises(impli.ImplisolidError):
        impli.bounds_edges(BOXES["unit"], depth)


FIT_CASES = [
    # search, bounds, resolution, margin
    (BOXES["unit"], [0.09375, 0.5, -0.125, 0.3125, -0.40625, 0.0], 32, 2),
    (BOXES["unit"], [-1, 0.5, -0.125, 1, -0.96875, 0.96875], 32, 2),            # sides that clamp to the settings box
    (BOXES["unit"], [-1, 1, -1, 1, -1, 1], 28, 3),                              # everything clamps
    (BOXES["large_offsets"], [1001.3, 1002.9, -5000.1, -4999.6, 123456.1, 123457.4], 512, 2),
    (BOXES["thirds"], [-0.1, 0.3, -0.5, 0.0, 0.002, 0.011], 7, 3),               # one cell for the bounds
    (BOXES["asymmetric"], [0.0, 1.0, 0.25, 0.75, -2.0, -1.0], 100, 0),           # no margin: the bounds themselves
]


@pytest.mark.parametrize("case", range(len(FIT_CASES)))
def test_fit_box_equals_the_restatement(impli, case):
    s, b, R, m = FIT_CASES[case]
    got = impli.fit_box(s, b, R, m)
    want = np_bounds.fit_box(s, b, R, m)
    assert np.array_equal(_u32(got), _u32(want)), (got, want)
    s32, b32 = np.array(s, np.float32), np.array(b, np.float32)
    assert (got[0::2] >= s32[0::2]).all() and (got[1::2] <= s32[1::2]).all(), "never leaves the settings box"
    assert (got[0::2] <= b32[0::2]).all() and (got[1::2] >= b32[1::2]).all(), "holds the bounds"


def test_fit_box_clamps_and_refuses(impli):
    got = impli.fit_box(BOXES["unit"], [-1, 0.5, -0.125, 1, -0.96875, 0.96875], 32, 2)
    assert got[0] == -1 and got[3] == 1 and got[4] == -1 and got[5] == 1
    assert got[1] > 0.5 and got[2] < -0.125
    for R, m in [(4, 2), (3, 2), (32, 16), (32, -1)]:
        assert np_bounds.fit_box(BOXES["unit"], BOXES["unit"], R, m) is None
        with pytest.raises(impli.ImplisolidError):
            impli.fit_box(BOXES["unit"], BOXES["unit"], R, m)
    assert impli.fit_box(BOXES["unit"], BOXES["unit"], 5, 2) is not None   # one cell left


def test_settings_key_parses(impli):
    from implisolid_amd import scenes
    mc = scenes.mc_settings(32, 1.0)
    assert "fit_box" not in mc, "the key is emitted only when given"
    assert impli.parse_fit_box(mc) == {"enabled": 0, "depth": 5, "margin": 2}
    assert impli.parse_fit_box(scenes.mc_settings(32, 1.0, fit_box=True)) == {"enabled": 1, "depth": 5, "margin": 2}
    assert impli.parse_fit_box(scenes.mc_settings(33, 1.0, fit_box=True))["depth"] == 6      # ceil(log2(R))
    assert impli.parse_fit_box(scenes.mc_settings(4, 1.0, fit_box={"margin": 1}))["depth"] == 3    # clamped below
    assert impli.parse_fit_box(scenes.mc_settings(4000, 1.0, fit_box=True))["depth"] == 10   # clamped above
    got = impli.parse_fit_box(scenes.mc_settings(64, 1.0, fit_box={"depth": 7, "margin": 3}))
    assert got == {"enabled": 1, "depth": 7, "margin": 3}
    # read as "projection.enabled" is: values that are no ints leave the key off
    for v in (True, False, "yes", 1.5, None, [1], {"on": 1}, 0):
        mc = scenes.mc_settings(32, 1.0)
        mc["fit_box"] = {"enabled": v}
        assert impli.parse_fit_box(mc)["enabled"] == 0, v
    for v in (1, 2, -3, "1"):
        mc = scenes.mc_settings(32, 1.0)
        mc["fit_box"] = {"enabled": v}
        assert impli.parse_fit_box(mc)["enabled"] == 1, v
    # the other settings are read as before
    a = impli.parse_settings(scenes.mc_settings(48, 0.75, projection=1, fit_box={"depth": 4}))
    b = impli.parse_settings(scenes.mc_settings(48, 0.75, projection=1))
    assert a == b


@pytest.mark.parametrize("fit", [{"depth": 2}, {"depth": 11}, {"margin": -1}, {"margin": 16}])
def test_settings_key_refuses_bad_values(impli, fit):
    from implisolid_amd import scenes
    with pytest.raises(impli.ImplisolidError) as e:
        impli.parse_fit_box(scenes.mc_settings(32, 1.0, fit_box=fit))
    assert "fit_box" in str(e.value)
    # a disabled key's values are not judged
    mc = scenes.mc_settings(32, 1.0, fit_box=fit)
    mc["fit_box"]["enabled"] = 0
    assert impli.parse_fit_box(mc)["enabled"] == 0


def test_slab_and_batch_refuse_the_key(impli):
    """Their grids are the caller's (a slab of the settings box) or shared by all objects: an enabled
    key is an error that names it, raised from the settings alone -- before any device is touched."""
    from implisolid_amd import scenes
    mc = scenes.mc_settings(32, 1.0, fit_box=True)
    with pytest.raises(impli.ImplisolidError) as e:
        impli.Slab(SPHERE, mc)
    assert "fit_box" in str(e.value)
    with pytest.raises(impli.ImplisolidError) as e:
        impli.Slab(SPHERE, mc, cuts=[1, 35], rank=0, nranks=1)
    assert "fit_box" in str(e.value)
    for n_streams in (0, 2):
        with pytest.raises(impli.ImplisolidError) as e:
            impli.Batch([SPHERE, SPHERE], mc, n_streams=n_streams)
        assert "fit_box" in str(e.value)


def test_abi_declares_the_bounds_entries(impli):
    L = impli.lib()
    for name in ("implisolid_bounds", "implisolid_bounds_edges", "implisolid_fit_box", "implisolid_parse_fit_box",
                 "implisolid_last_fit_box", "implisolid_debug_bounds_ms"):
        assert hasattr(L, name) and name in impli.ABI_SYMBOLS, name
    assert impli.last_fit_box() is None or impli.last_fit_box().shape == (6,)
