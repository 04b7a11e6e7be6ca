"""CPU checks behind the per-vertex normals kernel (ob02_device.hpp vertex_normals_body): the two
float forms it uses are the reference's double forms (mcc2.cpp:852-871) for every float, and the
"normals" settings key reaches the library without touching the caller's settings.  No GPU."""
import json

import numpy as np

import np_normals

THRESHOLD_BITS = 0x38D1B717   # the float nearest 0.0001


def test_float_quotient_is_the_rounded_double_quotient():
    """(float)(-1.0 / (double)norm) == -1.0f / norm over a stride through every positive float pattern
    (zero, subnormals, infinity and NaN included), plus dense windows at both ends and around the
    threshold, where the kernel's branch changes."""
    stride = np.arange(0, 0x7FFFFFFF, 251, dtype=np.int64)
    wins = np.concatenate([np.arange(c - 4096, c + 4096, dtype=np.int64) for c in
                           (4096, 0x00800000, THRESHOLD_BITS, 0x3F800000, 0x7F800000 - 4096, 0x7F800000 + 4096)])
    pats = np.concatenate([stride, wins]).astype(np.uint32)
    norm = pats.view(np.float32)
    with np.errstate(all="ignore"):
        via_double = (-1.0 / norm.astype(np.float64)).astype(np.float32)
        via_float = np.float32(-1.0) / norm
    assert via_float.dtype == np.float32
    same = (via_double.view(np.uint32) == via_float.view(np.uint32)) | (np.isnan(via_double) & np.isnan(via_float))
    assert same.all(), (pats[~same][:8], via_double[~same][:4], via_float[~same][:4])


def test_float_threshold_is_the_double_threshold():
    """norm > 0.0001 (double) == norm > 0.0001f on the +-64 float patterns around 0x38d1b717."""
    assert np.float32(0.0001).view(np.uint32) == THRESHOLD_BITS
    pats = np.arange(THRESHOLD_BITS - 64, THRESHOLD_BITS + 65, dtype=np.int64).astype(np.uint32)
    norm = pats.view(np.float32)
    as_double = norm.astype(np.float64) > 0.0001
    as_float = norm > np.float32(0.0001)
    assert np.array_equal(as_double, as_float), pats[as_double != as_float]
    assert as_double.any() and not as_double.all()
    for special in (0.0, np.inf, np.nan):
        x = np.float32(special)
        assert (np.float64(x) > 0.0001) == (x > np.float32(0.0001))


def test_rule_on_special_rows():
    g = np.array([[3.0, 0.0, 4.0], [0.0, 0.0, 0.0], [-0.0, 0.0, 0.0], [np.nan, 1.0, 0.0], [np.inf, 0.0, 0.0],
                  [5e-5, 0.0, 0.0], [0.0, 0.5, 0.0]], np.float32)
    n, bad = np_normals.normals_rule(g)
    assert bad == 4                                      # the zeros, the NaN row, |g| = 5e-5
    assert np.array_equal(n[0], np.float32([-0.6, -0.0, -0.8]))
    assert n[1].view(np.uint32).tolist() == [0x80000000] * 3   # 0 * -42 = -0
    assert n[2].view(np.uint32).tolist() == [0x00000000, 0x80000000, 0x80000000]
    assert np.isnan(n[3, 0]) and n[3, 1] == np.float32(-42.0)
    assert np.isnan(n[4, 0])                             # inf * (-1 / inf) = inf * -0
    assert n[5, 0] == np.float32(5e-5) * np.float32(-42.0)
    assert n[6, 1] == np.float32(-1.0)


def test_normals_keyword_merges_into_a_copy(impli):
    mc = {"resolution": 24, "normals": {"note": "kept"}, "box": {"xmin": -1}}
    before = json.dumps(mc, sort_keys=True)
    merged = impli._with_normals(mc, True)
    assert json.dumps(mc, sort_keys=True) == before      # the caller's dict, nested one included, is untouched
    assert merged is not mc and merged["normals"] == {"note": "kept", "enabled": 1}
    assert impli._with_normals(mc, False) is mc
    assert impli._with_normals(json.dumps({"resolution": 24}), True) == {"resolution": 24, "normals": {"enabled": 1}}
    assert impli._with_normals({"resolution": 24, "normals": 0}, True)["normals"] == {"enabled": 1}


def test_normals_key_leaves_the_parsed_settings_alone(impli, oracle):
    """implisolid_parse_settings and the oracle ignore the key: the other settings parse as before."""
    from implisolid_amd import scenes
    mc = scenes.mc_settings(24, 1.0, vresampl_iters=1, projection=1, qem=1, overall_repeats=2)
    want = impli.parse_settings(mc)
    for val in (1, 0, True, "x"):
        got = impli.parse_settings(dict(mc, normals={"enabled": val}))
        assert json.dumps(got, default=float, sort_keys=True) == json.dumps(want, default=float, sort_keys=True)
    s = oracle.parse_mc_settings(json.dumps(dict(mc, normals={"enabled": 1})))
    assert s.resolution == 24 and s.overall_repeats == 2


def test_abi_declares_the_normals_entries(impli):
    L = impli.lib()
    for name in ("get_n_size", "get_n_ptr", "get_n", "implisolid_normals_stats", "implisolid_eval_normals",
                 "implisolid_slab_emit_normals", "implisolid_slab_normals", "implisolid_slab_download_normals"):
        assert hasattr(L, name) and name in impli.ABI_SYMBOLS, name
    # host state only: nothing built yet in this process, or the last build's -- the calls are safe without a GPU
    assert L.get_n_size() >= 0
    _, _, src = impli.jit_compile({"type": "iellipsoid", "matrix": [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]}, points=True)
    assert "impli_pt_vertex_normals" in src and "vertex_normals_body" in src
