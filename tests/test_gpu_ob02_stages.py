"""GPU, OB02 stages one by one: the device's QEM against the float64 reference of the operation
(tests/np_ob02.py), the projection and the QEM each against the oracle on the device's own input,
the projected centroids against what any correct search must give, and both stages on meshes that
marching cubes never makes.

The parity tests compare whole loops with the oracle, which restates the same Eigen JacobiSVD as
ob02.hip does; tests/test_cpu_ob02.py pins the oracle to float64 and fixes the bound used here."""
import json

import numpy as np
import pytest

import matrices
import np_ob02
from test_cpu_ob02 import EITHER_WAY_CAP, M_CLAMP, M_RANK, MC_SCENES, oracle_stages, qem_bound, scene
from test_gpu_parity import SCREW_TREES, sync_jit  # noqa: F401  (sync_jit: fixture)

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_rows(a, b):
    """Rows equal bit for bit, a NaN matching a NaN."""
    return ((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))).all(1)


def _gpu_scene(name):
    """-> (shape, R, box) of the scenes built here: the three of the CPU test, a twist and a tree of
    general (rotated, non-dyadic) node matrices with a twist leaf."""
    if name == "twist_40":
        return SCREW_TREES["twist"], 40, 0.7
    if name == "matrix_rot_24":
        return matrices.family_tree("rot", seed=0, twist=True), 24, 1.0
    shape, R, _ = scene(name)
    return shape, R, 1.0


def _build(impli, name):
    """One repeat of one resampling, the projection and QEM on the device, and the point sets the
    loop recorded on its way."""
    from implisolid_amd import scenes
    shape, R, box = _gpu_scene(name)
    mc = scenes.mc_settings(R, box, vresampl_iters=1, vresampl_c=0.4, projection=1, qem=1)
    v, f = impli.make_geometry(shape, mc)
    out = {k: impli.get_pointset(k) for k in ("pre_p_centroids", "post_p_centroids", "pre_qem_verts", "post_qem_verts")}
    assert all(p is not None for p in out.values())
    assert np.array_equal(_bits(out["post_qem_verts"]), _bits(v))
    assert out["post_p_centroids"].shape == (len(f), 3) and out["pre_qem_verts"].shape == v.shape
    out.update(shape=shape, faces=f, avg32=impli.last_build_stats()["avg_edge"], jit_launches=impli.last_build_stats()["jit_launches"])
    with impli.ImplicitService(shape) as svc:
        out["f_at_c"], out["grad_at_c"] = svc.eval(out["post_p_centroids"], gradient=True)
    return out


_BUILDS = {}


def _stages(impli, name):
    """The interpreter (or async-JIT) build of a scene, made once and shared (read only)."""
    if name not in _BUILDS:
        _BUILDS[name] = _build(impli, name)
        for a in _BUILDS[name].values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return _BUILDS[name]


def _assert_qem_is_float64s(oracle, name, s, what):
    """The acceptance rule of test_cpu_ob02.test_oracle_qem_matches_float64, on the device's vertices."""
    pre, f = s["pre_qem_verts"], s["faces"]
    ref = np_ob02.QemReference(pre, f, s["post_p_centroids"], np_ob02.unit_normals_f32(s["grad_at_c"]),
                               np_ob02.average_edge(pre, f))
    err, either = np_ob02.qem_errors(s["post_qem_verts"], ref, M_RANK, M_CLAMP)
    ranks = np.bincount(ref.rank, minlength=4)
    bound = qem_bound(oracle)
    print(what, "verts", len(err), "ranks 0..3", ranks.tolist(), "clamped", int(ref.clamped.sum()),
          "worst %.3g p99 %.3g bound %.3g" % (err.max(), np.percentile(err, 99), bound), "either-way %d" % either.sum())
    assert ref.finite.all() and np.isfinite(s["post_qem_verts"]).all()
    assert ranks[1] > 0 and ranks[2] > 0 and ranks[3] > 0 and ref.clamped.any(), (ranks, ref.clamped.sum())
    assert abs(s["avg32"] / ref.avg - 1.0) < 3 * len(f) * 2.0 ** -24   # a sequential f32 sum of 3 nf terms
    assert either.mean() <= EITHER_WAY_CAP, either.sum()
    bad = np.flatnonzero(~(err <= bound))
    assert bad.size == 0, (what, bad.size, bad[:10], err[bad[:10]], ref.rank[bad[:10]])


# ---- a. QEM against float64 -------------------------------------------------------------------------
@pytest.mark.parametrize("name", MC_SCENES)
def test_qem_matches_float64(impli, oracle, name):
    """post_qem_verts is the float64 minimum-norm step from pre_qem_verts towards the planes through
    post_p_centroids, under the bound and the "either way" rule the CPU test holds the oracle to.

    Measured on an MI355X, worst error / avg (the oracle's next to it): config2_24 1.45e-5 (1.45e-5),
    config2_32 1.80e-5 (1.80e-5), config3_32 4.06e-5 (4.06e-5); bound 1.63e-4."""
    _assert_qem_is_float64s(oracle, name, _stages(impli, name), name)


@pytest.mark.parametrize("bake", [False, True])
def test_qem_matches_float64_jit(impli, oracle, sync_jit, bake):
    """The same over the JIT point module (it supplies the centroids and the normals k_qem reads),
    and over the module with the matrices baked in."""
    if bake:
        impli.set_jit_bake(1)
    try:
        s = _build(impli, "config2_24")
    finally:
        impli.set_jit_bake(2)
    assert s["jit_launches"] > 0
    _assert_qem_is_float64s(oracle, "config2_24", s, "config2_24 jit bake=%d" % bake)
    base = _stages(impli, "config2_24")
    assert _same_rows(s["post_p_centroids"], base["post_p_centroids"]).all()
    assert _same_rows(s["post_qem_verts"], base["post_qem_verts"]).all()


# ---- b. each stage against the oracle, on the device's own input ------------------------------------
@pytest.mark.parametrize("name", ["config2_24", "config3_32", "twist_40", "matrix_rot_24"])
def test_projection_and_qem_stage_against_oracle(impli, oracle, name):
    """The oracle's centroids_projection on the device's pre_qem_verts gives the device's
    post_p_centroids and post_qem_verts bit for bit (NaN rows matching): a wrong centroid shows here
    itself, not through n n^T (c - v) where the rank and the clamp allow."""
    s = _stages(impli, name)
    tree = oracle.mp5_to_nodes(json.dumps(s["shape"]))
    vr, cr, avg = oracle.centroids_projection(tree, s["pre_qem_verts"], s["faces"], 1)
    bad = np.flatnonzero(~_same_rows(s["post_p_centroids"], cr))
    assert bad.size == 0, (name, "centroids", bad.size, bad[:10])
    bad = np.flatnonzero(~_same_rows(s["post_qem_verts"], vr))
    assert bad.size == 0, (name, "vertices", bad.size, bad[:10])
    assert np.float32(s["avg32"]) == np.float32(avg)
    assert len(vr) > 500 and np.isfinite(vr).all(1).mean() > 0.9


# ---- c. projection invariants -----------------------------------------------------------------------
# scenes with flat parts (a twist's lids, config 3's cut faces) on which many centroids already lie
# within ROOT_TOLERANCE of the surface and stay: there the oracle itself moves fewer than 95 % of
# the faces (config3_32: 92.3 %, twist_40: 90.4 %)
STAY_PUT_SCENES = {"config3_32", "twist_40"}


@pytest.mark.parametrize("name", MC_SCENES + ["twist_40", "matrix_rot_24"])
def test_projected_centroids_invariants(impli, name):
    """Needs no oracle projection.  Every face's centroid either stays, bit for bit, or lands where
    |f| <= ROOT_TOLERANCE = (float)(0.001 / 10) (configs.hpp:33; f by the bit-exact point path); it
    moves no further than 15/16 of the average edge (np_ob02.MAX_ALPHA: the largest |alpha| of
    set_centers_on_surface's list, a tighter bound than the average edge itself; plus a few ulp); at
    least 95 % of the faces move -- except in STAY_PUT_SCENES, where the oracle moves fewer -- and in
    every scene at least 95 % of the centroids end within ROOT_TOLERANCE of the surface.

    Measured on the oracle: every moved centroid has |f| <= 1.0e-4; the largest displacement is
    0.9375 avg (= 15/16, config2_32; 0.937 config2_24, 0.901 config3_32, 0.492 twist_40, 0.861
    matrix_rot_24); faces moved 98.6 % config2_24, 98.0 % config2_32, 99.9 % matrix_rot_24, 92.3 %
    config3_32, 90.4 % twist_40."""
    s = _stages(impli, name)
    avg64 = np_ob02.average_edge(s["pre_qem_verts"], s["faces"])
    assert abs(s["avg32"] / avg64 - 1.0) < 3 * len(s["faces"]) * 2.0 ** -24
    c0 = s["pre_p_centroids"]
    p = s["pre_qem_verts"][s["faces"]]
    assert np.array_equal(_bits(c0), _bits(((p[:, 0] + p[:, 1]) + p[:, 2]) / np.float32(3.0)))
    inv = np_ob02.projection_invariants(c0, s["post_p_centroids"], s["f_at_c"], s["avg32"])
    print(name, "faces", len(c0), "moved %.4f on surface %.4f" % (inv["moved_share"], inv["on_surface_share"]),
          "worst |f| %.4g" % inv["worst_f"],
          "worst displacement %.6f avg (bound %.6f)" % (inv["worst_disp"], inv["disp_bound"]))
    assert not inv["bad_f"].any(), (name, np.flatnonzero(inv["bad_f"])[:10], inv["worst_f"])
    assert not inv["bad_disp"].any(), (name, np.flatnonzero(inv["bad_disp"])[:10], inv["worst_disp"])
    assert inv["on_surface_share"] >= 0.95, inv["on_surface_share"]
    if name not in STAY_PUT_SCENES:
        assert inv["moved_share"] >= 0.95, inv["moved_share"]


# ---- 4. meshes marching cubes never makes -----------------------------------------------------------
def _project_on_device(impli, shape, v, f, v0, v1):
    import torch
    from implisolid_amd import scenes
    mc = scenes.mc_settings(24, 1.0, vresampl_iters=1, vresampl_c=0.4, projection=1, qem=1)
    V = torch.from_numpy(v.reshape(-1).copy()).cuda()
    F = torch.from_numpy(f.reshape(-1).copy()).cuda()
    ob = impli.Ob02Shard(shape, mc)
    try:
        ob.load(V.data_ptr(), len(v), F.data_ptr(), len(f), v0, v1)
        ob.project()
        return ob.download()
    finally:
        ob.close()


@pytest.mark.parametrize("edit", np_ob02.EDITS)
def test_ob02_projection_qem_irregular_topology(impli, oracle, edit):
    """Projection and QEM on the resampled R = 24 mesh of config 2 with boundary edges, edges of three
    and four faces, faces with a repeated vertex (a zero-length edge in k_fold_walk, a zero facet
    normal among the search directions), a vertex in no face (an empty umbrella: it must not move)
    and fans that lift one vertex to valence 14, 15, 23 and 46 with ring vertices of valence 2 --
    both sides of k_qem's register umbrella (kUmbrellaRegs = 8) and its loop.  Vertices bit for bit the
    oracle's, which the CPU suite pins to float64 on these very meshes; faces unchanged."""
    s = oracle_stages(oracle, "edit_" + edit)
    v, f = s["pre"], s["faces"]
    vg, fg = _project_on_device(impli, scene("edit_" + edit)[0], v, f, 0, len(v))
    assert np.array_equal(fg, f)
    bad = np.flatnonzero(~_same_rows(vg, s["post"]))
    assert bad.size == 0, (edit, bad.size, bad[:10])
    err, _ = np_ob02.qem_errors(vg, s["ref"], M_RANK, M_CLAMP)
    assert err.max() <= qem_bound(oracle), (edit, err.max())
    if edit == "isolated":
        assert np.array_equal(_bits(vg[-1]), _bits(v[-1]))


def test_ob02_projection_qem_irregular_topology_owned_range(impli, oracle):
    """A shard that owns a strict subset [v0, v1) of fan17's vertices -- the hub inside, 8 of the 17
    ring vertices outside -- writes the oracle's values to the vertices it owns and leaves every
    other one as loaded."""
    s = oracle_stages(oracle, "edit_fan17")
    v, f = s["pre"], s["faces"]
    v0, v1 = 37, len(v) - 8
    assert v0 <= np_ob02.FAN_HUB < v1
    vg, fg = _project_on_device(impli, scene("edit_fan17")[0], v, f, v0, v1)
    assert np.array_equal(fg, f)
    own = np.zeros(len(v), bool)
    own[v0:v1] = True
    assert _same_rows(vg[own], s["post"][own]).all(), np.flatnonzero(own)[~_same_rows(vg[own], s["post"][own])][:10]
    assert np.array_equal(_bits(vg[~own]), _bits(v[~own]))
    assert (_bits(s["post"][~own]) != _bits(v[~own])).any()   # the oracle moves them: leaving them is the shard's doing
