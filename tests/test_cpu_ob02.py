"""CPU suite, OB02 stages: the oracle's QEM (or_ob02.c qem_vertex / jacobi_svd3, a restatement of
Eigen's JacobiSVD<Matrix3f>) against the float64 reference of the operation (tests/np_ob02.py,
numpy.linalg.svd).  This fixes the tolerance that tests/test_gpu_ob02_stages.py holds the device
to, and shows that the reference is right before any GPU run."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import np_ob02  # noqa: E402

M_RANK = 1e-3    # the f32 accumulation error of A is a few ulp of S_0, magnified 680-fold at the threshold
M_CLAMP = 1e-4
EITHER_WAY_CAP = 0.01
BOUND_CEILING = 1e-3     # in units of the average edge: a wrong rank, sign or order moves a vertex far more

MC_SCENES = ["config2_24", "config2_32", "config3_32"]
SCENES = MC_SCENES + ["edit_" + e for e in np_ob02.EDITS]


def scene(name):
    """-> (shape, R, edit or None); every scene uses the box [-1, 1]^3."""
    from implisolid_amd import scenes
    if name.startswith("edit_"):
        return scenes.union_sphere_cube(), 24, name[5:]
    cfg, R = name.split("_")
    return (scenes.union_sphere_cube() if cfg == "config2" else scenes.config3_tree()), int(R), None


_STAGES = {}


def oracle_stages(oracle, name):
    """Marching cubes, one resampling (c = 0.4), the scene's edit, then the projection with QEM, all
    by the oracle; the normals are its gradients at the projected centroids over their f32 norm.
    Computed once per scene and shared (read only)."""
    if name not in _STAGES:
        shape, R, edit = scene(name)
        tree = oracle.mp5_to_nodes(json.dumps(shape))
        v, f = oracle.marching_cubes(tree, R, [-1, 1] * 3)
        v, _ = oracle.vertex_resampling(tree, v, f, 0.4)
        if edit:
            v, f = np_ob02.edit_mesh(v, f, edit)
        v_post, cen, avg32 = oracle.centroids_projection(tree, v, f, 1)
        nrm = np_ob02.unit_normals_f32(oracle.eval_gradient(tree, cen))
        ref = np_ob02.QemReference(v, f, cen, nrm, np_ob02.average_edge(v, f))
        for a in (v, f, cen, v_post, nrm):
            a.setflags(write=False)
        _STAGES[name] = {"tree": tree, "pre": v, "faces": f, "centroids": cen, "post": v_post, "avg32": avg32,
                         "normals": nrm, "ref": ref}
    return _STAGES[name]


def oracle_errors(oracle, name):
    s = oracle_stages(oracle, name)
    return np_ob02.qem_errors(s["post"], s["ref"], M_RANK, M_CLAMP)


_BOUND = []


def qem_bound(oracle):
    """4 x the oracle's worst error against float64 over all scenes (units of the average edge): the
    margin covers a different but equally valid f32 rounding order.  Measured, not written down; a
    bound at or above BOUND_CEILING means the oracle itself is off, and no comparison may lean on it."""
    if not _BOUND:
        _BOUND.append(4.0 * max(float(oracle_errors(oracle, n)[0].max()) for n in SCENES))
    assert 0 < _BOUND[0] < BOUND_CEILING, _BOUND[0]
    return _BOUND[0]


def test_qem_bound_is_tight(oracle):
    """The bound every QEM comparison uses, 4 x the oracle's worst error, stays below 1e-3 of the
    average edge length.

    Measured (oracle vs float64, worst error / avg; the same figures with no "either way" allowance
    at all): config2_24 1.45e-5, config2_32 1.80e-5, config3_32 4.06e-5; edits boundary 8.29e-6,
    nonmanifold 1.49e-5, degenerate 1.97e-5, isolated 1.45e-5, fan8 1.34e-5, fan9 1.40e-5, fan17 1.57e-5,
    fan40 1.35e-5.  Bound = 4 x 4.06e-5 = 1.63e-4.

    Mutants of or_ob02.c (each run once against this file; all fail here and in every scene's test):
    rank threshold 1/600 -> worst 0.27 avg (config3_32: 1.07 avg); no sign fix-up of U -> worst 1.6 to
    2.9 avg in every scene; no sort of the singular values -> non-finite vertices in every scene."""
    worst = {n: float(oracle_errors(oracle, n)[0].max()) for n in SCENES}
    print("oracle vs float64, worst error / avg:", {n: "%.3g" % e for n, e in worst.items()})
    assert 0 < 4.0 * max(worst.values()) < BOUND_CEILING, worst
    print("bound %.4g" % qem_bound(oracle))
    for n in SCENES:       # the allowance is not what makes the oracle pass
        s = oracle_stages(oracle, n)
        strict, _ = np_ob02.qem_errors(s["post"], s["ref"], 0.0, 0.0)
        assert strict.max() <= qem_bound(oracle), (n, strict.max(), worst[n])


@pytest.mark.parametrize("name", SCENES)
def test_oracle_qem_matches_float64(oracle, name):
    """Every vertex the oracle's QEM writes is the float64 minimum-norm step's, within the bound, at
    the reference's rank and clamp branch -- or, for a vertex within M_RANK / M_CLAMP of a decision's
    threshold, at the neighbouring one.  Every scene reaches ranks 1, 2 and 3 and the clamp.

    Measured: rank 1 / 2 / 3 and clamped vertices -- config2_24 1296 / 237 / 433, 15; config2_32
    2482 / 572 / 476, 20; config3_32 196 / 526 / 556, 68; the edits as config2_24 plus their own
    vertices (isolated: one of rank 0; fanN: N ring vertices of rank 1).  "Either way" share: 7 of 3530
    vertices (0.20 %) at config2_32, whose closest rank decision lies 6.5e-4 from its threshold, and
    0 in every other scene (closest 1.6e-3; closest clamp decision 1.8e-3, config3_32).  99th
    percentile of the error 5e-6 to 7e-6 avg."""
    s = oracle_stages(oracle, name)
    ref = s["ref"]
    err, either = oracle_errors(oracle, name)
    ranks = np.bincount(ref.rank, minlength=4)
    print(name, "verts", len(err), "ranks 0..3", ranks.tolist(), "clamped", int(ref.clamped.sum()),
          "worst %.3g p99 %.3g" % (err.max(), np.percentile(err, 99)), "either-way %d" % either.sum(),
          "closest rank margin %.3g clamp margin %.3g" % (ref.rank_margin.min(), ref.clamp_margin.min()),
          "valence max", int(ref.valence.max()))
    assert np.isfinite(s["post"]).all() and ref.finite.all()
    assert ranks[1] > 0 and ranks[2] > 0 and ranks[3] > 0, ranks
    assert ref.clamped.any()
    assert abs(s["avg32"] / ref.avg - 1.0) < 3 * len(s["faces"]) * 2.0 ** -24   # a sequential f32 sum of 3 nf terms
    assert either.mean() <= EITHER_WAY_CAP, either.sum()
    bad = np.flatnonzero(~(err <= qem_bound(oracle)))
    assert bad.size == 0, (bad.size, bad[:10], err[bad[:10]], ref.rank[bad[:10]])


def test_edits_reach_the_umbrella_paths(oracle):
    """The edited meshes hold what marching cubes never makes: valence 1 and 2, valences on both sides
    of the device's register umbrella (8) and far above it, an empty umbrella of rank 0 that stays
    put, and a vertex listed twice by one face."""
    base = oracle_stages(oracle, "config2_24")["ref"].valence
    hub0 = int(base[np_ob02.FAN_HUB])
    for n in (8, 9, 17, 40):
        s = oracle_stages(oracle, "edit_fan%d" % n)
        val = s["ref"].valence
        assert val[np_ob02.FAN_HUB] == hub0 + n and (val[-n:] == 2).all()
    assert hub0 <= 8 < hub0 + 8
    s = oracle_stages(oracle, "edit_isolated")
    assert s["ref"].valence[-1] == 0 and s["ref"].rank[-1] == 0
    assert np.array_equal(s["post"][-1].view(np.uint32), s["pre"][-1].view(np.uint32))
    assert np.array_equal(s["ref"].verts[-1], s["pre"][-1].astype(np.float64))
    assert oracle_stages(oracle, "edit_boundary")["ref"].valence.min() >= 1
    assert oracle_stages(oracle, "edit_boundary")["ref"].valence.min() < base.min()


def test_reference_step_solves_the_normal_equations():
    """The float64 reference against its own definition on planes that meet in a known point: three
    independent planes give rank 3 and the point itself; two give rank 2 and the nearest point of
    their line; one gives rank 1 and the foot on the plane; a long step is cut to 1.5 avg."""
    verts = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    target = np.array([0.03, -0.02, 0.05])
    nrm = np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]])
    # vertex 0 lies in faces 0, 1, 2; vertex 1 in faces 0, 1; vertex 2 in face 0 only
    faces = np.array([[0, 1, 2], [0, 1, 3], [0, 3, 3]])
    cen = np.tile(target, (3, 1))
    out, rank, m_rank, m_clamp = np_ob02.qem_reference(verts, faces, cen, nrm, 10.0)
    assert rank.tolist() == [3, 2, 1, 2]
    assert np.allclose(out[0], target, atol=1e-15)
    assert np.allclose(out[1], [0.03, -0.02, 0.0], atol=1e-15)
    assert np.allclose(out[2], [0.03, 1.0, 0.0], atol=1e-15)
    short, *_ = np_ob02.qem_reference(verts, faces, cen, nrm, 0.01)
    step = np.linalg.norm(short[0] - verts[0])
    assert abs(step - 0.015) < 1e-15 and np.allclose((short[0] - verts[0]) / step, target / np.linalg.norm(target))
