"""Edge cases of the brick eval kernel's bookkeeping (impli_eval_bricks, the JIT tree modules): the
mesh of small seeded trees against the oracle's marching cubes on the same tree -- vertices bit for
bit, faces equal -- with the JIT module asserted, so the interpreter cannot stand in for it.

Shapes: R = 21 (n = R + 3 = 24 stored samples per axis: whole bricks, an even layer count) and R = 30
(n = 33: the last brick column and row have lanes past the grid edge, and the last brick layer holds a
single stored layer -- the clamped z of the layer pair); one grid as two Z-slabs at an odd cut (a
slab whose first stored layer is not 0, the sealed-layer test, the halo layer); pruning level 1 (no
claims) and 2 (mixed bricks claim their sign-definite neighbours across faces in x, y and z); the
per-shape and the value-baked module; and the kernel compiled without its occupancy request.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED, LEAVES = 401, 6      # a heart, a double mushroom and a screw among the leaves (f64 constant paths)
BOX = [-1.0, 1.0] * 3
_REF = {}


def _tree():
    from implisolid_amd import scenes
    return scenes.random_tree(SEED, LEAVES, twist_leaves=True)


def _leaf_types(s):
    return {s["type"]} if "children" not in s else set().union(*[_leaf_types(c) for c in s["children"]])


def _reference(oracle, R):
    """The oracle's mesh of the tree at R, computed once and shared (read-only)."""
    if R not in _REF:
        v, f = oracle.marching_cubes(oracle.mp5_to_nodes(json.dumps(_tree())), R, BOX)
        v.setflags(write=False)
        f.setflags(write=False)
        _REF[R] = (v, f)
    return _REF[R]


def _same(v, f, ref):
    vr, fr = ref
    assert len(fr) > 0
    assert f.shape == fr.shape and np.array_equal(f, fr)
    assert v.shape == vr.shape and np.array_equal(v.view(np.uint32), vr.view(np.uint32))


def _slabs_mesh(impli, shape, mc, module, nranks=1, cuts=None, check_rank=0, evals=1):
    """The concatenated mesh of the grid's Z-slabs; slab check_rank must have run a JIT module, and
    one of the given kind where the library tells the kinds apart: jit_module() says "baked" only
    for a hot object's switch to its baked module (bake mode 2).  In bake mode 1 the slab's one
    module is generated with the values baked in (test_bake_mode_1_source_is_value_baked) and is
    reported as "shape"."""
    slabs = [impli.Slab(shape, mc, r, nranks, cuts=cuts) for r in range(nranks)]
    try:
        counts = []
        for s in slabs:
            for _ in range(evals):
                s.eval()
                impli.jit_wait()
            s.count()
            counts.append(s.counts()[:2])
        impli.jit_wait()
        assert slabs[check_rank].used_jit()
        assert slabs[check_rank].jit_module() == module
        voff = np.concatenate([[0], np.cumsum([c[0] for c in counts])])
        foff = np.concatenate([[0], np.cumsum([c[1] for c in counts])])
        vs, fs = [], []
        for r, s in enumerate(slabs):
            s.set_offsets(int(voff[r]), int(foff[r]))
            s.emit()
            nv, nf, overflow = s.counts()
            assert not overflow
            v, f = s.download(nv, nf)
            vs.append(v)
            fs.append(f)
    finally:
        for s in slabs:
            s.close()
    return np.concatenate(vs), np.concatenate(fs)


@pytest.fixture
def sync_jit(impli):
    impli.set_jit(1)          # compile before the first eval: the module, not the interpreter, runs
    yield impli
    impli.set_jit(2)
    impli.set_jit_bake(2)
    impli.set_pruning(2)


def test_tree_has_the_f64_leaves():
    assert {"iheart", "implicit_double_mushroom", "screw"} <= _leaf_types(_tree())


@pytest.mark.parametrize("bake", [0, 1])
@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("R", [21, 30])
def test_edges_against_oracle(sync_jit, oracle, R, level, bake):
    from implisolid_amd import scenes
    I = sync_jit
    I.set_jit_bake(bake)
    I.set_pruning(level)
    v, f = _slabs_mesh(I, _tree(), scenes.mc_settings(R, 1.0), "shape")
    _same(v, f, _reference(oracle, R))


def test_bake_mode_1_source_is_value_baked(sync_jit):
    """Bake mode 1 generates the object's module with its matrices as bit-pattern literals, mode 0
    with loads from the matrix array: the bake = 1 cases here run other code than the bake = 0 ones."""
    I = sync_jit
    src = {}
    for bake in (0, 1):
        I.set_jit_bake(bake)
        src[bake] = I.jit_compile(_tree())[2]
    assert "__builtin_bit_cast(float, 0x" in src[1] and "__builtin_bit_cast(float, 0x" not in src[0]
    assert "impli_eval_bricks" in src[0] and "impli_eval_bricks" in src[1]


def test_hot_object_switches_to_its_baked_module(sync_jit, oracle):
    """Bake mode 2 (the default, what the benchmark runs): an object evaluated repeatedly gets its
    baked module, and the engine says so; the mesh from it is the oracle's."""
    from implisolid_amd import scenes
    I = sync_jit
    I.set_jit_bake(2)
    v, f = _slabs_mesh(I, _tree(), scenes.mc_settings(30, 1.0), "baked", evals=8)
    _same(v, f, _reference(oracle, 30))


def test_level2_has_sign_filled_bricks_beside_mixed_ones(sync_jit):
    """What the claim path needs is there at level 2: the R = 30 grid has mixed bricks and sign-filled
    ones (candidates are sign-filled neighbours of mixed bricks).  Whether a claim was made is not
    counted here; a claim that went wrong shows in the level-2 mesh comparisons above."""
    from implisolid_amd import scenes
    I = sync_jit
    I.set_pruning(2)
    s = I.Slab(_tree(), scenes.mc_settings(30, 1.0))
    try:
        s.eval()
        bricks, mixed, filled = s.brick_stats()
    finally:
        s.close()
    assert 0 < mixed < bricks and filled > 0


@pytest.mark.parametrize("bake", [0, 1])
def test_two_slabs_at_an_odd_cut(sync_jit, oracle, bake):
    from implisolid_amd import scenes
    I = sync_jit
    I.set_jit_bake(bake)
    R = 30
    cuts = [1, 13, R + 3]
    v, f = _slabs_mesh(I, _tree(), scenes.mc_settings(R, 1.0), "shape", nranks=2, cuts=cuts, check_rank=1)
    _same(v, f, _reference(oracle, R))


_CHILD = """
import json, sys
import numpy as np
sys.path.insert(0, %r)
try:
    import torch
    torch.cuda.is_available()
except Exception:
    pass
import implisolid_amd as I
from implisolid_amd import scenes
I.set_jit(1)
I.set_jit_bake(1)
I.set_pruning(2)
shape = scenes.random_tree(%d, %d, twist_leaves=True)
s = I.Slab(shape, scenes.mc_settings(30, 1.0))
nv, nf = s.run()
I.jit_wait()
assert s.used_jit()
v, f = s.download(nv, nf)
s.close()
np.savez(sys.argv[1], v=v, f=f)
"""


def test_without_the_occupancy_request(oracle, tmp_path):
    """IMPLISOLID_EVAL_WAVES=0 is read when the source is generated: a fresh process."""
    out = str(tmp_path / "mesh.npz")
    env = dict(os.environ, IMPLISOLID_EVAL_WAVES="0", IMPLISOLID_JIT_CACHE=str(tmp_path / "cache"))
    subprocess.run([sys.executable, "-c", _CHILD % (ROOT, SEED, LEAVES), out], check=True, env=env, timeout=120)
    with np.load(out) as d:
        _same(d["v"], d["f"], _reference(oracle, 30))
