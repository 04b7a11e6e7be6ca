"""Record the interval pass's pruning power (needs the GPU): for every tree of the matrix-family field
tests (tests/test_gpu_matrices.py OBJECTS) at R = 32, the number of bricks the pass classes mixed
(Slab.brick_stats()[1]) next to the number of interior bricks that truly hold both signs.

    python tests/golden/make_prune_power.py [out.json]     (default: tests/golden/prune_power.json)

tests/test_gpu_intervals.py::test_pruning_power_not_worse_than_recorded then asserts
true mixed <= mixed <= recorded.  Run it again, and commit the result, only when a change of the
interval evaluator lowers a count on purpose; a count that rises is a regression of the bounds."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))


def main():
    try:
        import torch
        torch.cuda.is_available()
    except Exception:
        pass
    import implisolid_amd as I
    from test_gpu_intervals import OBJECTS, pruning_counts
    out = {"R": 32, "box": 1.0, "mixed_bricks_r32": {}, "true_mixed_interior_bricks_r32": {}, "bricks": {}}
    for name in sorted(OBJECTS):
        true_mixed, mixed, bricks = pruning_counts(I, OBJECTS[name])
        assert true_mixed <= mixed, (name, true_mixed, mixed)
        out["mixed_bricks_r32"][name] = mixed
        out["true_mixed_interior_bricks_r32"][name] = true_mixed
        out["bricks"][name] = bricks
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "prune_power.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
