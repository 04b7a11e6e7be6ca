"""Worker of tests/test_gpu_cups.py::test_a_fresh_process_grows_its_arrays_chunk_by_chunk.

Launched as ``python tests/cups_grow_worker.py OUT CONNECTIVITY``: a process of its own, whose engine has handed out
no scratch yet, makes one implisolid_layer_cups call on the painted stack cup_inputs.growing with a layer per chunk
(IMPLISOLID_CUPS_CHUNK=1) and writes cup_offsets, the records, run_offsets, the run records and the statistics to
OUT (.npz).  The stack's five run arrays start empty there and take a larger block in most chunks, the earlier
chunks' entries copied over (test_cpu_cups.py restates the sizes); in the suite's own process the scratch that
earlier tests left is larger than any test stack needs.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    out_path, connectivity = sys.argv[1], int(sys.argv[2])
    os.environ["IMPLISOLID_CUPS_CHUNK"] = "1"   # below one layer's tiles: a layer per chunk
    import numpy as np
    try:   # torch's HIP runtime first, as in tests/conftest.py
        import torch
        torch.cuda.is_available()
    except Exception:
        pass
    import implisolid_amd as I
    import cup_inputs as cu
    import island_inputs as ii

    bits = cu.growing()
    L, H, W = bits.shape
    node, rect, z = ii.painted(bits)
    offs, cups, roffs, runs, stats = I.layer_cups(node, rect, W, H, z, 1, 1, connectivity, want_runs=True, return_stats=True)
    np.savez(out_path, offsets=offs, cups=cups, run_offsets=roffs, runs=runs, stats=np.asarray(stats, np.int64))
    I.jit_wait()   # no compile in flight at exit


if __name__ == "__main__":
    main()
