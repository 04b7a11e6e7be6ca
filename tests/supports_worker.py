"""Worker of tests/test_gpu_supports.py::test_feet_across_forced_chunks.

Launched as ``python tests/supports_worker.py OUT ITEMS``: a process of its own makes the implisolid_layer_supports
calls of the foot cases of support_inputs (the shelf stack and the same shape on repeated, unsorted planes, at every
cell of FOOT_CELLS) with IMPLISOLID_SUPPORTS_CHUNK = ITEMS set before the library is loaded, and writes the tips,
the offsets, the layer records and the statistics of each call to OUT (.npz).
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main():
    out_path, items = sys.argv[1], sys.argv[2]
    os.environ["IMPLISOLID_SUPPORTS_CHUNK"] = items
    import numpy as np
    try:   # torch's HIP runtime first, as in tests/conftest.py
        import torch
        torch.cuda.is_available()
    except Exception:
        pass
    import implisolid_amd as I
    import support_inputs as si

    out = {}
    for name in sorted(si.FEET):
        if name == "shelf_reordered":
            bits, node, rect, z = si.painted_reordered()
        else:
            bits = si.FEET[name]()
            node, rect, z = si.painted(bits)
        L, H, W = bits.shape
        for cell in si.FOOT_CELLS:
            tips, offs, recs, stats = I.layer_supports(node, rect, W, H, z, cell, return_stats=True)
            key = "%s_%d_" % (name, cell)
            out[key + "tips"], out[key + "offs"], out[key + "recs"], out[key + "stats"] = tips, offs, recs, np.asarray(stats, np.int64)
    np.savez(out_path, **out)
    I.jit_wait()   # no compile in flight at exit


if __name__ == "__main__":
    main()
