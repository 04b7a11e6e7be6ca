"""The reference rule for per-vertex normals (mcc2.cpp:852-871) in float32 numpy -- TEST
INFRASTRUCTURE ONLY.  The gradient comes from the oracle; the rule is written as
test_gpu_parity.test_direct_eval_abi_matches_reference_semantics writes it: the float norm, the
comparison with the double 0.0001, the quotient taken in double and rounded to float."""
import numpy as np


def normals_rule(g):
    """(normals float32 [n, 3], rows that took the -42 branch) of float32 gradients g [n, 3]."""
    g = np.ascontiguousarray(g, np.float32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        nrm = np.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1] + g[:, 2] * g[:, 2]).astype(np.float32)
        ok = nrm.astype(np.float64) > 0.0001   # the reference's double comparison; a NaN norm is false: -42
        fac = np.where(ok, (-1.0 / nrm.astype(np.float64)).astype(np.float32), np.float32(-42.0))
        n = (g * fac[:, None]).astype(np.float32)
    return n, int((~ok).sum())


def normals_ref(oracle, tree, verts):
    """oracle.eval_gradient at verts, then the rule: (normals, count of -42 rows)."""
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    if v.shape[0] == 0:
        return np.zeros((0, 3), np.float32), 0
    return normals_rule(oracle.eval_gradient(tree, v))


def same_bits(a, b):
    """Bit for bit, NaN rows matching by position (test_gpu_parity._same_bits)."""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())
