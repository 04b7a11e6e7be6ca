"""numpy restatement of the suction cups of the layer stack -- TEST INFRASTRUCTURE ONLY.

Written from the definition (include/implisolid.h implisolid_layer_cups), independent of the kernels:

  empty      a voxel (l, py, px) is empty iff cov[l][py][px] < threshold; the order of the layers is the print order
  adjacent   np_bodies' adjacency (connectivity 6 or 26) among the empty voxels
  prefix     P_l = layers 0 .. l; the plate below layer 0 and the film above layer l are closed
  frame      px in {0, W - 1} or py in {0, H - 1}
  pocket     a class of the transitive closure of adjacency among the empty voxels of P_l; open if it holds a frame
             voxel, else closed
  cup        the layer-l voxels of one closed pocket of P_l that has a voxel in layer l
  record     int64 {seed, area, x0, y0, x1, y1, pocket}: seed the smallest py W + px of the cup, pocket the smallest
             key l' W H + py W + px of the whole pocket; layer by layer in increasing seed, cup_offsets (L + 1,)
  run        a maximal sequence of empty voxels within one image row that lies in a cup: int32 {start = py W + x0,
             length, cup = the index of its record}; layer by layer in increasing start, run_offsets (L + 1,)

For each l it takes np_bodies.labels of the empty mask of cov[:l + 1] -- L separate component problems --, drops
the labels that own a frame voxel, and groups layer l's remaining voxels by label.
"""
import numpy as np

import np_bodies

FIELDS = ("seed", "area", "x0", "y0", "x1", "y1", "pocket")
RUN_FIELDS = ("start", "length", "cup")


def frame(H, W):
    f = np.zeros((H, W), bool)
    f[0, :] = f[H - 1, :] = True
    f[:, 0] = f[:, W - 1] = True
    return f


def cups(cov, threshold, connectivity):
    """cov uint8 (L, H, W) -> (cup_offsets int64 (L + 1,), records int64 (C, 7), run_offsets int64 (L + 1,), runs
    int32 (K, 3), decode int32 (L, H, W) = the voxel's cup index or -1, the empty row runs of the stack)"""
    empty = np.asarray(cov) < threshold
    L, H, W = empty.shape
    fr = frame(H, W)
    rec, runs, offs, roffs = [], [], [0], [0]
    decode = np.full((L, H, W), -1, np.int32)
    empty_runs = 0
    for l in range(L):
        lab = np_bodies.labels(empty[:l + 1], connectivity)   # the pockets of P_l, by their smallest key
        owners = np.unique(lab[:, fr])
        top = lab[l]
        closed = (top >= 0) & ~np.isin(top, owners[owners >= 0])
        py, px = np.nonzero(closed)
        of = top[py, px]
        index = {}
        for seed, pocket in sorted((int((py[of == u] * W + px[of == u]).min()), int(u)) for u in np.unique(of)):
            m = of == pocket
            index[pocket] = len(rec)
            rec.append([seed, int(m.sum()), px[m].min(), py[m].min(), px[m].max(), py[m].max(), pocket])
        on = empty[l]
        before = np.zeros_like(on)
        before[:, 1:] = on[:, :-1]
        after = np.zeros_like(on)
        after[:, :-1] = on[:, 1:]
        sy, sx = np.nonzero(on & ~before)   # row-major: row by row, left to right
        ey, ex = np.nonzero(on & ~after)    # the k-th end closes the k-th start
        assert np.array_equal(sy, ey) and (ex >= sx).all()
        empty_runs += len(sy)
        for y, a, b in zip(sy.tolist(), sx.tolist(), ex.tolist()):
            inside = closed[y, a:b + 1]
            assert inside.all() or not inside.any(), "a run lies in one pocket: it is cupped whole or not at all"
            if inside.all():
                assert (top[y, a:b + 1] == top[y, a]).all()
                runs.append([y * W + a, b - a + 1, index[int(top[y, a])]])
                decode[l, y, a:b + 1] = index[int(top[y, a])]
        offs.append(len(rec))
        roffs.append(len(runs))
    return (np.array(offs, np.int64), np.array(rec, np.int64).reshape(-1, 7), np.array(roffs, np.int64),
            np.array(runs, np.int32).reshape(-1, 3), decode, empty_runs)


def as_rows(a, fields=FIELDS):
    """a structured record array (implisolid_amd.CUP_DTYPE or CUP_RUN_DTYPE) as integers (n, fields)"""
    return np_bodies.as_rows(a, fields)
