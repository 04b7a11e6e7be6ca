"""Float64 references for the OB02 projection and QEM stages -- TEST INFRASTRUCTURE ONLY, numpy only.

The device QEM (ob02.hip k_qem / jacobi_svd3) and the oracle's (or_ob02.c qem_vertex / jacobi_svd3)
both restate Eigen's JacobiSVD<Matrix3f> line for line, so comparing one with the other cannot see
a misreading that both share.  This module states the *operation* instead, in float64 and with
numpy.linalg.svd: no sweep, no rotation, no sort and no sign fix-up of its own.

  qem_reference(verts, faces, centroids, normals, avg)
      per vertex v, over the faces that contain it (a face counts once per corner it holds v at,
      as make_neighbour_faces_of_vertex lists it):
          A = sum n n^T,  r = sum n n^T (c - v)
          U S V^T = svd(A);  rank = #{S_i >= S_0 / 680}  (0 when S_0 == 0)
          d = V_r diag(1 / S_r) U_r^T r                   the minimum-norm step
          if avg > 0 and |d| > avg: d *= min(1.5 avg, |d|) / |d|
      -> new vertices, ranks, and how far each of the two decisions lies from its threshold

  QemReference      the same, keeping the decomposition so that the step at a neighbouring rank or on
                    the other clamp branch can be formed (qem_errors' "either way" rule)
  qem_errors        the acceptance rule of tests/test_cpu_ob02.py
  edit_mesh         the meshes marching cubes never makes (boundary, non-manifold, degenerate,
                    isolated vertex, fans of valence 14 to 46)
  projection_invariants   what a projected centroid must satisfy whatever the search order
"""
import numpy as np

RANK_RATIO = 680.0                      # qem.hpp: svd.setThreshold(1.0 / 680.0)
ROOT_TOLERANCE = np.float32(0.001 / 10.0)   # configs.hpp:33
# set_centers_on_surface's alpha list (make_alpha_list(avg, 0.001, avg, 20), centroids_projection.cpp:
# 144-194): steps avg/2, avg/4, ... with odd multiples i * step, i <= min(20, avg / step) -- the
# largest |alpha| is 15/16 (step avg/16, i = 15; at avg/32 the cap of 20 gives 19/32).  Every search
# direction has length <= 1 (normalised, or left alone below 1e-6), the bisection stays between the
# centroid and the bracket's far end, so no centroid moves further than 15/16 of the average edge.
MAX_ALPHA = 15.0 / 16.0

EDITS = ["boundary", "nonmanifold", "degenerate", "isolated", "fan8", "fan9", "fan17", "fan40"]
FAN_HUB = 100


def average_edge(verts, faces):
    """compute_average_edge_length (centroids_projection.cpp:70-82) in float64."""
    p = np.asarray(verts, np.float64)[np.asarray(faces)]
    e = (np.linalg.norm(p[:, 0] - p[:, 1], axis=1) + np.linalg.norm(p[:, 0] - p[:, 2], axis=1)
         + np.linalg.norm(p[:, 2] - p[:, 1], axis=1))
    return float(e.sum() / (3.0 * len(faces)))


def unit_normals_f32(grad):
    """normalize_1111 (normalise_inplace.hpp:60-70): each gradient divided by its float32 norm."""
    g = np.ascontiguousarray(grad, np.float32)
    nm = np.sqrt(g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1] + g[:, 2] * g[:, 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        return g / nm[:, None]


class QemReference:
    def __init__(self, verts, faces, centroids, normals, avg):
        v = np.asarray(verts, np.float64)
        f = np.asarray(faces, np.int64)
        c = np.asarray(centroids, np.float64)
        n = np.asarray(normals, np.float64)
        nv = len(v)
        self.v, self.avg = v, float(avg)
        A = np.zeros((nv, 3, 3))
        r = np.zeros((nv, 3))
        nnT = n[:, :, None] * n[:, None, :]
        for s in range(3):                      # corner s of every face: the face joins that vertex's umbrella
            vid = f[:, s]
            np.add.at(A, vid, nnT)
            np.add.at(r, vid, np.einsum("fij,fj->fi", nnT, c - v[vid]))
        self.valence = np.bincount(f.reshape(-1), minlength=nv)
        self.finite = np.isfinite(A).all((1, 2)) & np.isfinite(r).all(1) & np.isfinite(v).all(1)
        A[~self.finite] = 0.0
        r[~self.finite] = 0.0
        U, S, Vt = np.linalg.svd(A)
        self.U, self.S, self.Vt, self.r = U, S, Vt, r
        thr = S[:, 0] / RANK_RATIO
        self.rank = np.where(S[:, 0] > 0, (S >= thr[:, None]).sum(1), 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            m = np.abs(np.log(S / thr[:, None]))
        m[~np.isfinite(m)] = np.inf             # S_i == 0 (or S_0 == 0): no threshold anywhere near
        self.rank_margin = m.min(1)
        self.near_index = m.argmin(1)           # the singular value nearest the threshold
        self.d = self.step(self.rank)
        self.dlen = np.linalg.norm(self.d, axis=1)
        self.clamped = (self.avg > 0) & (self.dlen > self.avg)
        with np.errstate(divide="ignore", invalid="ignore"):
            self.clamp_margin = np.abs(self.dlen / self.avg - 1.0) if self.avg > 0 else np.full(nv, np.inf)
        self.verts = self.moved(self.d, self.clamped)

    def step(self, rank):
        """d = V_r diag(1 / S_r) U_r^T r at the given rank per vertex."""
        keep = np.arange(3)[None, :] < np.asarray(rank)[:, None]
        utr = np.einsum("vji,vj->vi", self.U, self.r)
        with np.errstate(divide="ignore", invalid="ignore"):
            y = np.where(keep, utr / self.S, 0.0)
        return np.einsum("vji,vj->vi", self.Vt, y)

    def moved(self, d, clamp):
        """v + d, with d rescaled to length min(1.5 avg, |d|) where clamp is set."""
        ln = np.linalg.norm(d, axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            k = np.where(clamp & (ln > 0), np.minimum(1.5 * self.avg, ln) / ln, 1.0)
        out = self.v + d * k[:, None]
        out[~self.finite] = np.nan
        return out

    def neighbour_rank(self):
        """The rank each vertex would get if the singular value nearest the threshold fell on the
        other side of it (singular values are sorted, so that is rank - 1 or rank + 1)."""
        flip_down = self.near_index < self.rank
        return np.clip(np.where(flip_down, self.rank - 1, self.rank + 1), 0, 3)

    def at_neighbour_rank(self):
        d = self.step(self.neighbour_rank())
        ln = np.linalg.norm(d, axis=1)
        return self.moved(d, (self.avg > 0) & (ln > self.avg))

    def at_other_clamp(self):
        return self.moved(self.d, ~self.clamped & (self.avg > 0))


def qem_reference(verts, faces, centroids, normals, avg):
    """-> (new vertices [nv, 3] f64, rank [nv], rank margin [nv], clamp margin [nv]);
    rank margin = min_i |ln(S_i / (S_0 / 680))|, clamp margin = | |d| / avg - 1 |."""
    q = QemReference(verts, faces, centroids, normals, avg)
    return q.verts, q.rank, q.rank_margin, q.clamp_margin


def qem_errors(out, ref, m_rank=1e-3, m_clamp=1e-4):
    """The acceptance rule.  Per vertex the error max |component difference| / avg of `out`
    against the reference at the reference's rank and clamp branch; a vertex whose rank decision
    lies within m_rank of its threshold may take the error against the neighbouring rank instead, one
    whose clamp decision lies within m_clamp the error against the other clamp branch.  Such "either
    way" vertices stay in the comparison.  Rows that are non-finite in the reference must be
    non-finite in `out` (error 0) and the other way round (error inf).

    -> (err [nv], either_way [nv] bool)"""
    out = np.asarray(out, np.float64)

    def err_to(t):
        with np.errstate(invalid="ignore"):
            e = np.abs(out - t).max(1) / ref.avg
        fin_o, fin_t = np.isfinite(out).all(1), np.isfinite(t).all(1)
        e = np.where(fin_o & fin_t, e, np.where(fin_o == fin_t, 0.0, np.inf))
        return e

    err = err_to(ref.verts)
    near_rank = ref.rank_margin < m_rank
    near_clamp = ref.clamp_margin < m_clamp
    if near_rank.any():
        err = np.where(near_rank, np.minimum(err, err_to(ref.at_neighbour_rank())), err)
    if near_clamp.any():
        err = np.where(near_clamp, np.minimum(err, err_to(ref.at_other_clamp())), err)
    return err, near_rank | near_clamp


# ---- meshes marching cubes never makes ----------------------------------------------------------
def edit_mesh(verts, faces, edit):
    """-> (verts f32, faces i32) of `edit` applied to a closed MC mesh:

    boundary     three faces removed (valence drops, boundary edges)
    nonmanifold  two faces repeated and one repeated reversed (edges of three and four faces)
    degenerate   two faces with a repeated vertex (zero-length edge, zero facet normal)
    isolated     one extra vertex in no face (empty umbrella: A = 0, rank 0, must not move)
    fanN         N ring vertices around vertex FAN_HUB and N faces (hub, ring_k, ring_k+1): the hub's
                 valence rises by N, the ring vertices have valence 2
    """
    v = np.ascontiguousarray(verts, np.float32).copy()
    f = np.ascontiguousarray(faces, np.int32).copy()
    if edit == "boundary":
        f = np.delete(f, [5, 17, 40], axis=0)
    elif edit == "nonmanifold":
        f = np.concatenate([f, f[[3, 9]], f[[20]][:, ::-1]])
    elif edit == "degenerate":
        f = np.concatenate([f, [[f[7, 0], f[7, 0], f[7, 1]], [f[11, 2], f[11, 1], f[11, 2]]]])
    elif edit == "isolated":
        v = np.concatenate([v, [[0.8125, -0.6875, 0.71875]]]).astype(np.float32)
    elif edit.startswith("fan"):
        n = int(edit[3:])
        hub = v[FAN_HUB].astype(np.float64)
        rad = 0.6 * average_edge(v, f)
        # a frame across the hub's outward direction (from the mesh's mean), so the fan lies near the surface
        out = hub - v.astype(np.float64).mean(0)
        out /= np.linalg.norm(out)
        e1 = np.cross(out, [0.3, 0.5, 0.81])
        e1 /= np.linalg.norm(e1)
        e2 = np.cross(out, e1)
        a = 2.0 * np.pi * np.arange(n) / n
        ring = hub + rad * (np.cos(a)[:, None] * e1 + np.sin(a)[:, None] * e2)
        base = len(v)
        v = np.concatenate([v, ring.astype(np.float32)])
        k = np.arange(n)
        f = np.concatenate([f, np.stack([np.full(n, FAN_HUB), base + k, base + (k + 1) % n], axis=1)])
    else:
        raise ValueError(edit)
    return np.ascontiguousarray(v, np.float32), np.ascontiguousarray(f, np.int32)


# ---- projection invariants ------------------------------------------------------------------------
def projection_invariants(c0, c, f_at_c, avg):
    """What set_centers_on_surface (centroids_projection.cpp:421-1214) guarantees for every face,
    whatever the order of its search: the centroid either stays where it was, bit for bit, or ends
    on a point with |f| <= ROOT_TOLERANCE (a trial that hit the band, or the bisection's last
    midpoint), no further than MAX_ALPHA * avg from where it started.

    c0, c: centroids before and after [nf, 3] f32; f_at_c: the implicit function at c, f32.
    -> dict(moved [nf] bool, moved_share, worst_f (over moved), worst_disp (in units of avg),
            disp_bound (same units), bad_f [nf] bool, bad_disp [nf] bool)"""
    c0 = np.ascontiguousarray(c0, np.float32)
    c = np.ascontiguousarray(c, np.float32)
    same = ((c0.view(np.uint32) == c.view(np.uint32)) | (np.isnan(c0) & np.isnan(c))).all(1)
    moved = ~same
    fa = np.abs(np.asarray(f_at_c, np.float32))
    with np.errstate(invalid="ignore"):
        bad_f = moved & ~(fa <= ROOT_TOLERANCE)
        disp = np.linalg.norm(c.astype(np.float64) - c0.astype(np.float64), axis=1) / avg
    # cc = avg_f32 * alpha and x + cc * d round once each (relative 2^-24 apiece, the direction's
    # normalisation a few more); each stored coordinate of c rounds to half an ulp of its magnitude
    eps = float(np.finfo(np.float32).eps)
    reach = float(np.nanmax(np.abs(c0))) if c0.size else 0.0
    disp_bound = MAX_ALPHA * (1.0 + 8.0 * eps) + 2.0 * eps * reach / avg
    with np.errstate(invalid="ignore"):
        bad_disp = moved & ~(disp <= disp_bound)
    with np.errstate(invalid="ignore"):
        on_surface = fa <= ROOT_TOLERANCE      # moved there, or was there already and stayed
    return {"moved": moved, "moved_share": float(moved.mean()) if len(moved) else 0.0,
            "on_surface_share": float(on_surface.mean()) if len(moved) else 0.0,
            "worst_f": float(fa[moved].max()) if moved.any() else 0.0,
            "worst_disp": float(np.nanmax(disp[moved])) if moved.any() else 0.0,
            "disp_bound": disp_bound, "bad_f": bad_f, "bad_disp": bad_disp}
