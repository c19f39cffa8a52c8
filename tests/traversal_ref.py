"""Float64 brute-force closest hit and any-hit over a scene's world-space primitives: the yardstick of the traversal tests.

Independent of the oracle's and of the kernels' arithmetic: every ray is tested against every primitive in float64, in chunks of rays.
The primitives are the ones the geometry bake makes out of a PtrSceneDesc (csrc/host/scene_geometry.cpp):
  * mesh triangles after their column-major localToWorld (ref_tinybvh.mesh_world_triangles, float32 like the bake);
  * rectangles as the builder's two triangles {c, c+u, c+v, c+u+v}, winding flipped to agree with the stored normal;
  * spheres, |radius|, with the Embree rule: the front root if it lies in [tmin, tmax], else the back root.
Besides the hit, every ray carries how close it came to a decision boundary, so a test can leave out the rays whose answer float32
arithmetic may legitimately flip: a barycentric margin (signed, relative to the triangle) of any triangle whose plane the ray meets inside
its interval, the distance of any candidate root to tmin / tmax, and the cosine between ray and surface at the hit.
"""
import numpy as np

import ref_tinybvh as rt

KIND_TRIANGLE, KIND_SPHERE = 0, 1


def world_primitives(desc):
    """(triangles [T, 3, 3] float64, triangle sources [T, 3] {primType (0 mesh, 2 rectangle), geomIndex, primIndex}, spheres [S, 4] float64
    {centre, |radius|})."""
    tris, src = [], []
    for mi in range(desc.meshCount):
        m = desc.meshes[mi]
        if m.vertexCount == 0 or m.indexCount == 0:
            continue
        w = rt.mesh_world_triangles(desc, mi)
        tris.append(w.astype(np.float64))
        src.append(np.stack([np.zeros(len(w)), np.full(len(w), mi), np.arange(len(w))], axis=1))
    for ri in range(desc.rectCount):
        r = desc.rects[ri]
        c, eu, ev = (np.array(list(v)[:3], np.float32) for v in (r.corner, r.edgeU, r.edgeV))
        n = np.array(list(r.normalAndPlane)[:3], np.float64)
        p = [c, c + eu, c + ev, (c + eu) + ev]
        flip = np.dot(np.cross(eu.astype(np.float64), ev.astype(np.float64)), n) < 0.0
        order = (0, 2, 1, 1, 2, 3) if flip else (0, 1, 2, 2, 1, 3)
        tris.append(np.array([[p[order[h * 3 + k]] for k in range(3)] for h in range(2)], np.float64))
        src.append(np.array([[2, 0, ri], [2, 0, ri]]))
    tri = np.concatenate(tris) if tris else np.zeros((0, 3, 3))
    srcs = np.concatenate(src).astype(np.int64) if src else np.zeros((0, 3), np.int64)
    sph = np.array([[s.centerRadius[0], s.centerRadius[1], s.centerRadius[2], abs(s.centerRadius[3])]
                    for s in (desc.spheres[i] for i in range(desc.sphereCount))], np.float64).reshape(-1, 4)
    return tri, srcs, sph


class Reference:
    """Brute-force float64 queries over one scene description."""

    def __init__(self, desc):
        self.tri, self.src, self.sph = world_primitives(desc)
        v0, v1, v2 = self.tri[:, 0], self.tri[:, 1], self.tri[:, 2]
        self.v0, self.e1, self.e2 = v0, v1 - v0, v2 - v0
        self.n = np.cross(self.e1, self.e2)

    def extent(self):
        """The length L per triangle that turns a position error into a barycentric one (see the margin's resolution in _chunk): the
        square root of the parallelogram's area, the edge length of a triangle that is about as wide as it is long."""
        return np.sqrt(np.maximum(np.linalg.norm(self.n, axis=1), 1e-300))

    def trace(self, rays, chunk=0):
        """rays [n, 8] float32 {o, tmin, d, tmax}.  Returns a dict of [n] arrays: t (inf on a miss), kind (-1 miss, 0 triangle, 1 sphere),
        index (triangle or sphere number), cos (|cos| between ray and normal at the hit), margin (the smallest |signed barycentric| of any
        triangle whose plane the ray crosses inside [tmin, tmax], and the relative |l^2 - r^2| of any sphere it grazes: small = the
        hit-or-miss answer hangs on rounding), near_ends (some root lies within 1e-6 relative of tmin or of a finite tmax)."""
        rays = np.asarray(rays, np.float32).reshape(-1, 8).astype(np.float64)
        n = rays.shape[0]
        chunk = chunk or max(8, min(512, int(1_500_000 // max(len(self.tri) + len(self.sph), 1))))
        res = {"t": np.full(n, np.inf), "kind": np.full(n, -1, np.int64), "index": np.full(n, -1, np.int64), "cos": np.zeros(n),
               "margin": np.full(n, np.inf), "near_ends": np.zeros(n, bool)}
        with np.errstate(all="ignore"):   # (parallel rays, degenerate triangles: NaN / inf that the masks drop)
            for a in range(0, n, chunk):
                self._chunk(rays[a:a + chunk], res, slice(a, min(a + chunk, n)))
        return res

    def _chunk(self, r, res, sl):
        o, tmin, d, tmax = r[:, None, 0:3], r[:, 3:4], r[:, None, 4:7], r[:, 7:8]
        dn = d[:, 0] / np.linalg.norm(d[:, 0], axis=1, keepdims=True)
        best = np.full(r.shape[0], np.inf)
        kind = np.full(r.shape[0], -1, np.int64)
        index = np.full(r.shape[0], -1, np.int64)
        cos = np.zeros(r.shape[0])
        margin = np.full(r.shape[0], np.inf)
        near = np.zeros(r.shape[0], bool)

        def ends(t):
            scale = np.maximum(np.abs(t), 1.0)
            return (np.abs(t - tmin) <= 1e-6 * scale) | (np.isfinite(tmax) & (np.abs(t - tmax) <= 1e-6 * scale))

        if len(self.tri):
            # Moeller-Trumbore in float64: o + t d = v0 + u e1 + v e2
            dd3 = np.broadcast_to(d, (r.shape[0], len(self.tri), 3))
            pv = np.cross(dd3, self.e2[None])
            den = np.einsum("tk,rtk->rt", self.e1, pv)
            tv = o - self.v0[None]
            qv = np.cross(tv, self.e1[None])
            with np.errstate(divide="ignore", invalid="ignore"):
                u = np.einsum("rtk,rtk->rt", tv, pv) / den
                v = np.einsum("rtk,rtk->rt", dd3, qv) / den
                t = np.einsum("tk,rtk->rt", self.e2, qv) / den
            w = 1.0 - u - v
            inside = (u >= 0) & (v >= 0) & (w >= 0) & (den != 0)
            live = np.isfinite(t) & (t > tmin) & (t <= tmax)
            hit = inside & live
            tt = np.where(hit, t, np.inf)
            k = np.argmin(tt, axis=1)
            tk = tt[np.arange(len(k)), k]
            better = tk < best
            best = np.where(better, tk, best)
            kind = np.where(better, KIND_TRIANGLE, kind)
            index = np.where(better, k, index)
            nk = self.n[k] / np.linalg.norm(self.n[k], axis=1, keepdims=True)
            cos = np.where(better, np.abs(np.einsum("rk,rk->r", nk, dn)), cos)
            # how close the answer is to flipping: signed barycentric margin of every triangle whose plane lies in the interval (or within
            # 1e-6 of its ends), and the ends themselves
            plane = np.isfinite(t) & (den != 0) & (t > tmin - 1e-6 * np.maximum(np.abs(t), 1)) & \
                (t <= tmax + 1e-6 * np.maximum(np.abs(t), 1))
            # (where float32 operands cannot resolve 1e-6 - a barycentric of a triangle of edge ~L from a ray whose coordinates are ~X is
            # known to about 8 * 2^-24 * X / (L |cos|) - the margin is counted in units of that resolution instead)
            nlen = np.maximum(np.linalg.norm(self.n, axis=1), 1e-300)[None]
            cosr = np.maximum(np.abs(den) / (nlen * np.linalg.norm(d, axis=2)), 1e-300)
            resol = np.maximum(1.0, 8.0 * 2.0 ** -24 * (np.abs(o).max(axis=2) + np.abs(self.v0).max(axis=1)[None]) / (self.extent()[None] * cosr) / 1e-6)
            m = np.abs(np.minimum(np.minimum(u, v), w)) / resol
            margin = np.minimum(margin, np.where(plane, m, np.inf).min(axis=1))
            near |= (inside & np.isfinite(t) & ends(t)).any(axis=1)
        if len(self.sph):
            ctr, rad = self.sph[None, :, 0:3], self.sph[None, :, 3]
            dd = np.einsum("rxk,rxk->rx", d, d)
            c0 = ctr - o
            proj = np.einsum("rtk,rxk->rt", c0, d) / dd
            perp = c0 - proj[..., None] * d
            l2 = np.einsum("rtk,rtk->rt", perp, perp)
            r2 = rad * rad
            ok = l2 <= r2
            td = np.sqrt(np.maximum(r2 - l2, 0.0) / dd)
            tf, tb = proj - td, proj + td
            vf = ok & (tmin <= tf) & (tf <= tmax)
            vb = ok & (tmin <= tb) & (tb <= tmax)
            ts = np.where(vf, tf, np.where(vb, tb, np.inf))
            k = np.argmin(ts, axis=1)
            tk = ts[np.arange(len(k)), k]
            better = tk < best
            best = np.where(better, tk, best)
            kind = np.where(better, KIND_SPHERE, kind)
            index = np.where(better, k, index)
            p = o[:, 0] + tk[:, None] * d[:, 0]
            nrm = p - self.sph[k, 0:3]
            with np.errstate(invalid="ignore", divide="ignore"):
                nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
            cos = np.where(better, np.abs(np.einsum("rk,rk->r", nrm, dn)), cos)
            margin = np.minimum(margin, (np.abs(r2 - l2) / r2).min(axis=1))
            near |= ((ok & ends(tf)) | (ok & ends(tb))).any(axis=1)
        res["t"][sl], res["kind"][sl], res["index"][sl], res["cos"][sl] = best, kind, index, cos
        res["margin"][sl], res["near_ends"][sl] = margin, near

    def occluded(self, rays, chunk=0):
        """Any-hit over [tmin, tmax]: the closest hit exists."""
        return np.isfinite(self.trace(rays, chunk)["t"])
