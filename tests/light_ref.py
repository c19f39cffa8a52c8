"""Float64 restatement of the light side of a path vertex: the yardstick of test_lights_host.py (oracle) and test_gpu_lights.py (device).

Plain numpy from the PtrRect / environment arrays.  It shares nothing with the oracle or the kernels beyond the alias tables of the
environment sampler (held bitwise by test_env_tables_match_oracle_bitwise_and_hdr_loader) and the 24-bit random stream.
  environment   texel pdf p / (sin(theta) dTheta dPhi); the texel a triple of random numbers selects, its jittered direction and the
                rotation; the texel a direction looks its pdf up in - half a turn away from the texel it was drawn from (quirk Q2); the
                bilinear level-0 radiance (wrap in x, clamp in y)
  rectangles    the sampled point, d^2 / (A |cos| N), the Lambert NEE contribution E rho/pi cos / (pdf_light + cos/pi), the closed-form
                solid angle of the rectangle's two triangles (Van Oosterom and Strackee 1983), and - for the settled connections - the
                brute-force ray / rectangle test of traversal_ref.py over the lights alone
The discrete steps (alias lookups, texel of a direction) take float32 inputs and are evaluated with the float32 products the code
states, so that a texel choice is comparable at all; everything continuous is float64.
"""
import numpy as np

import traversal_ref as tr

PI = np.pi
ONE_MINUS = np.float32(0.99999994)


# ---------------------------------------------------------------- random stream (Rng::hash, 24-bit floats)
def rng_hash(x):
    x = np.asarray(x, np.uint64) & 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7feb352d) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846ca68b) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def rng_draw(states, count):
    """`count` floats per state: ([n, count] float64, each k / 2^24; the states afterwards [n] uint32)."""
    s = np.asarray(states, np.uint64)
    out = np.zeros((len(s), count))
    for k in range(count):
        s = rng_hash(s)
        out[:, k] = (s & 0xFFFFFF) / 16777216.0
    return out, s.astype(np.uint32)


# ---------------------------------------------------------------- environment
def env_texel_pdf(rgba):
    """[H, W] solid-angle pdf of every texel: p / (sin(theta) dTheta dPhi), p = luminance x cell / their sum."""
    rgba = np.asarray(rgba, np.float64)
    h, w = rgba.shape[:2]
    lum = 0.2126 * rgba[..., 0] + 0.7152 * rgba[..., 1] + 0.0722 * rgba[..., 2]
    cell = np.maximum(np.sin((np.arange(h) + 0.5) * PI / h), 0.0) * (PI / h) * (2.0 * PI / w)
    # a negative texel weighs nothing; one that is no number stays no number (max(lum, 0) keeps a NaN), makes the sum and with it every
    # pdf no number, and a pdf that is no positive number reads as 0: such a map is never sampled from, nor weighted by
    with np.errstate(invalid="ignore"):
        weight = np.where(lum < 0.0, 0.0, lum) * cell[:, None]
        pdf = weight / weight.sum() / cell[:, None]
    return np.where(np.isfinite(pdf) & (pdf > 0.0), pdf, 0.0)


def env_select(tables, u):
    """The texel (row, col) and the x jitter the code derives from u [n, 3] float32 {marginal, conditional, jitter}; the products and
    differences are the code's float32 ones (each a single IEEE operation)."""
    u = np.minimum(np.maximum(np.asarray(u, np.float32), np.float32(0)), ONE_MINUS)
    h, w = tables["cond_threshold"].shape
    row_choice = u[:, 0] * np.float32(h)
    row = np.minimum(row_choice.astype(np.uint32), h - 1)
    alias = (row_choice - row.astype(np.float32)) >= tables["marg_threshold"][row]
    row = np.where(alias, np.minimum(tables["marg_alias"][row], h - 1), row).astype(np.int64)
    col_choice = u[:, 1] * np.float32(w)
    col = np.minimum(col_choice.astype(np.uint32), w - 1)
    alias = (col_choice - col.astype(np.float32)) >= tables["cond_threshold"][row, col]
    col = np.where(alias, np.minimum(tables["cond_alias"][row, col], w - 1), col).astype(np.int64)
    return row, col, u[:, 1].astype(np.float64), u[:, 2].astype(np.float64)


def env_direction(row, col, jitter_x, jitter_y, w, h, rotation):
    """World direction of the point (col + jx, row + jy) of the map, float64."""
    theta = (row + jitter_y) / h * PI
    phi = (col + jitter_x) / w * 2.0 * PI
    m = np.stack([np.sin(theta) * np.cos(phi), np.cos(theta), np.sin(theta) * np.sin(phi)], axis=1)
    c, s = np.cos(float(rotation)), np.sin(float(rotation))
    return np.stack([m[:, 0] * c + m[:, 2] * s, m[:, 1], -m[:, 0] * s + m[:, 2] * c], axis=1)


def env_uv(directions, rotation):
    """(u, v) a world direction looks the map up at (float64): u = (atan2(z, x) + pi) / 2 pi of the direction rotated into the map."""
    d = np.asarray(directions, np.float64)
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    c, s = np.cos(float(rotation)), np.sin(float(rotation))
    x, y, z = d[:, 0] * c - d[:, 2] * s, d[:, 1], d[:, 0] * s + d[:, 2] * c
    return (np.arctan2(z, x) + PI) / (2.0 * PI), 0.5 - np.arcsin(np.clip(y, -1.0, 1.0)) / PI


def env_lookup_texel(directions, rotation, w, h):
    """(row, col) of the texel whose pdf a direction reads, and how far (in texels) (u W, v H) lies from the nearest texel border."""
    u, v = env_uv(directions, rotation)
    u, v = np.clip(u, 0.0, float(ONE_MINUS)), np.clip(v, 0.0, float(ONE_MINUS))
    fu, fv = u * w, v * h
    col, row = np.minimum(fu.astype(np.int64), w - 1), np.minimum(fv.astype(np.int64), h - 1)
    border = np.minimum(np.abs(fu - np.round(fu)), np.abs(fv - np.round(fv)))
    return row, col, border


def env_half_turn_texel(row, col, jitter_x, w):
    """Quirk Q2 in float64: the direction drawn from (col + jx) / W reads its pdf at u + 1/2 (mod 1), the same row."""
    u = ((col + jitter_x) / w + 0.5) % 1.0
    return row, np.minimum((u * w).astype(np.int64), w - 1), np.abs(u * w - np.round(u * w))


def env_bilinear(rgba, directions, rotation, intensity):
    """Level-0 radiance along directions: bilinear with texel centres at (i + 0.5), wrap in x, clamp in y."""
    rgba = np.asarray(rgba, np.float64)
    h, w = rgba.shape[:2]
    u, v = env_uv(directions, rotation)
    fx, fy = u * w - 0.5, v * h - 0.5
    x0, y0 = np.floor(fx).astype(np.int64), np.floor(fy).astype(np.int64)
    tx, ty = (fx - x0)[:, None], (fy - y0)[:, None]
    xa, xb = x0 % w, (x0 + 1) % w
    ya, yb = np.clip(y0, 0, h - 1), np.clip(y0 + 1, 0, h - 1)
    c0 = rgba[ya, xa, :3] * (1 - tx) + rgba[ya, xb, :3] * tx
    c1 = rgba[yb, xa, :3] * (1 - tx) + rgba[yb, xb, :3] * tx
    return (c0 * (1 - ty) + c1 * ty) * max(float(intensity), 0.0)


# ---------------------------------------------------------------- rectangle lights
class Lights:
    """The rectangle lights of a scene description, as float64 arrays: the rectangles whose material is a diffuse light with non-zero
    emission, in rectangle order."""

    def __init__(self, desc, emission_scale=1.0):
        rows = []
        for i in range(desc.rectCount):
            r = desc.rects[i]
            m = desc.materials[min(r.materialTwoSided[0], desc.materialCount - 1)]
            e = np.array(list(m.emission)[:3], np.float64) * emission_scale
            if int(m.typeEta[0]) != 3 or not (e @ e > 0.0):
                continue
            rows.append((i, list(r.corner)[:3], list(r.edgeU)[:3], list(r.edgeV)[:3], list(r.normalAndPlane)[:3], r.materialTwoSided[1] != 0, e))
        self.rect = np.array([r[0] for r in rows], np.int64)
        self.corner, self.eu, self.ev, nrm = (np.array([r[k] for r in rows], np.float64).reshape(-1, 3) for k in (1, 2, 3, 4))
        self.normal = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
        self.two_sided = np.array([r[5] for r in rows], bool)
        self.emission = np.array([r[6] for r in rows], np.float64).reshape(-1, 3)
        self.area = np.linalg.norm(np.cross(self.eu, self.ev), axis=1)
        self.count = len(rows)

    def sample(self, position, u):
        """u [n, 3] {pick, lu, lv} at positions [n, 3]: dict of light, point, direction, distance, cos (signed, at the light), pdf (solid
        angle, with the 1/N pick; 0 where the sample is rejected)."""
        p = np.asarray(position, np.float64)
        # (the pick multiplies a 24-bit float by N in float32)
        sel = np.minimum((np.asarray(u[:, 0], np.float32) * np.float32(self.count)).astype(np.int64), self.count - 1)
        point = self.corner[sel] + u[:, 1:2] * self.eu[sel] + u[:, 2:3] * self.ev[sel]
        to = point - p
        d2 = np.einsum("ij,ij->i", to, to)
        dist = np.sqrt(d2)
        with np.errstate(invalid="ignore", divide="ignore"):
            direction = to / dist[:, None]
            cos = -np.einsum("ij,ij->i", direction, self.normal[sel])
            seen = np.where(self.two_sided[sel], np.abs(cos), cos)
            pdf = d2 / (self.area[sel] * np.maximum(seen, 1e-6) * self.count)
        ok = (d2 > 0) & (self.area[sel] > 0) & (seen > 0) & np.isfinite(pdf)
        return {"light": sel, "point": point, "direction": direction, "distance": dist, "cos": cos, "pdf": np.where(ok, pdf, 0.0), "ok": ok}

    def lambert_contribution(self, s, normal, wo, albedo):
        """E rho/pi cos(theta) / (pdf_light + cos(theta)/pi) of the samples of sample() at shading normals [n, 3] seen from wo (firefly
        clamp off, throughput 1): [n, 3], zero where nothing contributes (the light or the viewer under the shading normal's horizon)."""
        normal = np.asarray(normal, np.float64)
        cos = np.maximum(np.einsum("ij,ij->i", normal, np.nan_to_num(s["direction"])), 0.0)
        ok = s["ok"] & (cos > 0) & (np.einsum("ij,ij->i", normal, np.asarray(wo, np.float64)) > 0)
        with np.errstate(invalid="ignore", divide="ignore"):
            k = cos / (s["pdf"] + cos / PI) / PI
        return np.where(ok[:, None], self.emission[s["light"]] * np.asarray(albedo, np.float64)[None] * k[:, None], 0.0), ok

    def pdf_for_point(self, light, point, origin):
        """d^2 / (A |cos| N) of `point` on light `light` seen from origin (0 behind a one-sided light)."""
        to = np.asarray(point, np.float64) - np.asarray(origin, np.float64)
        d2 = np.einsum("ij,ij->i", to, to)
        with np.errstate(invalid="ignore", divide="ignore"):
            cos = -np.einsum("ij,ij->i", to / np.sqrt(d2)[:, None], self.normal[light])
            seen = np.where(self.two_sided[light], np.abs(cos), cos)
            pdf = d2 / (self.area[light] * np.maximum(seen, 1e-6) * self.count)
        return np.where((d2 > 0) & (seen > 0) & (self.area[light] > 0), pdf, 0.0)

    def solid_angle(self, light, position):
        """Closed-form solid angle of rectangle `light` from positions [n, 3]: its two triangles by Van Oosterom and Strackee."""
        p = np.asarray(position, np.float64)
        c, eu, ev = self.corner[light], self.eu[light], self.ev[light]
        quad = [c - p, c + eu - p, c + eu + ev - p, c + ev - p]
        total = np.zeros(len(p))
        for a, b, d in ((quad[0], quad[1], quad[2]), (quad[0], quad[2], quad[3])):
            la, lb, ld = (np.linalg.norm(x, axis=1) for x in (a, b, d))
            num = np.einsum("ij,ij->i", a, np.cross(b, d))
            den = la * lb * ld + np.einsum("ij,ij->i", a, b) * ld + np.einsum("ij,ij->i", a, d) * lb + np.einsum("ij,ij->i", b, d) * la
            total += np.abs(2.0 * np.arctan2(num, den))
        return total


class Reference(tr.Reference):
    """traversal_ref.Reference whose edge margin knows slivers.  A barycentric coordinate moves by (position error) / (the triangle's
    altitude over that edge): traversal_ref takes the square root of the area for that length, which is right for triangles about as
    wide as long and 63 times too long for the halves of a light 1e-3 wide and 4 long - there a ray whose float32 origin (ulp 5e-7 at
    x = 5) puts it 5e-7 outside the long edge would count as decided.  Here the length is the smallest altitude, area / longest edge."""

    def extent(self):
        longest = np.maximum(np.maximum(np.linalg.norm(self.e1, axis=1), np.linalg.norm(self.e2, axis=1)), np.linalg.norm(self.e2 - self.e1, axis=1))
        return np.maximum(np.linalg.norm(self.n, axis=1), 1e-300) / np.maximum(longest, 1e-300)


def light_reference(desc, lights):
    """Reference over the triangles of the rectangle lights alone (the brute-force test nearestRectLight is held to); its `light` array
    maps a triangle to its light index."""
    full = Reference(desc)
    keep = (full.src[:, 0] == 2) & np.isin(full.src[:, 2], lights.rect)
    ref = Reference.__new__(Reference)
    ref.tri, ref.src, ref.sph = full.tri[keep], full.src[keep], np.zeros((0, 4))
    ref.v0, ref.e1, ref.e2, ref.n = full.v0[keep], full.e1[keep], full.e2[keep], full.n[keep]
    ref.light = np.searchsorted(lights.rect, ref.src[:, 2])
    return ref


def connection_contribution(emission, pdf, weight, bsdf_pdf, throughput):
    """The specular connection's contribution (E:2856-2917) in float64, firefly clamp off: throughput x weight x E x mis / pdf with the pdf
    floors 1e-4, 1 / pdf capped at 1e4 and mis = pdf / (pdf + bsdf pdf) held to [1e-4, 0.9999]; zero where pdf is 0."""
    lp, bp = np.maximum(pdf, 1e-4), np.maximum(bsdf_pdf, 1e-4)
    mis = np.clip(lp / (lp + bp), 1e-4, 0.9999)
    c = np.asarray(throughput) * np.asarray(weight) * np.asarray(emission) * (mis * np.minimum(1.0 / lp, 1e4))[:, None]
    return np.where((np.asarray(pdf) > 0)[:, None], np.maximum(c, 0.0), 0.0)


def env_pdf_candidates(texel_pdf, directions, rotation, band=1e-4):
    """The pdfs a direction may read: that of its lookup texel, and of the neighbours it lies within `band` texels of (float32 cannot
    place a direction on one side of a border it is that close to): [n, 4], the first column the float64 texel; and the border distance (0 for a
    direction straight up or down, whose u is 0, 1/2 or 1 by the signs of its zeros)."""
    h, w = texel_pdf.shape
    u, v = env_uv(directions, rotation)
    out = []
    for du in (0.0, -band, band):
        for dv in (0.0, -band, band):
            uu = np.clip(np.clip(u, 0.0, float(ONE_MINUS)) * w + du, 0.0, None)
            vv = np.clip(np.clip(v, 0.0, float(ONE_MINUS)) * h + dv, 0.0, None)
            # u is periodic: a direction within the band of the seam may land on u = 0 or on u ~ 1 (clamped to the last column)
            out.append(texel_pdf[np.minimum(vv.astype(np.int64), h - 1), np.minimum(uu.astype(np.int64), w - 1)])
    d = np.asarray(directions, np.float64)
    pole = (d[:, 0] == 0) & (d[:, 2] == 0)   # straight up or down: u is whatever the signs of the zeros make it
    row = np.minimum((np.clip(v, 0.0, float(ONE_MINUS)) * h).astype(np.int64), h - 1)
    seam = ((np.minimum(u, 1.0 - u) * w) < band) | pole
    out.append(np.where(seam, texel_pdf[row, 0], out[0]))
    out.append(np.where(seam, texel_pdf[row, w - 1], out[0]))
    out.append(np.where(pole, texel_pdf[row, w // 2], out[0]))
    border = env_lookup_texel(directions, rotation, w, h)[2]
    return np.stack(out, axis=1), np.where(pole, 0.0, border)
