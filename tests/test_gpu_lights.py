"""The light side of a path vertex on the device, sample by sample: envSample / envLookup / envPdfOf, rectLightNee, rectLightPdfForHit and
the settled specular connections (nearestRectLight, rectLightSurface, rectContributionAt) through the probes of include/ptr_debug.h,
against the oracle's functions of the same name and against the float64 restatement of light_ref.py.

Device against oracle: discrete outputs (queued, found, light, half, ignore word, random state, table pdfs) are equal; continuous ones
agree to the suite's device-function tolerance, relative 2e-4 (test_gpu_parity.py: ocml against libm).  A sample where a last-ulp
difference flips a discrete choice - a direction on a texel border, a shadow ray that ends on the surface it is aimed at (quirk Q9), a
ray through a rectangle's rim - is counted, and at most 0.2 % of a batch may be such.  Device against float64: the bounds of
test_lights_host.py plus that 2e-4.  No bound here was taken from the device's output.

Held to the oracle only, because float64 cannot decide them: receivers exactly in a light's plane (the 'plane' class, 1/8 of each batch's
directed rays), directions straight up or down (3 per batch of directions), exact ties between the two coplanar overlapping lights.
"""
import numpy as np
import pytest

import light_ref as lr
import light_scenes as ls
import oracle_lib as ol
import test_lights_host as lh
import traversal_ref as tr

pt = ls.pt
pytestmark = pytest.mark.gpu

TOL = 2e-4    # device function against oracle function, relative
CAP = 0.002   # share of a batch whose discrete outcome may hang on a last-ulp difference
METAL = pt.PTR_METAL_SSS | pt.PTR_METAL_CLAMPS   # selects the Metal-semantics instantiation (and the clamped NEE weight)


def _with(s, **kw):
    s = s.copy()
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _rel(a, b, floor=0.0):
    """Largest |a - b| per row relative to the row's largest |b| (or floor)."""
    a, b = np.asarray(a, np.float64).reshape(len(a), -1), np.asarray(b, np.float64).reshape(len(b), -1)
    return np.abs(a - b).max(axis=1) / np.maximum(np.abs(b).max(axis=1), max(floor, 1e-300))


# ---------------------------------------------------------------- environment
@pytest.mark.parametrize("size,kind,rotation", lh.ENV_CASES)
def test_env_sampling_matches_oracle_and_float64(tmp_path, size, kind, rotation):
    w, h = ls.ENV_SIZES[size]
    host, rgba = ls.env_scene(tmp_path, ls.env_map(kind, w, h), "env")
    assert rgba.shape == (h, w, 4)
    dev = pt.DeviceScene(host.desc, 0, keepalive=host)
    s = _with(host.settings_for(), environmentRotation=rotation, environmentIntensity=1.5)
    tables = pt.debug_env_distribution(rgba)   # (the tables the device samples from: bitwise the oracle's, tests/test_host.py)
    u = ls.env_u(tables, 20000, 11)
    got = dev.env_sample(s, u)
    rc, out, look = ol.env_sample(rgba, rotation, 1.5, u)
    assert rc == 0
    what = "device %s %s %.2f" % (size, kind, rotation)
    # against the oracle: the same texel (its pdf is a table read), the same direction
    same = (got[:, 3] == out[:, 6]) & (np.abs(got[:, 0:3] - out[:, 0:3]).max(axis=1) <= TOL)
    print("%s: %d of %d samples pick another texel than the oracle" % (what, int((~same).sum()), len(u)))
    assert (~same).sum() <= CAP * len(u), what
    # the pdf along the direction: the same table entry, but for directions on a texel border
    flip = same & (got[:, 7] != look[:, 3])
    assert flip.sum() <= CAP * len(u), (what, int(flip.sum()))
    bound = (2e-6 * w + 1e-6) * float(np.abs(rgba[..., :3]).max()) * 1.5
    m = same & ~flip
    assert (np.abs(got[m, 4:7] - look[m, 0:3]).max(axis=1) <= 2 * bound + TOL * np.abs(look[m, 0:3]).max(axis=1)).all(), what
    # against float64, Q2 included: the pdf read back is the half-turn texel's, not the sampled one's
    q2 = lh.check_env_sample(got[:, 0:4], got[:, 4:8], rgba, tables, u, rotation, 1.5, what, dir_tol=3.6e-6 + TOL, radiance_tol=bound + TOL * float(np.abs(rgba[..., :3]).max()) * 1.5)
    if w > 1 and kind in ("noise", "black_top"):
        assert q2 > 0
    if kind == "black_top":
        assert (got[:, 3] > 0).all() and (lr.env_select(tables, u)[0] != 0).all()


@pytest.mark.parametrize("size,kind,rotation", lh.ENV_CASES)
def test_env_lookups_match_oracle_and_float64(tmp_path, size, kind, rotation):
    w, h = ls.ENV_SIZES[size]
    host, rgba = ls.env_scene(tmp_path, ls.env_map(kind, w, h), "env")
    dev = pt.DeviceScene(host.desc, 0, keepalive=host)
    s = _with(host.settings_for(), environmentRotation=rotation, environmentIntensity=0.7)
    d = ls.env_directions(w, h, rotation, 20000, 5)
    got = dev.env_eval(s, d)
    rc, ref = ol.env_eval(rgba, rotation, 0.7, d)
    assert rc == 0
    what = "device %s %s %.2f" % (size, kind, rotation)
    flip = got[:, 3] != ref[:, 3]
    _, border = lr.env_pdf_candidates(lr.env_texel_pdf(rgba), d, rotation)
    print("%s: %d of %d directions read another texel's pdf than the oracle (%d of them within 1e-4 texels of a border)"
          % (what, int(flip.sum()), len(d), int((flip & (border <= 1e-4)).sum())))
    assert flip.sum() <= CAP * len(d) and not (flip & (border > 1e-3)).any(), what
    bound = (2e-6 * w + 1e-6) * float(np.abs(rgba[..., :3]).max()) * 0.7
    pole = (d[:, 0] == 0) & (d[:, 2] == 0)
    assert (np.abs(got[:, 0:3] - ref[:, 0:3]).max(axis=1) <= 2 * bound + TOL * np.abs(ref[:, 0:3]).max(axis=1))[~pole].all(), what
    # straight up and down: u hangs on the signs of the zeros, the row does not - the radiance is one of the pole row's, and the pdf too
    assert np.isfinite(got[pole]).all()
    lh.check_env_eval(got, rgba, d, rotation, 0.7, what, radiance_tol=bound + TOL * float(np.abs(rgba[..., :3]).max()) * 0.7)


def test_env_pdf_guard_and_missing_map(tmp_path):
    # a NaN, an infinite and a negative texel (test_lights_host.bad_env_map): no table pdf is a positive number, envPdfOf's guard returns 0
    # for every direction, as the oracle's does and float64's; the radiance is still looked up
    host, rgba = ls.env_scene(tmp_path, lh.bad_env_map("nan"), "bad")
    assert np.isnan(rgba[7, 3, 0]) and np.isinf(rgba[6, 1, 0]) and rgba[7, 9, 0] == -2.0 and not lr.env_texel_pdf(rgba).any()
    dev = pt.DeviceScene(host.desc, 0, keepalive=host)
    s = _with(host.settings_for(), environmentRotation=0.3, environmentIntensity=1.0)
    d = ls.env_directions(16, 8, 0.3, 2000, 2)
    got = dev.env_eval(s, d)
    rc, ref = ol.env_eval(rgba, 0.3, 1.0, d)
    assert (got[:, 3] == 0).all() and (ref[:, 3] == 0).all()
    # (a lookup that touches the NaN or the infinite texel is no number on either side; which lookups touch them hangs on a weight being
    # exactly 0, a last-ulp matter)
    dev_fin, ref_fin = np.isfinite(got[:, 0:3]).all(axis=1), np.isfinite(ref[:, 0:3]).all(axis=1)
    assert ref_fin.mean() > 0.8 and (dev_fin != ref_fin).sum() <= CAP * len(d)
    fin = dev_fin & ref_fin
    assert (_rel(got[fin, 0:3], ref[fin, 0:3], 1e-3) <= 10 * TOL).all()
    # the negative texel alone: its pdf is 0, it is never sampled, and the rest of the map behaves as any other
    host, rgba = ls.env_scene(tmp_path, lh.bad_env_map("negative"), "negative")
    assert rgba[7, 9, 0] == -2.0
    dev = pt.DeviceScene(host.desc, 0, keepalive=host)
    got = dev.env_eval(s, d)
    rc, ref = ol.env_eval(rgba, 0.3, 1.0, d)
    assert (got[:, 3] != ref[:, 3]).sum() <= CAP * len(d) and 0 < (got[:, 3] == 0).sum() < 0.05 * len(d)
    bound = (2e-6 * 16 + 1e-6) * float(np.abs(rgba[..., :3]).max())
    lh.check_env_eval(got, rgba, d, 0.3, 1.0, "device, negative texel", radiance_tol=bound + TOL * float(np.abs(rgba[..., :3]).max()))
    tables = pt.debug_env_distribution(rgba)
    u = ls.env_u(tables, 20000, 11)
    smp = dev.env_sample(s, u)
    assert (smp[:, 3] > 0).all()
    lh.check_env_sample(smp[:, 0:4], smp[:, 4:8], rgba, tables, u, 0.3, 1.0, "device, negative texel", dir_tol=3.6e-6 + TOL,
                        radiance_tol=bound + TOL * float(np.abs(rgba[..., :3]).max()))
    # no environment map: both probes say so
    lit = ls.light_scene(tmp_path, 1)
    plain = pt.DeviceScene(lit.desc, 0, keepalive=lit)
    for call in (lambda: plain.env_eval(s, d[:4]), lambda: plain.env_sample(s, np.zeros((4, 3), np.float32))):
        with pytest.raises(pt.PtrError, match="no environment map"):
            call()


# ---------------------------------------------------------------- rectangle-light NEE
def _queue_rays(out):
    """The shadow rays of the queued records, as ptr_debug_connect_rays takes them."""
    n = len(out)
    return np.concatenate([out[:, 2:5], np.full((n, 1), 1e-4, np.float32), out[:, 5:8], out[:, 8:9]], axis=1).astype(np.float32)


@pytest.mark.parametrize("semantics", [0, METAL], ids=["embree", "metal"])
@pytest.mark.parametrize("lights,scale", [(1, 1.0), (2, 1.0), (8, 1.0), (9, 1.0), (2, 137.5)])
def test_rect_light_nee_matches_oracle(tmp_path, lights, scale, semantics):
    """The hit's own material (every type of materials.scene), firefly clamp on, random throughputs: every output of rectLightNee against
    the oracle's NEE at the same vertex, the random state on every sample, and queued-and-unoccluded == the oracle's 'contributes'."""
    host = ls.light_scene(tmp_path, lights, scale)
    dev = pt.DeviceScene(host.desc, 0, keepalive=host)
    osc = ol.OracleScene(host)
    s = _with(host.settings_for(), metalSemantics=semantics)
    rays, cls, states, _ = lh.nee_inputs(lights, scale, n=6000)
    thr = np.random.default_rng(3).uniform(0.05, 1.0, (len(rays), 3)).astype(np.float32)
    out, after = dev.rect_light_nee(s, rays, thr, states)
    ref, ref_after = osc.rect_light_nee(s, rays, thr, states)
    what = "%d lights, scale %g, semantics %d" % (lights, scale, semantics)
    n = len(rays)
    assert np.array_equal(after, ref_after), (what, int((after != ref_after).sum()))
    assert (out[:, 12:] == 0).all()
    hit_flip = (out[:, 0] > 0) != (ref["hit"] > 0)
    queued, positive = out[:, 1] > 0, (ref["contribution"].max(axis=1) > 0)
    # queued = the sample has a positive contribution and the light's own rectangle does not end the shadow ray before it starts
    wrong = queued & ~positive
    dropped = positive & ~queued & ~(ref["occluded"] > 0)
    print("%s: %d rays, %d queued, %d hit flips, %d queued without an oracle contribution, %d contributions not queued though unoccluded"
          % (what, n, int(queued.sum()), int(hit_flip.sum()), int(wrong.sum()), int(dropped.sum())))
    assert hit_flip.sum() + wrong.sum() + dropped.sum() <= CAP * n, what
    assert queued.sum() > 0.05 * n and (positive & ~queued).sum() > 0   # (the pre-test of the light's own triangles does drop samples)
    m = queued & positive
    size = np.maximum(np.abs(out[m, 2:5]).max(axis=1), 1.0)
    assert (np.abs(out[m, 2:5] - ref["shadow_origin"][m]).max(axis=1) <= TOL * size).all(), what
    assert (np.abs(out[m, 5:8] - ref["direction"][m]).max(axis=1) <= TOL).all(), what
    assert (np.abs(out[m, 8] - ref["shadow_max"][m]) <= TOL * ref["shadow_max"][m]).all(), what
    cerr = _rel(out[m, 9:12], ref["contribution"][m])
    assert (cerr <= TOL).all(), (what, float(cerr.max()))
    # end to end: the queued record through the production k_connect, with its kind
    occ, _ = dev.connect_rays(_queue_rays(out[queued]))
    contributes = np.zeros(n, bool)
    contributes[np.flatnonzero(queued)] = ~occ
    flips = contributes != (ref["contributes"] > 0)
    print("%s: %d of %d visibility decisions differ (%s)" % (what, int(flips.sum()), n, dict(zip(*np.unique(cls[flips], return_counts=True)))))
    assert flips.sum() <= CAP * n, what
    assert contributes.sum() > 0.03 * n and (queued & ~contributes).sum() > 0
    # every class of receiver was there
    for c in ("near", "plane", "graze", "wall", "close", "far", "back"):
        assert (out[cls == c, 0] > 0).mean() > 0.5, c


@pytest.mark.parametrize("semantics", [0, METAL], ids=["embree", "metal"])
@pytest.mark.parametrize("lights,scale", [(1, 1.0), (2, 1.0), (8, 1.0), (9, 1.0), (2, 137.5)])
def test_rect_light_nee_matches_float64(tmp_path, lights, scale, semantics):
    """Lambert override, clamp off: contribution = E rho/pi cos / (pdf + cos/pi) in float64, and the pdf recovered from it equals
    rectLightPdfForHit at the sampled point (the area from two code paths, the 1/N pick from two more)."""
    host = ls.light_scene(tmp_path, lights, scale)
    dev = pt.DeviceScene(host.desc, 0, keepalive=host)
    osc = ol.OracleScene(host)
    s = _with(host.settings_for(), metalSemantics=semantics, fireflyClampEnabled=0)
    rays, cls, states, thr = lh.nee_inputs(lights, scale)
    out, after = dev.rect_light_nee(s, rays, thr, states, ls.lambert())
    sh = osc.surface_hits(np.concatenate([rays, rays[:, 3:]], axis=1))
    lit = lr.Lights(host.desc)
    u, _ = lr.rng_draw(states, 3)
    smp = lit.sample(sh[:, 2:5], u)
    # the override is a Lambert surface: the sampling runs at every hit, emitters included (their own material is not looked at)
    ran = out[:, 0] > 0
    assert (ran != (sh[:, 0] > 0)).sum() <= CAP * len(rays)
    queued = out[:, 1] > 0
    # recover the pdf: c = E rho/pi cos / (pdf + cos/pi), channel by channel the same number
    cos = np.einsum("ij,ij->i", sh[:, 8:11].astype(np.float64), out[:, 5:8].astype(np.float64))
    e = lit.emission[smp["light"]] * np.array(ls.LAMBERT_ALBEDO)
    with np.errstate(divide="ignore", invalid="ignore"):
        pdf = (e / np.pi * cos[:, None] / out[:, 9:12].astype(np.float64) - cos[:, None] / np.pi).mean(axis=1)
    # the pre-test drops the samples whose shadow ray the light's own rectangle ends (the oracle counts them as occluded): the device
    # reports no value for those, and they are left out here - the visibility check of test_rect_light_nee_matches_oracle holds them
    got = {"ran": ran, "sampled": queued, "direction": out[:, 5:8], "pdf": np.where(queued, pdf, 0.0), "contribution": out[:, 9:12]}
    ref, _ = osc.rect_light_nee(s, rays, thr, states, ls.lambert())
    pretested = ~queued & (ref["occluded"] > 0) & (ref["contribution"].max(axis=1) > 0)
    what = "device, %d lights, scale %g, semantics %d" % (lights, scale, semantics)
    # (recovering the pdf from the contribution divides by it: an error of the contribution grows by (pdf + 2 cos/pi) / pdf)
    errs = lh.check_nee_against_float64(host, osc, s, rays, cls, states, got, after, what, extra=TOL, pdf_gain=True, leave_out=pretested)
    # what was compared is the device's own: every class has its queued samples - at least those the oracle finds unoccluded, which the
    # pre-test cannot drop - except 'close', the plate 1e-3 under the first light and facing it, which the device can never queue a sample
    # of that light from (quirk Q9: the offset origin lies nearer the light than the shortened ray is long, so the light ends its own ray)
    rcos = np.abs(np.einsum("ij,ij->i", sh[:, 8:11].astype(np.float64), np.nan_to_num(smp["direction"])))
    klass = lh.nee_class(cls, smp, rcos, lit)
    free = (ref["occluded"] == 0) & (ref["contribution"].max(axis=1) > 0) & (np.abs(smp["cos"]) > 1e-5) & (rcos > 1e-5) & (cls != "plane")
    for k in ["near", "grazing"] + (["far"] if lights > 1 else []) + (["sliver"] if lights >= 8 else []):
        need = max(20 if k != "far" else 3, int(0.9 * (free & (klass == k)).sum()))
        assert k in errs and errs[k][2] >= need, (what, k, errs.get(k), need)
    # ... and that pdf is rectLightPdfForHit at position + direction x distance, from the same origin
    q = np.flatnonzero(queued)
    inp = np.zeros((len(q), 14), np.float32)
    inp[:, 0:3], inp[:, 3:6] = sh[q, 2:5], out[q, 5:8]
    inp[:, 6:9], inp[:, 9], inp[:, 10:13] = 1.0, 1.0, 1.0
    con, info = dev.light_connection(s, inp)
    assert info["lights"] == lit.count
    same = (con[:, 0] > 0) & (con[:, 2] == smp["light"][q])
    assert same.mean() > 0.9, (what, same.mean())
    gain = (pdf[q] + 2 * cos[q] / np.pi) / pdf[q]
    err = np.abs(con[:, 8] - pdf[q]) / pdf[q]
    print("%s: %d queued samples, the pdf in the contribution against rectLightPdfForHit: %.2e at most (relative)" % (what, int(same.sum()), err[same].max()))
    assert (err[same] <= 2 * TOL * gain[same]).all(), (what, float((err[same] / gain[same]).max()))


@pytest.mark.parametrize("lights", [1, 8])
def test_solid_angle_quadrature(tmp_path, lights):
    """The mean of 1 / (pdf N) over a 256 x 256 midpoint grid of (lu, lv), with the device's rectLightPdfForHit along rays to the grid
    points, is the closed-form solid angle of the light (2.1e-5: four times the quadrature's own error, plus the device tolerance)."""
    host = ls.light_scene(tmp_path, lights, plate=False)
    dev = pt.DeviceScene(host.desc, 0, keepalive=host)
    s = host.settings_for()
    lit = lr.Lights(host.desc)
    g = (np.arange(256) + 0.5) / 256
    lu, lv = (a.ravel() for a in np.meshgrid(g, g, indexing="ij"))
    for light, p in ((0, (0.3, 2.0, 0.2)), (0, (-2.0, 1.0, 0.5)), (0, (0.1, 3.75, -0.2)), (0, (-4.0, 3.5, 3.0))) + (((6, (-4.4, 1.0, 3.3)), (6, (-4.6, 5.5, 3.6))) if lights == 8 else ()):
        pos = np.tile(np.array(p, np.float32), (len(lu), 1))
        pts = lit.corner[light] + lu[:, None] * lit.eu[light] + lv[:, None] * lit.ev[light]
        omega = lit.solid_angle(light, pos[:1].astype(np.float64))[0]
        p64 = lit.pdf_for_point(np.full(len(lu), light), pts, pos)
        inp = np.zeros((len(lu), 14), np.float32)
        inp[:, 0:3], inp[:, 3:6] = pos, pts - pos
        inp[:, 6:9], inp[:, 9], inp[:, 10:13] = 1.0, 1.0, 1.0
        con, _ = dev.light_connection(s, inp)
        seen = (con[:, 0] > 0) & (con[:, 2] == light) & (con[:, 8] > 0)
        assert seen.mean() >= 1.0 - CAP, (light, p, seen.mean())   # (a grid point on the diagonal the two triangles share may be missed)
        q = np.mean(np.where(seen, 1.0 / np.maximum(con[:, 8].astype(np.float64) * lit.count, 1e-300), 1.0 / (p64 * lit.count)))
        print("light %d from %s: solid angle %.6f, device quadrature off by %.2e (relative), %d grid points not found" % (light, p, omega, abs(q / omega - 1), int((~seen).sum())))
        assert abs(q / omega - 1) <= 2.1e-5 + TOL


# ---------------------------------------------------------------- settled specular connections
@pytest.mark.parametrize("semantics", [0, METAL], ids=["embree", "metal"])
@pytest.mark.parametrize("lights,scale", [(1, 1.0), (2, 1.0), (8, 1.0), (2, 137.5)])
def test_settled_connections_match_oracle(tmp_path, lights, scale, semantics):
    host = ls.light_scene(tmp_path, lights, scale)
    dev = pt.DeviceScene(host.desc, 0, keepalive=host)
    osc = ol.OracleScene(host)
    s = _with(host.settings_for(), metalSemantics=semantics)
    inp = lh.connection_inputs(host, 8000, 9, scale)
    out, info = dev.light_connection(s, inp)
    assert info == {"settles": True, "lights": lights}
    ref = osc.light_connection(s, inp)
    lit = lr.Lights(host.desc)
    n = len(inp)
    what = "%d lights, scale %g, semantics %d" % (lights, scale, semantics)
    found, light, half = out[:, 0] > 0, out[:, 2].astype(np.int64), out[:, 3].astype(np.int64)
    assert ((half == 0) | (half == 1)).all() and (light[found] < lights).all() and (out[~found] == 0).all()
    rays = np.concatenate([inp[:, 0:3], np.full((n, 1), 1e-4, np.float32), inp[:, 3:6], np.full((n, 1), np.inf, np.float32)], axis=1)
    # found: the float64 ray / rectangle test over the lights alone, outside its edge margin (counted in altitudes of the triangle, so that
    # the light 1e-3 wide, whose width is 2000 ulps of the float32 origins, keeps a margin float32 can resolve: light_ref.Reference)
    only = lr.light_reference(host.desc, lit)
    r64 = only.trace(rays)
    clear = (r64["margin"] > 1e-6) & ~r64["near_ends"]
    assert clear.mean() > 0.95, (what, clear.mean())   # (the rays left out are those aimed at a rim; 2 % with the sliver)
    light64 = np.where(r64["index"] >= 0, only.light[np.maximum(r64["index"], 0)], -1)
    tie = np.zeros(n, bool)
    if lights >= 8:   # the two coplanar overlapping lights: either may be found where float64 has both at the same distance to 1e-6
        for a, b in ((4, 5), (5, 4)):
            sub = tr.Reference.__new__(tr.Reference)
            keep = only.light == b
            sub.tri, sub.sph = only.tri[keep], only.sph
            sub.v0, sub.e1, sub.e2, sub.n = only.v0[keep], only.e1[keep], only.e2[keep], only.n[keep]
            tb = sub.trace(rays)["t"]
            with np.errstate(invalid="ignore"):   # (inf - inf where neither is hit)
                tie |= (light64 == a) & (np.abs(tb - r64["t"]) <= 1e-6 * r64["t"])
        assert tie.sum() > 10
    bad = clear & ~tie & (np.where(found, light, -1) != light64)
    assert not bad.any(), (what, int(bad.sum()), inp[bad][:3], out[bad][:3], light64[bad][:3])
    # half: the triangle of the rectangle float64 finds (the pairs of traversal_ref: the half of the corner, then the half opposite; the
    # margin covers the diagonal they share)
    decided = clear & ~tie & found & (light == light64)
    assert decided.sum() > 0.25 * n and np.array_equal(half[decided], r64["index"][decided] % 2), (what, int((half[decided] != r64["index"][decided] % 2).sum()))
    assert (half[decided] == 0).sum() > 0.05 * n and (half[decided] == 1).sum() > 0.05 * n
    # light: the oracle's, wherever its closest hit over the whole scene is a light (nothing stands before the nearest light)
    lit_ref = found & (ref["hit"] > 0) & (ref["light"] >= 0)
    differ = lit_ref & ~tie & (light != ref["light"].astype(np.int64))
    print("%s: %d rays where the oracle's closest hit is a light, %d name another light" % (what, int(lit_ref.sum()), int(differ.sum())))
    assert lit_ref.sum() > 0.1 * n and not (differ & clear).any() and differ.sum() <= CAP * n, what
    assert found.mean() > 0.3 and (~found).mean() > 0.1
    if lights >= 8:
        assert (light[found] == 2).sum() > 10   # the light behind the first one
    # t: the traversal's, bit for bit, wherever the closest hit over the whole scene is that light
    hits, _ = dev.trace_rays(rays)
    closest = found & (hits["t"] >= 0) & (hits["primType"] == 2) & (hits["primIndex"] == lit.rect[np.minimum(light, lights - 1)])
    assert closest.sum() > 0.1 * n
    assert np.array_equal(out[closest, 1].view(np.uint32), hits["t"][closest].view(np.uint32)), (what, int((out[closest, 1] != hits["t"][closest]).sum()))
    # the ignore word names the light's rectangle (kind 2 in bits 31:30, the rectangle index in the low 26)
    word = out[found, 4].view(np.uint32)
    assert ((word >> 30) == 2).all() and np.array_equal((word & ((1 << 26) - 1)).astype(np.int64), lit.rect[light[found]])
    # the kind-3 record: the contribution worked out up front, zeroed when anything but the light's own triangles lies before it -
    # that is the reference's closest hit, then is-it-a-light
    f = np.flatnonzero(found)
    any_hit = rays[f].copy()
    any_hit[:, 7] = out[f, 1]
    occ, _ = dev.connect_rays(any_hit, ignore_light=light[f].astype(np.uint32))
    value = np.zeros((n, 3))
    value[f] = np.where(occ[:, None], 0.0, out[f, 5:8])
    pos_dev, pos_ref = value.max(axis=1) > 0, ref["contribution"].max(axis=1) > 0
    # (a tie between the coplanar lights is left out: the light found and the light the reference's closest hit names may differ, and the
    # other light's triangles, an ulp nearer or farther, may or may not end the any-hit query)
    if tie.any():
        print("%s: %d ties between coplanar lights, %d of them with a contribution on one side only" % (what, int(tie.sum()), int((tie & (pos_dev != pos_ref)).sum())))
    flips = (pos_dev != pos_ref) & ~tie
    print("%s: %d rays, %d find a light, %d of those occluded, %d oracle contributions, %d decisions differ"
          % (what, n, int(found.sum()), int(occ.sum()), int(pos_ref.sum()), int(flips.sum())))
    assert flips.sum() <= CAP * n, what
    assert occ.sum() > 20 and pos_ref.sum() > 0.05 * n   # (rays with a sphere, the wall or the plate before the light are there)
    m = pos_dev & pos_ref & ~tie
    cerr = _rel(value[m], ref["contribution"][m])
    assert (cerr <= TOL).all(), (what, float(cerr.max()))
    # emitter-branch MIS, computed here from either pdf: clamp(lastPdf / (lastPdf + pdf), 1e-4, 0.9999); lastPdf = 0 and pdf = 0 included
    hit_same = closest & (ref["hit"] > 0) & (ref["prim_type"] == 2) & (ref["prim_index"] == lit.rect[np.minimum(light, lights - 1)])
    assert hit_same.sum() > 0.1 * n and (out[hit_same, 8] == 0).sum() > 5 and ((out[hit_same, 8] == 0) == (ref["pdf"][hit_same] == 0)).all()
    for last in (0.0, 1e-3, 1.0, 50.0):
        def mis(pdf):
            denom = last + pdf.astype(np.float64)
            with np.errstate(divide="ignore", invalid="ignore"):
                return np.clip(np.where(denom > 0, last / denom, 1.0), 1e-4, 0.9999)
        a, b = mis(out[hit_same, 8]), mis(ref["pdf"][hit_same])
        assert (np.abs(a - b) <= TOL * b).all(), (what, last, float((np.abs(a - b) / b).max()))
    assert (_rel(out[hit_same, 8:9], ref["pdf"][hit_same][:, None], 1e-30)[ref["pdf"][hit_same] > 0] <= TOL).all()
    assert np.array_equal(out[hit_same, 9] > 0, ref["front_face"][hit_same] > 0)


def test_nine_lights_are_not_settled(tmp_path):
    """kSettleLightsMax = 8: the ninth light switches the settled connections off, and k_shade queues the closest-hit record instead; the
    equivalence above is therefore not asked of nine lights - only that the scene says so.  Eight lights still settle."""
    s9 = ls.light_scene(tmp_path, 9)
    dev = pt.DeviceScene(s9.desc, 0, keepalive=s9)
    _, info = dev.light_connection(s9.settings_for(), np.zeros((0, 14), np.float32))
    assert info == {"settles": False, "lights": 9}
    s8 = ls.light_scene(tmp_path, 8)
    _, info = pt.DeviceScene(s8.desc, 0, keepalive=s8).light_connection(s8.settings_for(), np.zeros((0, 14), np.float32))
    assert info == {"settles": True, "lights": 8}
