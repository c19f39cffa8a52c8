"""Host-side (no GPU) checks of the light side of a path vertex: the oracle's environment sampling, light pdfs, rectangle-light NEE and
specular connections against the float64 restatement of light_ref.py, on the scenes, maps and edge inputs of light_scenes.py.

With test_gpu_lights.py (device == oracle sample by sample) this makes device ~= float64.  Bounds: the oracle's error against float64
measured on these inputs (profiles/r5_light_reference.txt) times 4, the margin for other seeds and for the float32 conditioning of
d^2 / cos they will meet:
  sampled direction 3.6e-6 absolute, table pdf 6.8e-6 relative (measured 9e-7 and 1.7e-6);
  level-0 radiance (2e-6 W + 1e-6) max|rgb|: u carries about 5e-7 of float32 atan2 / asin error and the product u W another 2^-24 W, a
  bilinear weight is off by that many texels and the result by that times the largest difference between neighbours (<= 2 max|rgb|);
  256 x 256 midpoint quadrature of 1 / (pdf N) against the closed-form solid angle 2.1e-5 relative, receivers >= 0.25 off the plane;
  rectangle NEE pdf and Lambert contribution per class: NEE_BOUNDS below.
A texel choice float32 cannot make (a direction within 1e-4 texels of a border) is held to the texels on either side of the border.
What float64 cannot decide is held to the oracle only (test_gpu_lights.py): receivers exactly in a light's plane (the cosine is an exact
0 or rounding noise: 312 of the 'plane' samples per scene here) and exact ties between coplanar lights.
"""
import ctypes as C
import os

import numpy as np
import pytest

import light_ref as lr
import light_scenes as ls
import oracle_lib as ol
import traversal_ref as tr

pt = ls.pt

# relative bounds (pdf, contribution) of the oracle's rectangle NEE against float64: 4 x the largest error measured per class of sample
# over the five scenes (profiles/r5_light_reference.txt: near 3.5e-7 / 6.6e-6, far 2.2e-7 / 4.0e-7, grazing 8.1e-7 / 1.05e-6, sliver
# 3.3e-7 / 1.2e-5, close 6.9e-6 / 2.0e-6).  The contribution carries the receiver's cosine, known to 2^-24 / cos: 6e-6 at the 1e-2
# where 'grazing' begins; the plate 1e-3 under the light at Cornell scale knows its distance to 2^-24 x 550 / 0.14.
NEE_BOUNDS = {"near": (1.4e-6, 2.7e-5), "far": (8.8e-7, 1.6e-6), "grazing": (3.3e-6, 4.2e-6), "sliver": (1.3e-6, 4.9e-5), "close": (2.8e-5, 8.2e-6)}
# relative bounds (pdf, contribution) of the oracle's specular connection against float64, on top of each sample's own conditioning: 4 x
# the largest errors measured over the four scenes (profiles/r5_light_reference.txt: 1.85e-6 and 5.55e-7)
CONNECTION_BOUNDS = (7.4e-6, 2.2e-6)
SLIVER = 3   # index of the sliver among the lights of the 8- and 9-light scenes
ZERO = 7     # index of the zero-area light


def nee_class(cls, sample, receiver_cos, lights):
    """The tolerance class of every sample: 'sliver' by the light picked, 'grazing' where the cosine at the light or at the receiver is
    below 1e-2 or the receiver lies in or just under the first light's plane, 'far' for the receivers 1e4 away, 'close' for the plate 1e-3
    under the first light (its distance to the light is known to 2^-24 |P| / 1e-3 only), else 'near'."""
    out = np.where(cls == "far", "far", np.where(cls == "close", "close", "near")).astype(object)
    out[(np.abs(sample["cos"]) < 1e-2) | (receiver_cos < 1e-2) | (cls == "plane") | (cls == "graze")] = "grazing"
    if lights.count >= 8:
        out[sample["light"] == SLIVER] = "sliver"
    return out.astype(str)


def test_light_probes_check_their_arguments():
    """A null scene is refused before anything touches a device: with a GPU or without one."""
    lib = pt.load_library()
    err = C.create_string_buffer(256)
    f = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    u32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    s = pt.HostScene.load(os.path.join(ls.GOLDEN, "smoke.scene")).settings_for(8, 8)
    a, out, st = np.zeros((1, 14), np.float32), np.zeros((1, 16), np.float32), np.zeros(1, np.uint32)
    info = (C.c_uint32 * 2)()
    for name, call in (("ptr_debug_env_sample", lambda: lib.ptr_debug_env_sample(None, C.byref(s), f(a), 1, f(out), err, 256)),
                       ("ptr_debug_env_eval", lambda: lib.ptr_debug_env_eval(None, C.byref(s), f(a), 1, f(out), err, 256)),
                       ("ptr_debug_rect_light_nee", lambda: lib.ptr_debug_rect_light_nee(None, C.byref(s), None, f(a), f(a), u32(st), 1, f(out), u32(st), err, 256)),
                       ("ptr_debug_light_connection", lambda: lib.ptr_debug_light_connection(None, C.byref(s), f(a), 1, f(out), info, err, 256))):
        err.value = b""
        assert call() != 0 and name.encode() in err.value and b"null argument" in err.value, name
        assert not out.any()


# ---------------------------------------------------------------- environment
ENV_CASES = [("64x32", "noise", 0.0), ("64x32", "spot", 0.3), ("33x17", "noise", np.pi), ("33x17", "black_top", -7.0), ("33x17", "flat", 0.3),
             ("7x5", "spot", -7.0), ("7x5", "black_top", 0.0), ("16x3", "noise", np.pi), ("16x3", "flat", 0.0), ("1x1", "noise", 0.3)]


def _rgba(rgb):
    return np.concatenate([rgb, np.ones(rgb.shape[:2] + (1,), np.float32)], axis=2)


def check_env_sample(out, look, rgba, tables, u, rotation, intensity, what, dir_tol=3.6e-6, pdf_tol=6.8e-6, radiance_tol=None):
    """out [n, 4] {direction, pdf}, look [n, 4] {rgb, pdf along the direction} of the sampler under test against float64."""
    h, w = rgba.shape[:2]
    pdf64 = lr.env_texel_pdf(rgba)
    row, col, jx, jy = lr.env_select(tables, u)
    d64 = lr.env_direction(row, col, jx, jy, w, h, rotation)
    err = np.abs(out[:, :3] - d64).max()
    p64 = pdf64[row, col]
    assert (p64 > 0).all(), "%s: a texel of pdf 0 was sampled" % what
    perr = (np.abs(out[:, 3] - p64) / p64).max()
    print("%s: %d samples, direction error %.2e, sampled-texel pdf error %.2e" % (what, len(u), err, perr))
    assert err <= dir_tol and perr <= pdf_tol, (what, err, perr)
    # the pdf read back along the direction is that of the texel half a turn away (quirk Q2), not of the texel sampled
    hrow, hcol, border = lr.env_half_turn_texel(row, col, jx, w)
    cand, _ = lr.env_pdf_candidates(pdf64, out[:, :3], rotation)
    rel = np.abs(look[:, 3:4] - cand) / np.maximum(cand, 1e-30)
    ok = (rel <= pdf_tol).any(axis=1) | ((look[:, 3] == 0) & (cand == 0).any(axis=1))
    assert ok.all(), (what, int((~ok).sum()), u[~ok][:3], look[~ok][:3], cand[~ok][:3])
    clear = (border > 1e-3) & (np.abs(jy * 1.0 + row - np.round(jy + row)) > 1e-3)
    q2 = clear & (np.abs(pdf64[hrow, hcol] - p64) > 1e-3 * p64)
    if w > 1 and len(np.unique(pdf64)) > 8:   # (a map of many values: most samples tell the two texels apart)
        assert q2.sum() > 0.2 * len(u), (what, int(q2.sum()))
    hp = pdf64[hrow, hcol][q2]
    got = look[q2, 3]
    assert (np.abs(got - hp) <= pdf_tol * np.maximum(hp, 1e-30)).all(), what
    assert (np.abs(got - p64[q2]) > 1e-4 * p64[q2]).all(), what
    # level-0 radiance: bilinear, wrap in x, clamp in y
    c64 = lr.env_bilinear(rgba, out[:, :3], rotation, intensity)
    tol = radiance_tol if radiance_tol is not None else (2e-6 * w + 1e-6) * float(np.abs(rgba[..., :3]).max()) * max(intensity, 0.0)
    cerr = np.abs(look[:, :3] - c64).max()
    assert cerr <= tol, (what, cerr, tol)
    return int(q2.sum())


@pytest.mark.parametrize("size,kind,rotation", ENV_CASES)
def test_oracle_env_sampling_matches_float64(size, kind, rotation):
    w, h = ls.ENV_SIZES[size]
    rgba = _rgba(ls.env_map(kind, w, h))
    rc, tables = ol.env_build(rgba)
    assert rc == 0
    if kind == "flat" and w > 1:   # the map whose alias thresholds include exact 0 and exact 1
        assert (tables["cond_threshold"] == 0).any() and (tables["cond_threshold"] == 1).any()
    u = ls.env_u(tables, 20000, 11)
    rc, out, look = ol.env_sample(rgba, rotation, 1.5, u)
    assert rc == 0
    check_env_sample(out[:, [0, 1, 2, 6]], look, rgba, tables, u, rotation, 1.5, "oracle %s %s %.2f" % (size, kind, rotation))
    row, _, _, _ = lr.env_select(tables, u)
    if kind == "black_top":
        assert (row != 0).all()


def check_env_eval(got, rgba, directions, rotation, intensity, what, pdf_tol=6.8e-6, radiance_tol=None):
    h, w = rgba.shape[:2]
    pdf64 = lr.env_texel_pdf(rgba)
    cand, border = lr.env_pdf_candidates(pdf64, directions, rotation)
    rel = np.abs(got[:, 3:4] - cand) / np.maximum(cand, 1e-30)
    ok = (rel <= pdf_tol).any(axis=1) | ((got[:, 3] == 0) & (cand == 0).any(axis=1))
    ok &= (rel[:, 0] <= pdf_tol) | (border <= 1e-4) | ((got[:, 3] == 0) & (cand[:, 0] == 0))   # away from the borders: the float64 texel itself
    assert ok.all(), (what, int((~ok).sum()), directions[~ok][:3], got[~ok][:3], cand[~ok][:3])
    c64 = lr.env_bilinear(rgba, directions, rotation, intensity)
    tol = radiance_tol if radiance_tol is not None else (2e-6 * w + 1e-6) * float(np.abs(rgba[..., :3]).max()) * max(intensity, 0.0)
    pole = (directions[:, 0] == 0) & (directions[:, 2] == 0)   # u of a direction straight up or down hangs on the signs of its zeros
    cerr = np.abs(got[:, :3] - c64)[~pole].max()
    print("%s: %d directions, %d within 1e-4 texels of a border, radiance error %.2e (bound %.2e)" % (what, len(directions), int((border <= 1e-4).sum()), cerr, tol))
    assert cerr <= tol, (what, cerr, tol)


@pytest.mark.parametrize("size,kind,rotation", ENV_CASES)
def test_oracle_env_lookups_match_float64(size, kind, rotation):
    w, h = ls.ENV_SIZES[size]
    rgba = _rgba(ls.env_map(kind, w, h))
    d = ls.env_directions(w, h, rotation, 20000, 5)
    rc, got = ol.env_eval(rgba, rotation, 0.7, d)
    assert rc == 0
    check_env_eval(got, rgba, d, rotation, 0.7, "oracle %s %s %.2f" % (size, kind, rotation))


def bad_env_map(kind):
    """'negative': a negative texel in the bottom row - it weighs nothing, its pdf is 0 and the map is sampled as ever.  'nan': a NaN, an
    infinite and a negative texel - the NaN makes the weights' sum no number and every table pdf with it, which the pdf guard reads as 0.
    (A table pdf is infinite only if a weight is while their sum is not, which no map does: the guard's test for a finite value cannot be
    told from its test for a positive one.)"""
    rgb = ls.env_map("noise", 16, 8)
    rgb[7, 9] = -2.0
    if kind == "nan":
        rgb[7, 3], rgb[6, 1] = np.nan, np.inf
    return rgb


def test_oracle_env_pdf_guard_on_bad_texels():
    d = ls.env_directions(16, 8, 0.3, 2000, 2)
    rc, got = ol.env_eval(_rgba(bad_env_map("nan")), 0.3, 1.0, d)
    assert np.isfinite(got[:, 3]).all() and (got[:, 3] == 0).all() and not lr.env_texel_pdf(_rgba(bad_env_map("nan"))).any()
    # the negative texel alone: pdf 0 in its texel, the distribution alive everywhere else and never sampling it
    rgba = _rgba(bad_env_map("negative"))
    pdf64 = lr.env_texel_pdf(rgba)
    assert pdf64[7, 9] == 0 and (np.delete(pdf64.ravel(), 7 * 16 + 9) > 0).all()
    rc, got = ol.env_eval(rgba, 0.3, 1.0, d)
    assert rc == 0 and 0 < (got[:, 3] == 0).sum() < 0.05 * len(d)
    check_env_eval(got, rgba, d, 0.3, 1.0, "oracle, negative texel")
    rc, tables = ol.env_build(rgba)
    u = ls.env_u(tables, 20000, 11)
    rc, out, look = ol.env_sample(rgba, 0.3, 1.0, u)
    assert rc == 0
    check_env_sample(out[:, [0, 1, 2, 6]], look, rgba, tables, u, 0.3, 1.0, "oracle, negative texel")


def test_oracle_env_texel_frequencies():
    # 2 M samples, fixed seed: every texel is drawn within 5 sigma of its binomial expectation p = pdf x solid angle
    for size, kind in (("33x17", "noise"), ("7x5", "spot")):
        w, h = ls.ENV_SIZES[size]
        rgba = _rgba(ls.env_map(kind, w, h))
        n = 2_000_000
        u = np.random.default_rng(2024).random((n, 3), dtype=np.float32)
        rc, out, _ = ol.env_sample(rgba, 0.0, 1.0, u)
        d = out[:, :3].astype(np.float64)
        col = np.minimum(((np.arctan2(d[:, 2], d[:, 0]) / (2 * np.pi)) % 1.0 * w).astype(np.int64), w - 1)
        row = np.minimum((np.arccos(np.clip(d[:, 1], -1, 1)) / np.pi * h).astype(np.int64), h - 1)
        count = np.bincount(row * w + col, minlength=w * h).reshape(h, w)
        cell = np.sin((np.arange(h) + 0.5) * np.pi / h) * (np.pi / h) * (2 * np.pi / w)
        p = lr.env_texel_pdf(rgba) * cell[:, None]
        assert abs(p.sum() - 1.0) < 1e-12
        sigma = np.sqrt(n * p * (1 - p))
        z = np.abs(count - n * p) / np.maximum(sigma, 1.0)
        print("%s %s: largest deviation %.2f sigma" % (size, kind, z.max()))
        assert z.max() <= 5.0, (size, kind, z.max())


# ---------------------------------------------------------------- rectangle lights
def nee_inputs(lights_count, scale, n=4000, seed=5):
    rays, cls = ls.receiver_rays(n, seed + lights_count, scale)
    states = np.random.default_rng(seed).integers(1, 2 ** 32, len(rays), dtype=np.uint32)
    return rays, cls, states, np.ones((len(rays), 3), np.float32)


def check_nee_against_float64(host, osc, settings, rays, cls, states, got, got_states, what, extra=0.0, pdf_gain=False, leave_out=None):
    """got: {sampled-or-queued mask 'sampled', 'direction', 'pdf' (or None), 'contribution'} of the NEE under test at the hits the oracle
    reports, Lambert override, clamp off.  Returns the per-class largest relative errors and sample counts {class: (pdf, contribution,
    samples)}.  pdf_gain: the pdf was recovered from the contribution c = E rho/pi cos / (pdf + cos/pi), which multiplies c's error by
    (pdf + 2 cos/pi) / pdf.  leave_out: samples whose value the NEE under test does not report (the random stream is still compared)."""
    lights = lr.Lights(host.desc)
    sh = osc.surface_hits(np.concatenate([rays, rays[:, 3:]], axis=1))
    hit = sh[:, 0] > 0
    u, after = lr.rng_draw(states, 3)
    # the random stream: three numbers at every hit that is no emitter (the override material is never a delta surface), none elsewhere
    ran = got["ran"]
    assert (got_states[ran] == after[ran]).all() and (got_states[~ran] == states[~ran]).all(), what
    s = lights.sample(sh[:, 2:5], u)
    wo = -rays[:, 3:] / np.linalg.norm(rays[:, 3:], axis=1, keepdims=True)
    c64, ok = lights.lambert_contribution(s, sh[:, 8:11], wo, ls.LAMBERT_ALBEDO)
    ok &= ran
    receiver_cos = np.abs(np.einsum("ij,ij->i", sh[:, 8:11].astype(np.float64), np.nan_to_num(s["direction"])))
    klass = nee_class(cls, s, receiver_cos, lights)
    # float64 decides the sample wherever its cosines are not rounding noise
    decided = ran & hit & (np.abs(s["cos"]) > 1e-5) & (receiver_cos > 1e-5) & (cls != "plane")
    if leave_out is not None:
        decided &= ~leave_out
    positive = got["contribution"].max(axis=1) > 0
    bad = decided & (positive != ok)
    assert bad.sum() <= 0.002 * len(rays), (what, int(bad.sum()))
    if lights.count >= 8:   # the zero-area light draws its three numbers and contributes nothing
        z = ran & (s["light"] == ZERO)
        assert z.sum() > 20 and not positive[z].any() and not got["sampled"][z].any(), what
    both = decided & positive & ok
    errs = {}
    for k in np.unique(klass[both]):
        m = both & (klass == k)
        ce = (np.abs(got["contribution"][m] - c64[m]).max(axis=1) / np.abs(c64[m]).max(axis=1)).max()
        de = np.abs(got["direction"][m] - s["direction"][m]).max()
        gain = (s["pdf"][m] + 2.0 * receiver_cos[m] / np.pi) / s["pdf"][m] if pdf_gain else 1.0
        pe = (np.abs(got["pdf"][m] - s["pdf"][m]) / s["pdf"][m] / gain).max()
        errs[k] = (float(pe), float(ce), int(m.sum()))
        print("%s: class %-8s %5d samples  pdf %.2e  contribution %.2e  direction %.2e" % (what, k, int(m.sum()), pe, ce, de))
        # (a recovered pdf carries the contribution's error, so it is held to the contribution's bound)
        assert pe <= NEE_BOUNDS[k][1 if pdf_gain else 0] + extra and ce <= NEE_BOUNDS[k][1] + extra, (what, k, pe, ce)
    return errs


@pytest.mark.parametrize("lights,scale", [(1, 1.0), (2, 1.0), (8, 1.0), (9, 1.0), (2, 137.5)])
def test_oracle_rect_light_nee_matches_float64(tmp_path, lights, scale):
    host = ls.light_scene(tmp_path, lights, scale)
    osc = ol.OracleScene(host)
    s = host.settings_for()
    s.fireflyClampEnabled = 0
    rays, cls, states, thr = nee_inputs(lights, scale)
    res, after = osc.rect_light_nee(s, rays, thr, states, ls.lambert())
    got = {"ran": res["ran"] > 0, "sampled": res["sampled"] > 0, "direction": res["direction"], "pdf": res["pdf"], "contribution": res["contribution"]}
    errs = check_nee_against_float64(host, osc, s, rays, cls, states, got, after, "oracle, %d lights, scale %g" % (lights, scale))
    assert set(errs) >= ({"near", "grazing", "close"} | ({"far"} if lights > 1 else set()) | ({"sliver"} if lights >= 8 else set())), errs
    # every class of receiver is there, and each decision is: behind the one-sided light nothing is sampled
    for c in ("near", "plane", "graze", "wall", "close", "far", "back"):
        assert (res["hit"][cls == c] > 0).mean() > 0.5, c
    lit = lr.Lights(host.desc)
    sh = osc.surface_hits(np.concatenate([rays, rays[:, 3:]], axis=1))
    picked = lit.sample(sh[:, 2:5], lr.rng_draw(states, 3)[0])
    behind = (res["ran"] > 0) & (picked["light"] == 0) & (sh[:, 3] > 4.5 * scale)   # the ceiling, over the light that faces down
    assert behind.sum() > 20 and not (res["sampled"][behind] > 0).any()
    # the shadow ray's length is measured from the hit, not from its offset origin (quirk Q9)
    m = res["sampled"] > 0
    assert np.allclose(res["shadow_max"][m], np.maximum(res["distance"][m] - np.float32(1e-4), 1e-4), rtol=1e-6)


@pytest.mark.parametrize("lights", [1, 8])
def test_solid_angle_quadrature(tmp_path, lights):
    """mean over a 256 x 256 midpoint grid of 1 / (pdf N) = the solid angle of the light, for the float64 pdf and for the oracle's
    rectLightPdfForHit along rays to the grid points."""
    host = ls.light_scene(tmp_path, lights, plate=False)
    osc = ol.OracleScene(host)
    s = host.settings_for()
    lit = lr.Lights(host.desc)
    g = (np.arange(256) + 0.5) / 256
    lu, lv = (a.ravel() for a in np.meshgrid(g, g, indexing="ij"))
    for light, p in ((0, (0.3, 2.0, 0.2)), (0, (-2.0, 1.0, 0.5)), (0, (0.1, 3.75, -0.2)), (0, (-4.0, 3.5, 3.0))) + (((6, (-4.4, 1.0, 3.3)), (6, (-4.6, 5.5, 3.6))) if lights == 8 else ()):
        pos = np.tile(np.array(p, np.float32), (len(lu), 1))
        pts = lit.corner[light] + lu[:, None] * lit.eu[light] + lv[:, None] * lit.ev[light]
        omega = lit.solid_angle(light, pos[:1].astype(np.float64))[0]
        p64 = lit.pdf_for_point(np.full(len(lu), light), pts, pos)
        q64 = np.mean(1.0 / (p64 * lit.count))
        inp = np.zeros((len(lu), 14), np.float32)
        inp[:, 0:3], inp[:, 3:6] = pos, pts - pos
        inp[:, 6:9], inp[:, 9], inp[:, 10:13] = 1.0, 1.0, 1.0
        res = osc.light_connection(s, inp)
        seen = (res["light"] == light) & (res["pdf"] > 0)
        # a grid point on the diagonal the two triangles share, or on the rim, may be missed or hidden: at most 0.2 %, left to float64
        assert seen.mean() >= 0.998, (light, p, seen.mean())
        qo = np.mean(np.where(seen, 1.0 / np.maximum(res["pdf"].astype(np.float64) * lit.count, 1e-300), 1.0 / (p64 * lit.count)))
        print("light %d from %s: solid angle %.6f, quadrature float64 %.2e, oracle %.2e (relative)" % (light, p, omega, abs(q64 / omega - 1), abs(qo / omega - 1)))
        assert abs(q64 / omega - 1) <= 2.1e-5 and abs(qo / omega - 1) <= 2.1e-5


def connection_inputs(host, n, seed, scale=1.0):
    """Specular-connection rays [m, 14]: random ones, rays aimed at points of the lights (past the spheres and the wall, through the first
    light to the one behind it, at the lights' backs), weights, bsdf pdfs (0 included) and throughputs."""
    rng = np.random.default_rng(seed)
    lit = lr.Lights(host.desc)
    o = rng.uniform((-7, 0.2, -7), (7, 5.8, 7), (n, 3)) * scale
    d = rng.normal(size=(n, 3))
    aimed = rng.random(n) < 0.75
    k = rng.integers(0, lit.count, n)
    target = lit.corner[k] + rng.uniform(-0.05, 1.05, (n, 1)) * lit.eu[k] + rng.uniform(-0.05, 1.05, (n, 1)) * lit.ev[k]
    d = np.where(aimed[:, None], target - o, d)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    inp = np.zeros((n, 14), np.float32)
    inp[:, 0:3], inp[:, 3:6] = o, d
    inp[:, 6:9] = rng.uniform(0.1, 2.0, (n, 3))
    inp[:, 9] = rng.choice((0.0, 1e-5, 0.3, 4.0, 1e3), n)
    inp[:, 10:13] = rng.uniform(0.05, 1.0, (n, 3))
    return inp


@pytest.mark.parametrize("lights,scale", [(1, 1.0), (2, 1.0), (8, 1.0), (2, 137.5)])
def test_oracle_light_connection_matches_float64(tmp_path, lights, scale):
    host = ls.light_scene(tmp_path, lights, scale)
    osc = ol.OracleScene(host)
    s = host.settings_for()
    s.fireflyClampEnabled = 0
    inp = connection_inputs(host, 6000, 9, scale)
    res = osc.light_connection(s, inp)
    lit = lr.Lights(host.desc)
    rays = np.concatenate([inp[:, 0:3], np.full((len(inp), 1), 1e-4, np.float32), inp[:, 3:6], np.full((len(inp), 1), np.inf, np.float32)], axis=1)
    full = lr.Reference(host.desc)   # (the sliver: its edge margin counts in altitudes)
    r64 = full.trace(rays)
    clear = (r64["margin"] > 1e-6) & ~r64["near_ends"]
    src = full.src[np.maximum(r64["index"], 0)]
    rect64 = np.where((r64["kind"] == 0) & (src[:, 0] == 2), src[:, 2], -1)
    light64 = np.where(np.isin(rect64, lit.rect), np.searchsorted(lit.rect, np.maximum(rect64, 0)), -1)
    light64 = np.where(np.isin(rect64, lit.rect), light64, -1)
    got_light = np.where(res["hit"] > 0, res["light"], -1).astype(np.int64)
    # (coplanar overlapping lights: either may win where float64 sees both at the same distance to 1e-6)
    tie = np.zeros(len(inp), bool)
    if lights >= 8:
        only = lr.light_reference(host.desc, lit)
        for a, b in ((4, 5), (5, 4)):
            sub = tr.Reference.__new__(tr.Reference)
            keep = only.light == b
            sub.tri, sub.sph = only.tri[keep], only.sph
            sub.v0, sub.e1, sub.e2, sub.n = only.v0[keep], only.e1[keep], only.e2[keep], only.n[keep]
            tb = sub.trace(rays)["t"]
            with np.errstate(invalid="ignore"):   # (inf - inf where neither is hit)
                tie |= (light64 == a) & (np.abs(tb - r64["t"]) <= 1e-6 * r64["t"])
    bad = clear & ~tie & (got_light != light64)
    assert not bad.any(), (int(bad.sum()), inp[bad][:3], got_light[bad][:3], light64[bad][:3])
    assert (light64 >= 0).mean() > 0.2 and ((light64 < 0) & (r64["kind"] >= 0)).mean() > 0.1
    same = clear & (got_light == light64) & (light64 >= 0)
    point = inp[:, 0:3].astype(np.float64) + r64["t"][:, None] * inp[:, 3:6]
    p64 = lit.pdf_for_point(np.maximum(light64, 0), point, inp[:, 0:3])
    front = -np.einsum("ij,ij->i", inp[:, 3:6].astype(np.float64), lit.normal[np.maximum(light64, 0)])
    decided = same & (np.abs(front) > 1e-4)
    zero = decided & (p64 == 0)
    assert zero.sum() > 5 and (res["pdf"][zero] == 0).all() and (res["contribution"][zero] == 0).all()   # the back of a one-sided light
    m = decided & (p64 > 0)
    perr = np.abs(res["pdf"][m] - p64[m]) / p64[m]
    c64 = lr.connection_contribution(lit.emission[light64[m]], p64[m], inp[m, 6:9], inp[m, 9], inp[m, 10:13])
    cerr = np.abs(res["contribution"][m] - c64).max(axis=1) / c64.max(axis=1)
    # the hit point o + t d of a float32 ray is known to 2^-24 (|o| + t): d^2 / cos carries that over the distance and the cosine.  Every
    # sample is held to its own conditioning plus CONNECTION_BOUNDS, never to the batch's worst ray
    cond = 4.0 * 2.0 ** -24 * (np.abs(inp[m, 0:3]).max(axis=1) + r64["t"][m]) * (1.0 / r64["t"][m] + 1.0 / (r64["t"][m] * np.abs(front[m])))
    print("%d lights, scale %g: %d connections reach a light (%d from behind a one-sided one), pdf error %.2e, contribution error %.2e; "
          "over each sample's own conditioning (median %.1e): %.2f and %.2f at most"
          % (lights, scale, int(m.sum()), int(zero.sum()), perr.max(), cerr.max(), np.median(cond), (perr / cond).max(), (cerr / cond).max()))
    assert (perr <= CONNECTION_BOUNDS[0] + cond).all(), float((perr - cond).max())
    assert (cerr <= CONNECTION_BOUNDS[1] + cond).all(), float((cerr - cond).max())
