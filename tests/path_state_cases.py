"""The scenes, settings and pixel lists of test_path_state_host.py and test_gpu_path_state.py, and what both do with a side's recorded
vertices: lay them out as one table and hold each vertex to the float64 bookkeeping of tests/path_state_ref.py given that side's own
BSDF sample.  No GPU needed to make them; test_path_state_host.py shows them fair from the oracle's recorder and the reference alone.

Spheres, boxes and rectangles only.  Groups:
  nested   ten concentric non-thin dielectric spheres, each with its own ior and absorption, whose materials sit above index 255 at mixed
           parity in a table of 310 (the ids need their high byte and land in both halves of all four words of the packed stack); camera
           `through` looks through the common centre, camera `inside` starts inside sphere 3 with an empty stack (its pops find depth 0)
  mixed    an absorbing glass box, a thin pane, a rough and a smooth metal sphere in a Lambert room open to the top;
           roulette on
  lit      `mixed` under one rectangle light: rectangle NEE alone, with specular NEE, and with MNEE and its two-bounce chain (record slots
           0, 3 and 4); `traced`: under nine lights, past the eight up to which k_shade settles a specular connection itself, so that the
           connection is queued as a closest-hit record (kind 1) and k_connect works it out
  env      `mixed` under a 16 x 8 environment map with a sampling distribution (light_scenes.env_map), specular NEE on: environment NEE and
           the specular environment connection (record slots 1 and 2), and the escaped ray's MIS weight
  deep     two facing mirrors, the camera between them: depth 511
"""
import importlib
import os

import numpy as np

import light_scenes as ls
import path_state_ref as R

pt = importlib.import_module("metal-pathtracer-arm64_amd")

WIDTH, HEIGHT = 32, 24
BACKGROUND = (0.5, 0.6, 0.8)
NESTED_MATERIALS = (257, 258, 261, 264, 267, 270, 275, 282, 299, 304)   # sphere 0 (outermost) .. 9: above 255, odd and even
NESTED_TABLE = 310
NESTED_RADII = tuple(1.0 - 0.08 * i for i in range(10))

# ---------------------------------------------------------------- bounds
# Against the oracle (test_gpu_parity.test_sample_bsdf_matches_oracle): direction 2e-4 absolute; weight, pdf, throughput rtol 3e-3, atol 1e-5
DIR_ATOL, RTOL, ATOL = 2e-4, 3e-3, 1e-5
NEAR_TIE_CAP = 0.02
# Against float64, given the side's own float32 inputs (throughput before, t, sample weight), the next throughput is
#   ((thr x expf(-(sigma x t))) x weight) / p            [the last only when roulette spares the path]
# which is four float32 roundings (sigma x t, the two products, the division: 2^-24 relative each), the rounding of expf's argument seen
# through expf (|sigma t| x 2^-24 relative) and expf's own error.  No document of the device library's expf error is at hand, so it was
# measured: the largest error of the device's expf over the recorded arguments of the groups below, from the recorded throughputs
# (test_gpu_path_state prints it), is EXPF_MEASURED_ULP; the bound takes twice that.  1 ulp = 2^-23 relative.
EXPF_MEASURED_ULP = 0.2   # (0.19 on an MI355X, in `nested/through`: what its largest deviation leaves once the roundings have had their full share)
EXPF_ULP = 2.0 * EXPF_MEASURED_ULP
ROUNDINGS = 4.0
# Where clampThroughput engages the throughput is also multiplied by limit / max(luminance, 1e-6): the luminance is three products and two
# sums of positive terms (three roundings at most, relative to the sum), then the division and the product: five more.
CLAMP_ROUNDINGS = 5.0
# Radiance added at once - an escaped ray's background, an emitter's emission - is throughput x (radiance x mis), mis = lastPdf / (lastPdf +
# lightPdf) clamped: the sum, the division, the two products; where the firefly clamp engages, its luminance and scale as above, twice
# (the contribution's and the throughput's).  The published item adds it to the sum so far: one more, relative to the item.
IMMEDIATE_ROUNDINGS = 4.0 + 2.0 * CLAMP_ROUNDINGS


def throughput_bound(sigma_t, clamped=False):
    """relative bound [n] on a throughput component after one vertex; sigma_t [n]: the largest |sigma x t| of the vertex (0: no medium);
    clamped [n]: the throughput clamp engaged there"""
    return (ROUNDINGS + CLAMP_ROUNDINGS * np.asarray(clamped) + np.abs(sigma_t) + 2.0 * EXPF_ULP * (np.abs(sigma_t) > 0.0)) * 2.0 ** -24


# ---------------------------------------------------------------- scenes
def _write(tmp_path, name, text):
    path = os.path.join(str(tmp_path), name + ".scene")
    with open(path, "w") as f:
        f.write(text)
    return pt.HostScene.load(path, str(tmp_path))


def nested_scene(tmp_path):
    text = "camera target=0,0,0 distance=4 yaw=0.3 pitch=0.2 vfov=12\nrenderer width=%d height=%d maxDepth=48 seed=4242\n" % (WIDTH, HEIGHT)
    text += "background solid=%g,%g,%g\n" % BACKGROUND
    glass = {m: i for i, m in enumerate(NESTED_MATERIALS)}
    for m in range(NESTED_TABLE):
        if m in glass:
            i = glass[m]
            text += "material type=dielectric ior=%g sigmaA=%g,%g,%g\n" % (1.15 + 0.04 * i, 0.05 + 0.03 * i, 0.4 - 0.03 * i, 0.1 + 0.05 * ((i * 3) % 7))
        else:
            text += "material type=lambert albedo=0.5,0.5,0.5\n"
    for i, m in enumerate(NESTED_MATERIALS):
        text += "sphere center=0,0,0 radius=%g material=%d\n" % (NESTED_RADII[i], m)
    return _write(tmp_path, "nested", text)


def mixed_scene(tmp_path, light=0, env=False):
    text = "camera target=0,0.6,0 distance=4.5 yaw=1.2 pitch=0.25 vfov=38\nrenderer width=%d height=%d maxDepth=16 seed=977\n" % (WIDTH, HEIGHT)
    if env:
        text += "background env=%s\n" % ls.write_env(os.path.join(str(tmp_path), "path_state_env.pfm"), ls.env_map("noise", 16, 8))
    else:
        text += "background solid=%g,%g,%g\n" % BACKGROUND
    text += ("material type=lambert albedo=0.35,0.3,0.25\n"                       # 0 floor and walls: maxComp under 0.05 after three bounces
             "material type=dielectric ior=1.5 sigmaA=0.8,0.2,0.05\n"              # 1 the glass box
             "material type=dielectric ior=1.5 thin=on\n"                          # 2 the pane
             "material type=metal albedo=0.99,0.98,0.97 roughness=0.4\n"            # 3 rough metal: maxComp stays above 0.95
             "material type=metal albedo=0.99,0.99,0.99 roughness=0\n"              # 4 smooth metal
             "material type=lambert albedo=0.97,0.97,0.97\n"                        # 5 the back and front walls: bright
             "material type=lambert albedo=0.7,0.65,0.6\n")                         # 6 the floor and the right wall: in between
    text += "rectangle x=-3,3 y=0 z=-3,5 normal=1 material=6\n"
    text += "rectangle x=-3,3 y=0,4 z=-3 normal=1 material=5\n"
    text += "rectangle x=-3 y=0,4 z=-3,5 normal=1 material=0\n"
    text += "rectangle x=3 y=0,4 z=-3,5 normal=-1 material=6\n"
    text += "rectangle x=-3,3 y=0,4 z=5 normal=-1 material=5\n"
    text += "box min=-1.6,0.01,-0.6 max=-0.6,1.1,0.5 material=1\n"
    text += "rectangle x=-0.4,1.8 y=0.02,1.6 z=1.3 normal=1 twoSided=1 material=2\n"
    text += "sphere center=0.6,0.5,-0.4 radius=0.5 material=3\n"
    text += "sphere center=1.7,0.45,0.5 radius=0.45 material=4\n"
    if light:
        text += "material type=diffuse_light emit=3,2.8,2.5\n"
        for i in range(light):   # strips of equal width
            text += "rectangle x=%.9g,%.9g y=3.9 z=-2.5,4 normal=-1 material=7\n" % (-2.5 + 5.0 * i / light, -2.5 + 5.0 * (i + 1) / light)
    return _write(tmp_path, "env" if env else ("lit%d" % light if light else "mixed"), text)


def lit_scene(tmp_path):
    return mixed_scene(tmp_path, light=1)


def nine_lights_scene(tmp_path):
    return mixed_scene(tmp_path, light=9)


def env_scene(tmp_path):
    return mixed_scene(tmp_path, env=True)


def deep_scene(tmp_path):
    text = "camera target=0,0,0 distance=0.5 yaw=0.02 pitch=0.015 vfov=2\nrenderer width=8 height=8 maxDepth=511 seed=31\n"
    text += "background solid=%g,%g,%g\n" % BACKGROUND
    text += "material type=metal albedo=1,1,1 roughness=0\n"
    text += "rectangle x=-1 y=-400,400 z=-400,400 normal=1 twoSided=1 material=0\n"
    text += "rectangle x=1 y=-400,400 z=-400,400 normal=-1 twoSided=1 material=0\n"
    return _write(tmp_path, "deep", text)


def _settings(host, semantics, roulette, max_depth, spec=0, mnee=0, **camera):
    s = host.settings_for()
    s.metalSemantics = semantics
    s.enableRussianRoulette = roulette
    s.enableSpecularNee, s.enableMnee, s.enableMneeSecondary = spec, mnee, mnee
    s.maxDepth = max_depth
    for k, v in camera.items():
        setattr(s, k, v)
    return s


def groups():
    """name -> (scene builder, settings of a loaded scene, vertices a path can have)"""
    out = {}
    for sem in (5, 7):
        out["nested/through/%d" % sem] = (nested_scene, lambda h, sem=sem: _settings(h, sem, 0, 48), 48)
        out["nested/inside/%d" % sem] = (nested_scene, lambda h, sem=sem: _settings(h, sem, 0, 48, cameraDistance=0.72, cameraVerticalFov=40.0), 48)
    for sem in (0, 5):
        out["mixed/%d" % sem] = (mixed_scene, lambda h, sem=sem: _settings(h, sem, 1, 16), 16)
    for variant, (spec, mnee) in (("nee", (0, 0)), ("spec", (1, 0)), ("mnee", (0, 1))):
        out["lit/" + variant] = (lit_scene, lambda h, spec=spec, mnee=mnee: _settings(h, 5, 1, 16, spec=spec, mnee=mnee), 16)
    out["lit/traced"] = (nine_lights_scene, lambda h: _settings(h, 5, 1, 16, spec=1), 16)
    out["env"] = (env_scene, lambda h: _settings(h, 5, 1, 16, spec=1), 16)
    out["deep"] = (deep_scene, lambda h: _settings(h, 0, 0, 511), 511)
    return out


def pixels_of(settings):
    return np.arange(settings.width * settings.height, dtype=np.uint32)


def xys_of(settings, pixels, sample=0):
    p = np.asarray(pixels, np.int64)
    return np.stack([p % settings.width, p // settings.width, np.full(len(p), sample)], axis=1).astype(np.uint32)


def scene_tables(host):
    """what the bookkeeping reads of the scene: per material the type, the thin flag, the absorption; per primitive its material"""
    d = host.desc
    mats = [d.materials[i] for i in range(d.materialCount)]
    types = np.array([int(m.typeEta[0]) for m in mats])
    roughness = np.array([m.baseColorRoughness[3] for m in mats])
    rect_material = np.array([d.rects[i].materialTwoSided[0] for i in range(d.rectCount)], np.int64)
    return dict(type=types, thin=np.array([m.typeEta[3] > 0.5 for m in mats]),
                delta=(types == 2) | ((types == 1) & (roughness <= 1.0e-3)),    # materialIsDelta: such a surface takes no light sample
                env=bool(d.envWidth > 0), emission=np.array([[m.emission[c] for c in range(3)] for m in mats], np.float32),
                lights=int((types[np.minimum(rect_material, len(mats) - 1)] == 3).sum()) if d.rectCount else 0,
                sigma=np.array([[m.dielectricSigmaA[c] for c in range(3)] for m in mats], np.float32),
                sphere_material=np.array([d.spheres[i].materialIndex[0] for i in range(d.sphereCount)], np.int64),
                rect_material=np.array([d.rects[i].materialTwoSided[0] for i in range(d.rectCount)], np.int64), count=d.materialCount)


# ---------------------------------------------------------------- a side's vertices, as one table
ORACLE_ROW = {"valid": 0, "hit": 1, "t": 2, "u:prim_type": 3, "u:prim_index": 4, "u:material": 5, "front": 6, "u:rng_entry": 7, "u:rng_rect": 8,
              "u:rng_env": 9, "u:rng_bsdf": 10, "u:rng_after": 11, "direction": slice(12, 15), "weight": slice(15, 18), "pdf": 18, "is_delta": 19,
              "medium_event": 20, "sampled": 21, "roulette": 22, "roulette_draw": 23, "roulette_threshold": 24, "throughput": slice(25, 28),
              "last_pdf": 28, "last_delta": 29, "u:spec_depth": 30, "u:medium_depth": 31, "u:stack": slice(32, 40), "next_origin": slice(40, 43),
              "next_direction": slice(43, 46), "immediate": slice(46, 49), "queued": slice(49, 52), "u:queued_mask": 52, "ended": 53,
              "u:near": 54, "ray_origin": slice(55, 58), "ray_direction": slice(58, 61), "normal": slice(61, 64), "next_gap": 64}


def oracle_table(rows):
    """[n, cap, 68] rows of OracleScene.path_states -> field -> [cap, n, ..] arrays (vertex first, like the device's snapshots)"""
    rows = np.ascontiguousarray(np.swapaxes(rows, 0, 1))
    return pt.sss_fields(rows, ORACLE_ROW)


def oracle_vertices(host, settings, cap, oracle_lib):
    """the oracle's recorded vertices of every pixel as the table check_vertices takes, plus the raw fields, the radiance and the camera rays"""
    pixels = pixels_of(settings)
    rows, radiance = oracle_lib.OracleScene(host).path_states(settings, pixels, 0, cap)
    t = oracle_table(rows)
    cam, cam_states = oracle_lib.camera_rays(settings, xys_of(settings, pixels))
    v = dict(exists=(t["valid"] != 0) & (t["hit"] != 0) & (t["sampled"] != 0), valid=t["sampled"] == 1, initial_rng=cam_states)
    for f in ("t", "material", "rng_bsdf", "weight", "pdf", "is_delta", "medium_event", "throughput", "last_pdf", "last_delta", "spec_depth",
              "medium_depth", "stack", "rng_after", "ended"):
        v[f] = t[f]
    v["is_delta"], v["medium_event"] = t["is_delta"] != 0, t["medium_event"].astype(np.int64)
    return v, t, radiance, cam, cam_states


def state_before(v, k):
    """the state a side's table `v` (check_vertices) has before vertex k: vertex k - 1's, or a fresh path's"""
    n = v["throughput"].shape[1]
    if k == 0:
        return R.initial_state(n, v["initial_rng"])
    return dict(throughput=v["throughput"][k - 1].astype(np.float64), last_pdf=v["last_pdf"][k - 1].astype(np.float64),
                last_delta=np.asarray(v["last_delta"][k - 1]) != 0, spec_depth=np.asarray(v["spec_depth"][k - 1], np.int64),
                medium_depth=np.asarray(v["medium_depth"][k - 1], np.int64), stack=np.asarray(v["stack"][k - 1], np.int64))


def immediate_radiance(settings, tables, v, k, rows, miss, front, material, t, env, light_pdf):
    """float64: what vertex k of the paths `rows` adds at once, from the side's state before it.  miss [m]: the ray escaped - the
    background (env [m, 4] {radiance, pdf} of the side's environment along the ray, or None: the solid colour), MIS-weighted against
    environment sampling; otherwise an emitter hit (its material, front face, t; light_pdf [m]: the side's rectLightPdfForHit),
    MIS-weighted against rectangle-light sampling.  Returns (radiance [m, 3], relative bound [m])."""
    before = {f: a[rows] for f, a in state_before(v, k).items() if f != "rng"}
    media = bool(settings.metalSemantics & 1)
    att, sigma, on = R.attenuation(before, np.where(miss, 0.0, t), tables["sigma"], media)
    before["throughput"] = before["throughput"] * np.where(miss[:, None], 1.0, att)
    background = env[:, 0:3].astype(np.float64) if env is not None else np.broadcast_to(np.array(BACKGROUND, np.float32).astype(np.float64), (len(rows), 3))
    escaped = R.escaped(settings, before, background, env[:, 3].astype(np.float64) if env is not None else 0.0, tables["env"])
    scale = settings.emissionScale if settings.emissionScale > 0 else 1.0
    emission = tables["emission"][material].astype(np.float32) * np.float32(scale)
    lit = R.emitter(settings, before, np.where(front[:, None], emission.astype(np.float64), 0.0), light_pdf, tables["lights"] > 0)
    sigma_t = (sigma.max(axis=1) * np.maximum(t, 0.0)) * (on & ~miss)
    bound = (IMMEDIATE_ROUNDINGS + 1.0 + sigma_t + 2.0 * EXPF_ULP * (sigma_t > 0.0)) * 2.0 ** -24
    return np.where(miss[:, None], escaped, lit), bound


def check_vertices(settings, tables, v, name):
    """Holds every vertex of a side's table `v` (fields [V, n, ..], vertex k's `before` state being vertex k - 1's `after`) that took a
    BSDF sample to path_state_ref.step given that side's sample.  v: exists [V, n] (the path reaches vertex k and hits a surface there that
    is no emitter), t, material, rng_bsdf (after the sample), weight, pdf, is_delta, medium_event, valid; after the vertex: throughput,
    last_pdf, last_delta, spec_depth, medium_depth, stack, rng_after, ended; and `initial_rng` [n].
    Asserts the discrete state and the random state exactly and the throughput within throughput_bound; returns the figures the tests
    print and count: vertices, the largest throughput deviation as a fraction of its bound, branch counts."""
    V, n = v["exists"].shape
    state = R.initial_state(n, v["initial_rng"])
    counts = dict(vertices=0, depth8=0, push_at_8=0, pop_at_0=0, clamped=0, killed={}, spared={}, worst=0.0, expf_ulp=0.0, max_depth_seen=0)
    for k in range(V):
        rows = np.flatnonzero(v["exists"][k])
        if rows.size == 0:
            break
        sub = {f: a[rows] for f, a in state.items()}
        sub["depth"] = np.full(rows.size, k)
        sub["rng"] = v["rng_bsdf"][k][rows]
        vertex = dict(t=v["t"][k][rows], material=np.minimum(v["material"][k][rows], tables["count"] - 1))
        sample = {f: v[f][k][rows] for f in ("weight", "pdf", "is_delta", "medium_event", "valid")}
        want, info = R.step(settings, sub, vertex, sample, tables["sigma"])
        goes = ~info["ended"]
        got_ended = v["ended"][k][rows] != 0
        assert np.array_equal(got_ended, info["ended"]), (name, k, rows[got_ended != info["ended"]][:8], info["reason"][got_ended != info["ended"]][:8])
        # the random state: the roulette draw is the only consumer after the sample, and only from depth 5 on
        assert np.array_equal(v["rng_after"][k][rows][goes], want["rng"][goes]), (name, k, "rng")
        if k < R.ROULETTE_FROM or not settings.enableRussianRoulette:
            assert not info["roulette_taken"].any() and np.array_equal(v["rng_after"][k][rows][goes], v["rng_bsdf"][k][rows][goes]), (name, k, "a draw before depth 5")
        for f in ("spec_depth", "medium_depth", "last_delta"):
            assert np.array_equal(np.asarray(v[f][k][rows][goes], np.int64), np.asarray(want[f][goes], np.int64)), (name, k, f)
        # every stack entry below the depth (what lies above it is never read)
        live = np.arange(R.MAX_STACK)[None, :] < want["medium_depth"][:, None]
        assert np.array_equal(np.where(live, v["stack"][k][rows], 0)[goes], np.where(live, want["stack"], 0)[goes]), (name, k, "stack")
        assert np.array_equal(v["last_pdf"][k][rows][goes].astype(np.float64), want["last_pdf"][goes]), (name, k, "last_pdf")
        top = np.where(state["medium_depth"][rows] > 0, state["stack"][rows, np.maximum(state["medium_depth"][rows] - 1, 0)], 0)
        sigma_t = (np.maximum(tables["sigma"][top], 0.0).max(axis=1)
                   * np.maximum(vertex["t"], 0.0) * (info["attenuation"] != 1.0).any(axis=1))
        bound = throughput_bound(sigma_t, info["clamped"])
        got = v["throughput"][k][rows].astype(np.float64)
        rel = np.abs(got - want["throughput"]) / np.maximum(np.abs(want["throughput"]), 1e-300)
        ratio = (rel / bound[:, None])[goes]
        assert np.all(ratio <= 1.0), (name, k, "throughput", float(ratio.max()), rows[goes][np.argmax(ratio.max(axis=1))])
        counts["worst"] = max(counts["worst"], float(ratio.max(initial=0.0)))
        medium = goes & (sigma_t > 0.0)
        if medium.any():   # what is left for expf once the roundings and its argument's have had their share, in ulps
            left = (rel[medium].max(axis=1) / 2.0 ** -24 - ROUNDINGS - sigma_t[medium]) / 2.0
            counts["expf_ulp"] = max(counts["expf_ulp"], float(left.max()))
        # branches
        before_depth = state["medium_depth"][rows]
        counts["vertices"] += rows.size
        counts["depth8"] += int((want["medium_depth"] == R.MAX_STACK).sum())
        counts["push_at_8"] += int(((info["medium_event"] > 0) & (before_depth == R.MAX_STACK)).sum())
        counts["pop_at_0"] += int(((info["medium_event"] < 0) & (before_depth == 0)).sum())
        counts["clamped"] += int(info["clamped"].sum())
        counts["killed"][k] = int(info["roulette_killed"].sum())
        counts["spared"][k] = int((info["roulette_taken"] & ~info["roulette_killed"]).sum())
        counts["max_depth_seen"] = k
        # the recorded state carries on (each vertex is held to the float64 step from the side's own state before it)
        for f in ("throughput", "last_pdf", "last_delta", "spec_depth", "medium_depth", "stack"):
            state[f] = np.array(state[f])
            state[f][rows] = v[f][k][rows]
    return counts
