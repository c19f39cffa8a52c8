"""The inputs of test_sss_walk_host.py and test_gpu_sss_walk.py: the materials and input rows of every group of sssWalkBegin and
sssWalkStep, and the three scenes of the whole-walk tests.  No GPU needed to make them; test_sss_walk_host.py shows them fair."""
import importlib
import os

import numpy as np

import bsdf_domain as D
import sss_walk_ref as R

pt = importlib.import_module("metal-pathtracer-arm64_amd")

N = 4096   # rows per group
WIDTH, HEIGHT = 48, 32
_cache = {}


def settings(max_steps=32):
    s = D.settings("sss")
    s.sssMode = 2
    s.sssMaxSteps = max_steps
    return s


def _sss(name):
    m = D._copy({nm: m for nm, _, m in D.materials()}[name])
    m.sssParams[1] = 1.0   # method=randomwalk
    return m


def _variant(base="sss_jade", **fields):
    m = _sss(base)
    for k, v in fields.items():
        arr, i = k.rsplit("_", 1)
        getattr(m, arr)[int(i)] = v
    return m


def begin_materials():
    """group -> material.  coatParams = {roughness, thickness, sample weight, .}; typeEta.y the ior; sssParams.z the coat tint switch."""
    tint = dict(coatTint_0=0.9, coatTint_1=0.7, coatTint_2=0.5, coatParams_1=0.5, coatAbsorption_0=0.3, coatAbsorption_1=0.1, coatAbsorption_2=0.2)
    return {
        "skin": _sss("sss_skin"), "jade": _sss("sss_jade"),
        "coat_weight_0": _variant(coatParams_2=0.0), "coat_weight_1": _variant(coatParams_2=1.0), "coat_weight_half": _variant(coatParams_2=0.5),
        "coat_rough_0.02": _variant(coatParams_0=0.02, coatParams_2=0.5), "coat_rough_0.6": _variant(coatParams_0=0.6, coatParams_2=0.5),
        "ior_1": _variant(typeEta_1=1.0), "ior_1.33": _variant(typeEta_1=1.33), "ior_2": _variant(typeEta_1=2.0),
        "tint_on": _variant(sssParams_2=1.0, **tint), "tint_off": _variant(sssParams_2=0.0, **tint),
    }


def begin_inputs(group, k=N):
    """(inputs [k, 12] {point, entry normal, wo, incident = -wo}, states [k]): normals of every kind of bsdf_domain.normals in turn; wo at
    normal incidence (1/8 of the rows), at a cosine in [0.05, 1] (3/8), from 0.05 down to 1e-3 above the horizon (2/8), below it (2/8)."""
    rng = np.random.default_rng(D._seed("sss begin " + group))
    kinds = np.arange(k) % 3
    parts = [D.normals(a, k, rng) for a in D.NORMALS]
    n = np.where((kinds == 0)[:, None], parts[0], np.where((kinds == 1)[:, None], parts[1], parts[2]))
    cls = (np.arange(k) // 3) % 8
    cos = np.where(cls < 3, rng.uniform(0.05, 1.0, k), np.where(cls < 5, np.exp(rng.uniform(np.log(1e-3), np.log(0.05), k)),
                                                                 -np.exp(rng.uniform(np.log(1e-3), 0.0, k))))
    wo = D._at_cosine(n, cos, rng)
    wo = np.where((cls == 7)[:, None], n, wo)
    point = rng.uniform(-2, 2, size=(k, 3)).astype(np.float32)
    states = rng.integers(1, 2**32 - 1, size=k, dtype=np.uint64).astype(np.uint32)
    return np.concatenate([point, n, wo, -wo], axis=1).astype(np.float32), states


def step_groups():
    """group -> (material, sssMaxSteps, step rule).  The anisotropy g is sssSigmaS.w; step rule 'recorded' keeps the recorded step,
    -1 / -2 set step = limit - 1 / max(limit - 2, 0)."""
    out = {"skin": (_sss("sss_skin"), 32, "recorded"), "jade": (_sss("sss_jade"), 32, "recorded")}
    for g in (0.0, 9e-4, 1.1e-3, 0.5, -0.5, 1.0, -1.0):
        out["g_%g" % g] = (_variant(sssSigmaS_3=g), 32, "recorded")
    for limit in (0, 1, 2, 32):
        for back in (1, 2):
            out["limit_%d_minus_%d" % (limit, back)] = (_sss("sss_skin"), limit, -back)
    return out


def _choose_states(rng, k, material, want_beyond):
    """random states whose first draw gives a free flight of more than twice want_beyond [k] (NaN: any state)"""
    m = R.Material(material)
    states = rng.integers(1, 2**32 - 1, size=(k, 64), dtype=np.uint64).astype(np.uint32)
    u, _ = R.lr.rng_draw(states.reshape(-1), 1)
    dist = (-np.log(1.0 - np.clip(u[:, 0], R.XI_LO, R.XI_HI)) / m.sigma_t_scalar).reshape(k, 64)
    ok = np.isnan(want_beyond)[:, None] | (dist > 2.0 * np.nan_to_num(want_beyond)[:, None])
    first = np.argmax(ok, axis=1)
    return states[np.arange(k), first]


SYNTHETIC = ("miss", "t_0", "t_5e-5", "t_1e-4", "t_10", "normal_zero", "normal_nan", "normal_inf", "normal_long", "perpendicular", "tir",
             "thr_5e-4", "thr_2e-3")


def step_inputs(group, recorded, k=N):
    """(rows [k, 20], states [k], kind [k]): three quarters recorded steps of a whole walk (`recorded`: (rows [., 20], states) of a walk
    probe), one quarter the synthetic rows of SYNTHETIC in turn (kind = its index + 1; 0 for a recorded row)."""
    material, limit_setting, rule = step_groups()[group]
    rng = np.random.default_rng(D._seed("sss step " + group))
    rec_rows, rec_states = recorded
    pick = rng.integers(0, len(rec_rows), size=k)
    rows = np.ascontiguousarray(rec_rows[pick, :20], np.float32).copy()
    rows[:, 18:20] = 0.0
    states = rec_states[pick].copy()
    words = rows.view(np.uint32)
    # (a miss four times and total internal reflection three times in the turn of eighteen, so that either branch holds 5 % of the rows)
    turn = np.array([SYNTHETIC.index(s) for s in SYNTHETIC + ("miss",) * 3 + ("tir",) * 2])
    kind = np.where(np.arange(k) % 4 == 3, 1 + turn[(np.arange(k) // 4) % len(turn)], 0)
    name = lambda s: kind == 1 + SYNTHETIC.index(s)
    syn = kind > 0
    # a synthetic row starts from a plain boundary query: a unit direction, a hit at t = 1e-3 with the normal against the direction,
    # throughput 1; the free flight beyond the hit unless the row asks for something else
    d = D._unit(rng.normal(size=(k, 3))).astype(np.float32)
    rows[syn, 0:3] = rng.uniform(-1, 1, size=(k, 3)).astype(np.float32)[syn]
    rows[syn, 3:6] = d[syn]
    rows[syn, 6:9] = 1.0
    rows[syn, 10], rows[syn, 11] = 1.0, 1e-3
    rows[syn, 15:18] = -d[syn]
    beyond = np.where(syn, 1e-3, np.nan)
    rows[name("miss"), 10] = 0.0
    for s, t in (("t_0", 0.0), ("t_5e-5", 5e-5), ("t_1e-4", 1e-4), ("t_10", 10.0)):
        rows[name(s), 11] = t
        beyond[name(s)] = np.nan if t == 10.0 else 1e-4
    rows[name("normal_zero"), 15:18] = 0.0
    rows[name("normal_nan"), 16] = np.nan
    rows[name("normal_inf"), 17] = np.inf
    rows[name("normal_long"), 15:18] *= 3.0
    rows[name("perpendicular"), 3:6] = np.array([1, 0, 0], np.float32)
    rows[name("perpendicular"), 15:18] = np.array([0, 1, 0], np.float32)
    # beyond the critical angle of ior 1.5 (41.8 degrees): 60 degrees of incidence
    rows[name("tir"), 3:6] = np.array([np.sqrt(0.75), -0.5, 0], np.float32)
    rows[name("tir"), 15:18] = np.array([0, 1, 0], np.float32)
    rows[name("thr_5e-4"), 6:9] = 5e-4
    rows[name("thr_2e-3"), 6:9] = 2e-3
    rows[syn, 12:15] = (rows[syn, 0:3].astype(np.float64) + rows[syn, 3:6].astype(np.float64) * rows[syn, 11:12]).astype(np.float32)
    chosen = _choose_states(rng, k, material, beyond)
    states = np.where(syn, chosen, states).astype(np.uint32)
    limit = max(limit_setting, 1)
    if rule != "recorded":
        words[:, 9] = max(limit + rule, 0)
    else:
        words[syn, 9] = rng.integers(0, 30, size=k).astype(np.uint32)[syn]
    return rows, states, kind


# ---------------------------------------------------------------- whole walks
_HEAD = ("camera target=0,0,0 distance=5 yaw=0.6 pitch=0.3 vfov=30\n"
         "renderer width=%d height=%d maxDepth=2 seed=1337 sss=randomwalk\n"
         "background solid=0.5,0.6,0.8\n"
         "material type=lambert albedo=0.7,0.7,0.7 name=inner\n"
         "material type=sss albedo=0.8,0.5,0.3 mfp=0.3 method=randomwalk name=walker\n") % (WIDTH, HEIGHT)
SCENES = ("sphere", "cube_outward", "cube_inward")
BACKGROUND = np.array([0.5, 0.6, 0.8], np.float32)
CUBE_HALF, INNER_RADIUS = 0.9, 0.35


def scene(name, tmp_path):
    """(host scene, its analytic twin) of one of SCENES: a walker (sphere of radius 1, or a cube of half side 0.9 written to tmp_path as
    an OBJ of 12 triangles, wound outward or inward) holding the small Lambert sphere that lets a walk leave (bsdf.h: sssWalkStep)."""
    inner = "sphere center=0,0,0 radius=%g material=0\n" % INNER_RADIUS
    if name == "sphere":
        text = _HEAD + "sphere center=0,0,0 radius=1 material=1\n" + inner
        twin = R.AnalyticScene(spheres=[((0, 0, 0), 1.0), ((0, 0, 0), INNER_RADIUS)])
    else:
        inward = name == "cube_inward"
        obj = os.path.join(str(tmp_path), name + ".obj")
        with open(obj, "w") as f:
            f.write(R.cube_obj((0, 0, 0), CUBE_HALF, inward))
        text = _HEAD + "mesh path=%s material=walker\n" % os.path.basename(obj) + inner
        twin = R.AnalyticScene(spheres=[((0, 0, 0), INNER_RADIUS)], triangles=R.cube_triangles((0, 0, 0), CUBE_HALF, inward))
    path = os.path.join(str(tmp_path), name + ".scene")
    with open(path, "w") as f:
        f.write(text)
    return pt.HostScene.load(path, str(tmp_path)), twin


def walk_settings(host, max_steps=32):
    s = host.settings_for(width=WIDTH, height=HEIGHT, max_depth=2, seed=1337)
    s.metalSemantics = pt.PTR_METAL_SSS
    s.enableRussianRoulette = 0
    s.sssMaxSteps = max_steps
    assert s.sssMode == 2
    return s


def all_pixels():
    ys, xs = np.mgrid[0:HEIGHT, 0:WIDTH]
    return np.stack([xs.ravel(), ys.ravel(), np.zeros(WIDTH * HEIGHT, np.int64)], axis=1).astype(np.uint32)


def recorded_steps(steps):
    """(rows [m, 24], states before [m]) of the steps a walk probe recorded (`steps`: the first dict sss_walks returns): every step that was
    taken, which is every row with a non-zero direction."""
    raw = steps["raw"].reshape(-1, 24)
    taken = np.any(raw[:, 3:6] != 0.0, axis=1)
    return raw[taken], raw.view(np.uint32)[taken, 18]


# ---------------------------------------------------------------- comparing a side (oracle or device) with the float64 reference
# test_gpu_parity.test_sample_bsdf_matches_oracle on the subsurface materials: direction atol 2e-4; weight, pdf and throughput rtol 3e-3,
# atol 1e-5.  A position is a sum of three terms of size <= 2.1 in float32 (ulp 2.4e-7): atol 1e-6.
DIR_ATOL, RTOL, ATOL, POS_ATOL = 2e-4, 3e-3, 1e-5, 1e-6

# Against float64 a group that needs more than those bounds gets it by the one rule: move normal and wo one float32 ulp in float64 (eight
# patterns), take the reference's own change, times 4, row by row (begin_sensitivity).  The groups that need it are those whose coat lobe is
# narrow: at coat roughness 0.05 alpha^2 = 6e-6 (at 0.02: 1.6e-7) and ggx_D's denominator c^2 (alpha^2 - 1) + 1 is of that size at the peak.
# DERIVED records, per such group, the largest addition the rule gives (relative for weight, pdf and their product); it comes from the
# reference alone and test_sss_walk_host.py asserts that it is what is written here.
SENSITIVE_BEGIN = ("skin", "jade", "coat_weight_1", "coat_weight_half", "coat_rough_0.02", "ior_1", "ior_1.33", "ior_2", "tint_on", "tint_off")
DERIVED = {   # group -> the largest addition to {direction (absolute), weight, pdf, weight x pdf product (relative)}
    "skin": (1.20280e-06, 0.438697, 0.492731, 0.0257060), "jade": (8.68184e-06, 0.297875, 0.321843, 0.0203070),
    "coat_weight_1": (3.18570e-05, 0.496937, 0.567409, 0.0256278), "coat_weight_half": (5.06664e-05, 0.341535, 0.373420, 0.0235716),
    "coat_rough_0.02": (6.69653e-06, 21.7462, 2.33221e+07, 0.139511), "ior_1": (1.24902e-06, 0.298420, 0.322479, 0.299217),
    "ior_1.33": (6.09976e-06, 0.327465, 0.356664, 0.0264815), "ior_2": (1.17113e-05, 0.303818, 0.328791, 0.0148471),
    "tint_on": (2.28964e-05, 0.298928, 0.323073, 0.0308240), "tint_off": (3.47857e-06, 0.426339, 0.477200, 0.0234946),
}
DERIVED = {g: dict(zip(("direction", "weight", "pdf", "product"), v)) for g, v in DERIVED.items()}
SENSITIVITY_SEEN = {}   # group -> field -> the largest finite addition of the run (held to DERIVED)
# What the rule cannot give, because the reference does not move where float32 rounds: rows the reference itself marks as beyond float32
# are EXCLUDED from the strict comparison of the value in question, held to a looser statement that float32 can meet, and their share
# of the group is capped by the figure below (from the reference alone; 0 for a group not named):
#   coat_rough_0.02  one rounding of ggx_D's cosine moves D by half its size or more (ill_conditioned): weight and pdf each are noise,
#                    their product weight x max(pCoat pdf, 1e-6) = value x cos is not (D cancels, or the tail clamp has flattened it) and
#                    is held to the strict bound there as everywhere
#   ior_1            cosT = sqrt(1 - (1 - cos^2)) loses what 1 - cos^2 rounds away: the throughput of a grazing entry is held to 4 x
#                    that rounding (entry_slack) where it exceeds the strict bound
#   g_0.0011         (1 + g^2 - s^2) / (2 g) just past the isotropic switch: the scattered direction is held to 4 x hg_slack on top
EXCLUDED_CAP = {"coat_rough_0.02": 0.32, "ior_1": 0.11, "g_0.0011": 0.62}
# Rows that miss the strict bound all the same (a cosine at the lobe's peak is stationary in the inputs, so the rule says nothing there,
# while a float32 cosine still lands 6e-8 off) count with the near ties towards the one cap of 2 %, and must still lie within 4 x what
# one such rounding does by the reference's own slope of D (d_cond) or of the azimuth (azimuth_slack): no row goes unbounded.


def _perturbed(inputs, rng):
    x = np.array(inputs, np.float32)
    for cols in (slice(3, 6), slice(6, 9)):
        x[:, cols] = D.one_ulp(x[:, cols], rng.random(x[:, cols].shape) < 0.5)
    x[:, 9:12] = -x[:, 6:9]
    return x


def _product(weight, pdf, p_coat):
    """weight x max(pCoat pdf, 1e-6): the coat sample's value x cos, whatever its pdf"""
    return weight * np.maximum(p_coat * pdf, R.f32(1e-6))[:, None]


def begin_sensitivity(material, settings, inputs, states, ref):
    """(field -> [n] or [n, 3]: 4 x the largest change of the reference's sample when normal and wo move by one float32 ulp, eight random
    patterns of directions; [n] bool: the rows whose outcome changes with them)"""
    rng = np.random.default_rng(D._seed("sss sensitivity"))
    p_coat = R.Material(material).p_coat
    mine = dict(ref, product=_product(ref["weight"], ref["pdf"], p_coat))
    extra = {f: np.zeros_like(mine[f]) for f in ("direction", "weight", "pdf", "product")}
    unstable = np.zeros(len(ref["outcome"]), bool)
    for _ in range(8):
        other = R.begin(material, settings, _perturbed(inputs, rng), states)
        other["product"] = _product(other["weight"], other["pdf"], p_coat)
        unstable |= other["outcome"] != ref["outcome"]
        for f in extra:
            extra[f] = np.maximum(extra[f], 4.0 * np.abs(other[f] - mine[f]))
    return extra, unstable


def _close(got, want, rtol, atol, extra=0.0):
    return np.abs(got - want) <= atol + rtol * np.abs(want) + extra


def _rows(good):
    return good.reshape(len(good), -1).all(axis=1) if len(good) else np.zeros(0, bool)


def assert_begin_values(group, got, ref, ok, material, settings, inputs, states):
    """The rows of a side (pt.sss_fields of SSS_BEGIN_FIELDS) against the reference, in the rows `ok` whose outcomes agree.  Returns
    (outside, excluded): the rows that miss the strict bound (the caller caps them with the near ties) and the rows the reference marks
    as beyond float32 (the caller caps them by EXCLUDED_CAP)."""
    k = len(ref["outcome"])
    sample, walking = ok & (ref["outcome"] == R.SAMPLE), ok & (ref["outcome"] == R.WALKING)
    p_coat = R.Material(material).p_coat
    mine = dict(ref, product=_product(ref["weight"], ref["pdf"], p_coat))
    theirs = dict(got, product=_product(got["weight"].astype(np.float64), got["pdf"].astype(np.float64), p_coat))
    outside = np.zeros(k, bool)
    extra = {}
    if group in SENSITIVE_BEGIN:
        extra, unstable = begin_sensitivity(material, settings, inputs, states, ref)
        outside |= ok & unstable
        sample, walking = sample & ~unstable, walking & ~unstable
        compared = lambda f: sample & ~ref["azimuth_free"] if f == "direction" else sample
        relative = lambda f: extra[f][compared(f)] / (1.0 if f == "direction" else np.maximum(np.abs(mine[f][compared(f)]), 1e-30))
        SENSITIVITY_SEEN[group] = {f: float(np.max(relative(f), initial=0.0)) for f in extra}
    ill = sample & ref["ill_conditioned"]
    grazing = walking & (4.0 * ref["entry_slack"] > RTOL)
    excluded = ill | grazing
    free = sample & ref["azimuth_free"]   # (normal incidence: the azimuth about the normal is rounding noise on every side)
    one_rounding = {"direction": 4.0 * ref["azimuth_slack"], "weight": 4.0 * 6e-8 * ref["d_cond"], "pdf": 4.0 * 6e-8 * ref["d_cond"],
                    "product": 4.0 * 6e-8 * ref["d_cond"]}
    for rows, f, rtol, atol in ((sample & ~free, "direction", 0.0, DIR_ATOL), (sample & ~ill, "weight", RTOL, ATOL), (sample & ~ill, "pdf", RTOL, ATOL),
                                (sample, "product", RTOL, ATOL), (walking, "direction", 0.0, DIR_ATOL), (walking & ~grazing, "weight", RTOL, ATOL),
                                (walking, "position", 0.0, POS_ATOL)):
        if not rows.any():
            continue
        g, w = theirs[f][rows].astype(np.float64), mine[f][rows]
        add = extra[f][rows] if f in extra else 0.0
        missed = ~_rows(_close(g, w, rtol, atol, add))
        outside[np.flatnonzero(rows)[missed]] = True
        # ... and a row that misses is still within what one rounding of the cosine (or of the azimuth) does, by the reference's own slope
        slack = one_rounding.get(f, np.zeros(k))[rows]
        slack = slack if f == "direction" else slack * np.abs(w).reshape(len(w), -1).max(axis=1)
        bounded = _rows(_close(g, w, rtol, atol, add + (slack[:, None] if g.ndim == 2 else slack)))
        # (no such slope for a row that enters the medium: there a miss fails)
        assert bounded[missed].all(), (group, f, int((~bounded).sum()), int(rows.sum()), float(np.max(np.abs(g - w), initial=0.0)))
    cos = lambda side: np.einsum("ij,ij->i", side["direction"][free].astype(np.float64), ref["normal"][free])
    assert _close(cos(got), cos(ref), 0.0, DIR_ATOL).all(), group
    # a grazing entry at ior 1: the throughput within 4 x the rounding of its transmitted cosine
    bound = 4.0 * (ref["entry_slack"] * np.abs(ref["weight"]).max(axis=1))[grazing][:, None]
    assert _close(got["weight"][grazing].astype(np.float64), ref["weight"][grazing], RTOL, ATOL, bound).all(), group
    assert free.mean() <= 0.126   # (one row in eight is at normal incidence, by begin_inputs)
    return outside, excluded


def assert_step_values(group, got, ref, ok, material, limit, rows, states):
    """The rows of a side (SSS_STEP_FIELDS) against the reference: the walk state where the walk goes on, the throughput and the step as the
    pass left them everywhere, the exit sample where the path leaves.  Returns the rows outside the strict bound and the rows EXCLUDED from the strict bound on the direction
    (a small g just past the isotropic switch: EXCLUDED_CAP), which are held to 4 x hg_slack on top instead."""
    walking, sample = ok & (ref["outcome"] == R.WALKING), ok & (ref["outcome"] == R.SAMPLE)
    scale = np.maximum(1.0, np.abs(ref["position"]).max(axis=1))[:, None]
    loose = walking & (4.0 * ref["hg_slack"] > 0.0) if group in EXCLUDED_CAP else np.zeros(len(ok), bool)
    # (a scattered direction that misses the strict bound - a cosine next to 1 or -1 turns its rounding into 1 / sin as much of the
    # direction - counts with the near ties towards their cap, and is still within 4 x hg_slack on top)
    strict = _rows(_close(got["direction"].astype(np.float64), ref["direction"], 0.0, DIR_ATOL))
    outside = walking & ~loose & ~strict
    checks = ((walking, "position", 0.0, POS_ATOL * scale), (walking, "direction", 0.0, DIR_ATOL + 4.0 * ref["hg_slack"][:, None]),
              (ok, "throughput", RTOL, ATOL), (sample, "exit_direction", 0.0, DIR_ATOL),
              (sample, "exit_weight", RTOL, ATOL), (sample, "exit_point", 0.0, 0.0))
    for sel, f, rtol, atol in checks:
        a = atol[sel] if isinstance(atol, np.ndarray) else atol
        g, w = got[f][sel].astype(np.float64), ref[f][sel]
        with np.errstate(invalid="ignore"):
            good = _close(g, w, rtol, a) | (np.isnan(g) & np.isnan(w)) | (g == w)
        assert good.all(), (group, f, int((~good).sum()), int(sel.sum()), np.flatnonzero(~_rows(good))[:5])
    assert np.array_equal(got["step"][ok], ref["step"][ok]), group
    assert np.all(got["exit_pdf"][sample] == 1.0) and np.all(got["has_exit"][sample] == 1.0), group
    assert np.all(got["raw"][ok & (ref["outcome"] != R.SAMPLE), 11:] == 0.0), group
    return outside, loose


# ---------------------------------------------------------------- the float64 walk over analytic hits
def reference_walks(host, twin, settings, camera_rays, camera_states):
    """The first bounce with its whole walk in float64: camera rays (float32, as the camera probe gives them) and the random states
    after them; closest hits from the analytic twin; begin and step from sss_walk_ref.  Returns first_hit, started, queries, outcome
    (final), outcomes [n, limit] (-1 past the end), hits per step (hit, t, point, normal), states."""
    walker = host.desc.materials[1]
    assert int(walker.typeEta[0]) == 5 and walker.sssParams[1] >= 0.5
    o, d = camera_rays[:, 0:3].astype(np.float64), camera_rays[:, 3:6].astype(np.float64)
    k = len(o)
    limit = max(int(settings.sssMaxSteps), 1)
    hit, t, p, nrm = twin.closest(o, d)
    inner = hit & (np.abs(np.linalg.norm(p, axis=1) - INNER_RADIUS) < 1e-6)
    front = _dot3(d, nrm) < 0.0
    started = hit & ~inner & front
    inc = d / np.linalg.norm(d, axis=1, keepdims=True)
    inputs = np.concatenate([p, nrm, -inc, inc], axis=1).astype(np.float32)
    b = R.begin(walker, settings, inputs, camera_states)
    outcome = np.where(started, b["outcome"], -1)
    states = np.where(started, b["states"], camera_states).astype(np.uint32)
    pos, direction, thr = b["position"].copy(), b["direction"].copy(), b["weight"].copy()
    stp = np.zeros(k, np.uint32)
    outcomes = np.full((k, limit), -1)
    queries = np.zeros(k, np.int64)
    near = started & R.near_ties(b)
    for q in range(limit):
        live = started & (outcome == R.WALKING)
        if not live.any():
            break
        bh, bt, bp, bn = twin.closest(pos, direction)
        rows = np.zeros((k, 20), np.float32)
        rows[:, 0:3], rows[:, 3:6], rows[:, 6:9] = pos, direction, thr
        rows.view(np.uint32)[:, 9] = stp
        rows[:, 10], rows[:, 11], rows[:, 12:15], rows[:, 15:18] = bh, bt, bp, bn
        r = R.step(walker, settings.sssMaxSteps, rows, states)
        near |= live & R.near_ties(r)
        outcome = np.where(live, r["outcome"], outcome)
        outcomes[live, q] = r["outcome"][live]
        pos, direction = np.where(live[:, None], r["position"], pos), np.where(live[:, None], r["direction"], direction)
        thr, stp = np.where(live[:, None], r["throughput"], thr), np.where(live, r["step"], stp)
        states = np.where(live, r["states"], states).astype(np.uint32)
        queries += live
    return dict(first_hit=hit, started=started, queries=queries, outcome=outcome, outcomes=outcomes, states=states, near=near)


def _dot3(a, b):
    return np.einsum("ij,ij->i", a, b)


def walks_agree(steps, final, ref):
    """[n] bool: the recorded walk of a side (sss_walks) has the reference's sequence of outcomes, query count and final outcome, and
    the random state the reference has when its walk ends."""
    n, cap = steps["outcome"].shape
    limit = ref["outcomes"].shape[1]
    took = np.arange(cap)[None, :] < final["queries"].astype(np.int64)[:, None]
    seq = np.where(took, steps["outcome"].astype(np.int64), -1)[:, :limit]
    same = (seq == ref["outcomes"][:, :cap]).all(axis=1) & (final["queries"].astype(np.int64) == ref["queries"])
    same &= np.where(ref["started"], final["outcome"].astype(np.int64) == ref["outcome"], final["outcome"] == -1)
    last_state = np.where(final["queries"] > 0, steps["state_after"][np.arange(n), np.maximum(final["queries"].astype(np.int64) - 1, 0) % cap], 0)
    same &= np.where(ref["queries"] > 0, last_state == ref["states"], True)
    return same
