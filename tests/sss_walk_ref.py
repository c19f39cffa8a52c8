"""Float64 restatement of the random-walk subsurface path of the Metal integrator: the yardstick of test_sss_walk_host.py (oracle) and
test_gpu_sss_walk.py (device).

Written from the shader (shaders/pathtrace.metal: sample_sss_random_walk_software 4060-4311, the Henyey-Greenstein sampler 4003-4033,
offset_surface_point 1210-1220, and what those call: the coat helpers 3825-3894, the medium coefficients 3916-3948, fresnel_dielectric_exact
3645-3674, the GGX terms 3699-3797, build_onb 934-940), cut into the same two pieces the integrator is cut into: `begin` is the function up
to the loop, `step` one pass of the loop body given the closest hit of the walk's ray.  Plain numpy on whole batches, everything continuous
in float64 from the float32 inputs; random numbers from light_ref.rng_draw.  It shares no code with the oracle or the kernels.

Besides its results every function returns the *margin* of each decision it takes: the signed distance of the compared quantity from its
threshold, NaN in rows that never reach the decision.  `near_ties` turns the margins into the rows whose outcome a float32 evaluation may
legitimately decide the other way; BANDS says how wide each band is and why.  A margin of exactly zero is no tie: from float32 inputs a
float64 difference vanishes only where every product in it is exact (axis-aligned vectors, a value equal to its threshold), and there the
float32 evaluation is exact too and must decide as the shader's comparison reads.
"""
import numpy as np

import light_ref as lr

PI = np.pi
FALLBACK, SAMPLE, WALKING = 0, 1, 2


def f32(x):
    """the value of a float32 literal of the shader, as a float64"""
    return float(np.float32(x))


EPS = f32(1e-4)            # kRayOriginEpsilon
CUTOFF = f32(1e-3)         # kSssThroughputCutoff
FRAME_Z = f32(0.999)       # build_onb's switch of the up vector
XI_LO, XI_HI = f32(1e-6), float(np.float32(1.0) - np.float32(1e-6))

# Width of the near-tie band of each decision: (absolute, relative to the threshold side).  Unit vectors carry about 1 ulp (6e-8) per
# component after a float32 normalize, a dot product of two of them 3 roundings more: 4e-7 bounds it; reflecting or refracting first
# doubles that.  The free-flight distance is -log(1 - xi) / sigma: 1 - xi rounds by at most 2^-25 = 3e-8 where xi is small, which is an
# absolute 3e-8 / sigma of distance, plus the 2-ulp logf and the division, relative.  A throughput is a product of two or three expf of
# arguments up to 14 (xi is clamped at 1 - 1e-6), whose argument rounding (1 ulp of 14) is a relative 8e-7 of the value each.
BANDS = {
    "lobe": (0.0, 0.0),                # rand < pCoat: both float32 values as given; exact on every side
    "hg_isotropic": (0.0, 0.0),        # |g| < 1e-3: g is the material's float32 value, clamped exactly
    "coat_wh": (1e-6, 0.0),            # dot(wh, n) <= 0
    "coat_cos_i": (2e-6, 0.0),         # dot(n, wi) <= 0 with wi = reflect(-wo, wh)
    "coat_cos_o": (4e-7, 0.0),         # dot(n, wo) <= 0
    "coat_wi_wh": (2e-6, 0.0),         # dot(wi, wh) <= 0
    "coat_pdf": (2e-6, 0.0),           # ggx_pdf's own three cosines
    "entry_cos": (4e-7, 0.0),          # dot(-incident, n) <= 0
    "frame": (4e-7, 0.0),              # |n.z| < 0.999 in build_onb (another frame is another sample)
    "free_flight": (0.0, 4e-6),        # distance < boundaryDistance; plus 1.2e-7 / sigma absolute (see near_ties)
    "cutoff": (0.0, 6e-6),             # max throughput < 1e-3
    "exit_cos": (4e-7, 0.0),           # cosExitI > 0
    "tir": (8e-6, 0.0),                # k = 1 - eta^2 (1 - ndi^2) < 0, eta up to 2: eta^2 x the 4e-7 of ndi, x 2 for ndi^2, x 2.5
}
DECISIONS = tuple(BANDS)
COAT_ORDER = ("coat_wh", "coat_cos_i", "coat_cos_o", "coat_wi_wh", "coat_pdf")   # the order the shader rejects in (4107-4137)


def _dot(a, b):
    return np.einsum("ij,ij->i", a, b)


def _unit(v):
    """safe_normalize: zero for a zero vector"""
    l2 = _dot(v, v)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where((l2 > 0.0)[:, None], v / np.sqrt(l2)[:, None], 0.0)


def _finite3(v):
    return np.isfinite(v).all(axis=1)


class Material:
    """What the walk reads of a PtrMaterial, in float64."""

    def __init__(self, m):
        g = lambda a: np.array([float(x) for x in a])
        coat, tint, absorb = g(m.coatParams), g(m.coatTint), g(m.coatAbsorption)
        self.p_coat = float(np.clip(coat[2], 0.0, 1.0))
        self.coat_roughness = max(float(np.clip(coat[0], 0.0, 1.0)), f32(1e-3))
        self.eta = max(float(m.typeEta[1]), 1.0)
        ratio = (self.eta - 1.0) / max(self.eta + 1.0, f32(1e-6))
        self.f0 = float(np.clip(ratio * ratio, 0.0, f32(0.999)))
        t = np.clip(tint[:3], 0.0, 1.0)
        thickness, a = max(coat[1], 0.0), np.maximum(absorb[:3], 0.0)
        self.spec_tint = t if (thickness <= 0.0 or (a <= f32(1e-6)).all()) else np.clip(t * np.exp(-a * thickness), 0.0, 1.0)
        self.tinted = float(m.sssParams[2]) > 0.5
        self.g_raw = float(m.sssSigmaS[3])
        self.g = float(np.clip(self.g_raw, f32(-0.99), f32(0.99)))
        mfp = max(float(m.sssParams[0]), f32(1e-4))
        reduce = max(1.0 - self.g, f32(0.01))
        sa, ss = g(m.sssSigmaA), g(m.sssSigmaS)
        if sa[3] > 0.5:
            self.sigma_a = np.maximum(sa[:3], f32(1e-6))
            self.sigma_s = np.maximum(ss[:3], 0.0) * reduce
        else:
            sigma_t = 1.0 / max(mfp, f32(1e-4))
            base = np.clip(g(m.baseColorRoughness)[:3], 0.0, 1.0)
            self.sigma_s = np.maximum(np.clip(base, 0.0, f32(0.999)) * sigma_t, 0.0) * reduce
            self.sigma_a = np.maximum(sigma_t - self.sigma_s, f32(1e-6))
        self.sigma_t = np.maximum(self.sigma_a + self.sigma_s, f32(1e-6))
        self.sigma_t_scalar = max(float(self.sigma_t.max()), f32(1e-4))
        self.albedo = np.clip(self.sigma_s / np.maximum(self.sigma_t, f32(1e-6)), 0.0, 1.0)


class Clamps:
    """make_firefly_params (3537-3548) of the settings, as the two clamps of the coat lobe read them."""

    def __init__(self, settings, metal_clamps_bit=64):
        self.enabled = bool(settings.fireflyClampEnabled)
        self.floor = max(float(settings.fireflyClampFloor), 0.0)
        self.tail_base = max(float(settings.specularTailClampBase), 0.0)
        self.tail_scale = max(float(settings.specularTailClampRoughnessScale), 0.0)
        self.metal = bool(settings.metalSemantics & metal_clamps_bit)
        self.min_pdf_raw = float(settings.minSpecularPdf)
        self.min_pdf = max(self.min_pdf_raw, f32(1e-8))

    def spec_pdf(self, pdf):
        if self.metal:   # 3579-3590
            ok = np.isfinite(pdf) & (pdf > 0.0)
            return np.where(ok, pdf if self.min_pdf_raw <= 0.0 else np.maximum(pdf, self.min_pdf_raw), 0.0)
        return np.where(np.isfinite(pdf), np.maximum(pdf, self.min_pdf), self.min_pdf)

    def spec_tail(self, value, roughness, f0):   # 3608-3633
        fin = _finite3(value)
        positive = np.where(fin[:, None], np.maximum(value, 0.0), 0.0)
        if not self.enabled or (self.metal and self.tail_base <= 0.0 and self.tail_scale <= 0.0):
            return positive
        limit = max((self.tail_base + self.tail_scale * roughness) * max(f0, f32(1e-3)), self.floor)
        lum = positive @ np.array([f32(0.2126), f32(0.7152), f32(0.0722)])
        scale = np.where((lum > limit) & (lum > 0.0), limit / np.maximum(lum, f32(1e-6)), 1.0)
        return positive * scale[:, None]


def frame(n):
    """build_onb of the unit vector n: (tangent, bitangent, margin of its |n.z| < 0.999)"""
    z = np.abs(n[:, 2])
    up = np.where((z < FRAME_Z)[:, None], np.array([[0.0, 0.0, 1.0]]), np.array([[1.0, 0.0, 0.0]]))
    t = _unit(np.cross(up, n))
    return t, np.cross(n, t), FRAME_Z - z


def _ggx_lambda(alpha, c):
    c = np.abs(c)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.sqrt(np.maximum(0.0, 1.0 - c * c))
        a = alpha * (s / c)
        return np.where((c <= 0.0) | (s == 0.0), 0.0, (-1.0 + np.sqrt(1.0 + a * a)) * 0.5)


def _ggx_g1(alpha, c):
    return 1.0 / (1.0 + _ggx_lambda(alpha, c))


def _ggx_d(alpha, c):
    a2 = alpha * alpha
    d = c * c * (a2 - 1.0) + 1.0
    return a2 / (PI * d * d)


def _fresnel(cos_i, eta_i, eta_t):
    """fresnel_dielectric_exact: (reflectance, cos of the transmitted angle)"""
    ac = np.abs(np.clip(cos_i, -1.0, 1.0))
    sin_t2 = (eta_i / eta_t) ** 2 * np.maximum(0.0, 1.0 - ac * ac)
    tir = sin_t2 >= 1.0
    cos_t = np.sqrt(np.maximum(0.0, 1.0 - sin_t2))
    with np.errstate(divide="ignore", invalid="ignore"):
        rs = (eta_i * ac - eta_t * cos_t) / (eta_i * ac + eta_t * cos_t)
        rp = (eta_t * ac - eta_i * cos_t) / (eta_t * ac + eta_i * cos_t)
    return np.where(tir, 1.0, 0.5 * (rs * rs + rp * rp)), np.where(tir, 0.0, cos_t)


def _refract(i, n, eta):
    """MSL refract(): (direction - zero on total internal reflection -, k)"""
    ndi = _dot(n, i)
    k = 1.0 - eta * eta * (1.0 - ndi * ndi)
    r = eta * i - (eta * ndi + np.sqrt(np.maximum(k, 0.0)))[:, None] * n
    return np.where((k < 0.0)[:, None], 0.0, r), k


def offset_surface_point(point, normal, direction):   # 1210-1220
    ok = _finite3(normal) & (_dot(normal, normal) > 0.0)
    with np.errstate(invalid="ignore"):
        n = np.where(ok[:, None], _unit(np.where(ok[:, None], normal, 1.0)), np.array([[0.0, 1.0, 0.0]]))
    sign = np.where(_dot(direction, n) >= 0.0, 1.0, -1.0)
    return point + n * (sign * EPS * 4.0)[:, None] + direction * EPS * 0.5


def _margins(n):
    return {k: np.full(n, np.nan) for k in DECISIONS}


def begin(material, settings, inputs, states):
    """The function up to its loop on inputs [n, 12] {point, entry normal, wo, incident} and random states [n].  Returns a dict: outcome
    [n], direction / weight / pdf (outcome 1), direction / throughput / position (outcome 2), states afterwards, draws taken, margins."""
    m = material if isinstance(material, Material) else Material(material)
    cl = Clamps(settings)
    x = np.asarray(inputs, np.float32).astype(np.float64).reshape(-1, 12)
    point, n, wo, inc = x[:, 0:3], x[:, 3:6], x[:, 6:9], x[:, 9:12]
    k = len(x)
    u, state3 = lr.rng_draw(states, 3)
    _, state1 = lr.rng_draw(states, 1)
    mg = _margins(k)
    outcome = np.full(k, FALLBACK)
    direction, weight, pdf, position = np.zeros((k, 3)), np.zeros((k, 3)), np.zeros(k), np.zeros((k, 3))
    coat = (m.p_coat > 0.0) & (u[:, 0] < m.p_coat)
    mg["lobe"] = m.p_coat - u[:, 0] if m.p_coat > 0.0 else np.full(k, -1.0)

    with np.errstate(divide="ignore", invalid="ignore"):
        # ---- the coat lobe, 4105-4155: a VNDF half vector, the reflection about it, five rejections
        alpha_s = max(m.coat_roughness ** 2, f32(1e-4))
        t, b, fm = frame(n)
        won = _unit(wo)
        wl = np.stack([_dot(won, t), _dot(won, b), np.maximum(_dot(won, n), f32(1e-6))], axis=1)
        vh = _unit(np.stack([alpha_s * wl[:, 0], alpha_s * wl[:, 1], wl[:, 2]], axis=1))
        lensq = vh[:, 0] ** 2 + vh[:, 1] ** 2
        t1 = np.where((lensq > 0.0)[:, None], np.stack([-vh[:, 1], vh[:, 0], np.zeros(k)], axis=1) / np.sqrt(lensq)[:, None],
                      np.array([[1.0, 0.0, 0.0]]))
        t2 = np.cross(vh, t1)
        r, phi = np.sqrt(u[:, 1]), 2.0 * PI * u[:, 2]
        a1, a2 = r * np.cos(phi), r * np.sin(phi)
        s = 0.5 * (1.0 + vh[:, 2])
        a2 = (1.0 - s) * np.sqrt(np.maximum(0.0, 1.0 - a1 * a1)) + s * a2
        a3 = np.sqrt(np.maximum(0.0, 1.0 - a1 * a1 - a2 * a2))
        nh = a1[:, None] * t1 + a2[:, None] * t2 + a3[:, None] * vh
        ne = _unit(np.stack([alpha_s * nh[:, 0], alpha_s * nh[:, 1], np.maximum(nh[:, 2], 0.0)], axis=1))
        wh = _unit(ne[:, 0:1] * t + ne[:, 1:2] * b + ne[:, 2:3] * n)
        wi = _unit(-wo - 2.0 * _dot(-wo, wh)[:, None] * wh)
        cos_i, cos_o, wi_wh = _dot(n, wi), _dot(n, wo), _dot(wi, wh)
        alpha = m.coat_roughness ** 2
        spec = (m.f0 + (1.0 - m.f0) * np.clip(1.0 - wi_wh, 0.0, 1.0) ** 5) * \
            (_ggx_d(alpha, np.abs(_dot(n, wh))) * _ggx_g1(alpha, cos_o) * _ggx_g1(alpha, cos_i) / np.maximum(4.0 * cos_o * cos_i, f32(1e-6)))
        spec = cl.spec_tail(spec[:, None] * m.spec_tint[None, :], m.coat_roughness, m.f0)
        wh2 = _unit(wo + wi)   # ggx_pdf, 3724-3739
        cos_h, wo_wh = _dot(n, wh2), _dot(wo, wh2)
        pdf_raw = np.where((cos_o <= 0.0) | (cos_h <= 0.0) | (wo_wh <= 0.0), 0.0,
                           _ggx_d(alpha, cos_h) * _ggx_g1(alpha, cos_o) * cos_h / (4.0 * np.maximum(wo_wh, f32(1e-6))))
        spec_pdf = cl.spec_pdf(pdf_raw)
        w = np.maximum(spec * cos_i[:, None] / np.maximum(m.p_coat * spec_pdf, f32(1e-6))[:, None], 0.0)
        # (the margins of all five rejections in every coat row, reached or not: near_ties applies the shader's order)
        alive = coat.copy()
        for name, value in zip(COAT_ORDER, (_dot(wh, n), cos_i, cos_o, wi_wh, np.minimum(np.minimum(cos_o, cos_h), wo_wh))):
            mg[name] = np.where(coat, value, np.nan)
            alive = alive & (value > 0.0)
        mg["frame"] = np.where(coat, fm, np.nan)
        alive = alive & _finite3(wi) & (pdf_raw > 0.0) & _finite3(w)
        outcome[alive] = SAMPLE
        direction[alive], weight[alive], pdf[alive] = wi[alive], w[alive], spec_pdf[alive]

        # ---- into the medium, 4157-4193
        walk = ~coat
        cos_ti = _dot(-inc, n)
        mg["entry_cos"] = np.where(walk, cos_ti, np.nan)
        fr, cos_tt = _fresnel(cos_ti, 1.0, m.eta)
        enter, _ = _refract(inc, n, 1.0 / m.eta)
        ok = walk & (cos_ti > 0.0) & _finite3(enter) & (_dot(enter, enter) > 0.0)
        enter = _unit(enter)
        thr = (1.0 / max(1.0 - m.p_coat, f32(1e-3))) * np.maximum(1.0 - fr, 0.0) * (m.eta * m.eta) * (cos_tt / np.maximum(cos_ti, f32(1e-6)))
        thr = thr[:, None] * (m.spec_tint[None, :] if m.tinted else np.ones((1, 3)))
        pos = offset_surface_point(point, -n, enter)
    outcome[ok] = WALKING
    # cos of the transmitted angle is sqrt(1 - eta^2 (1 - cos^2)): the two subtractions from 1 round by 6e-8 each (the inner one scaled by
    # eta^2 = 1 / ior^2), which the root passes on over 2 cosT, relative to cosT.  Nothing at ior 1.5 (cosT >= 0.74); at ior 1, where
    # cosT = cosI, it is 6 % at the grazing end of the inputs.  The throughput is proportional to cosT.
    with np.errstate(divide="ignore", invalid="ignore"):
        entry_slack = 6e-8 * (1.0 + 1.0 / (m.eta * m.eta)) / (2.0 * cos_tt * cos_tt)
    entry_slack = np.where(ok & np.isfinite(entry_slack), entry_slack, 0.0)
    direction[ok], weight[ok], position[ok] = enter[ok], thr[ok], pos[ok]
    draws = np.where(coat, 3, 1)
    # At normal incidence the VNDF sampler's tangent T1 = (-Vh.y, Vh.x, 0) / |.| is the direction of what is left of wo beside the normal:
    # rounding noise of size 1e-7 in float32, so the sample's azimuth about the normal is anybody's (the lobe is symmetric about it: no
    # harm).  Where that remainder is below 1e-6 only what does not depend on the azimuth can be compared: cos to the normal, weight, pdf.
    azimuth_free = coat & (np.hypot(wl[:, 0], wl[:, 1]) < 1e-6)
    # The relative change of ggx_D per unit change of its cosine c, |dD/dc| / D = 4 c (1 - alpha^2) / (c^2 (alpha^2 - 1) + 1), summed over the
    # two cosines the lobe evaluates D at (dot(n, wh) for the value, dot(n, normalize(wo + wi)) for the pdf): what one rounding of c costs.
    a2 = alpha * alpha
    with np.errstate(divide="ignore", invalid="ignore"):
        c1 = np.abs(_dot(n, wh))
        d_cond = 4.0 * c1 * (1.0 - a2) / (c1 * c1 * (a2 - 1.0) + 1.0) + 4.0 * np.abs(cos_h) * (1.0 - a2) / (cos_h * cos_h * (a2 - 1.0) + 1.0)
    d_cond = np.where(coat & np.isfinite(d_cond), d_cond, 0.0)
    # ... and above it the azimuth still carries the rounding of wl.x and wl.y (6e-8 each) over their length, as an angle about the
    # normal; it moves the sample by that angle times its distance from the normal's axis
    with np.errstate(divide="ignore", invalid="ignore"):
        azimuth_slack = np.where(coat & ~azimuth_free, 1.2e-7 / np.hypot(wl[:, 0], wl[:, 1]) * np.linalg.norm(wi - cos_i[:, None] * n, axis=1), 0.0)
    azimuth_slack = np.where(np.isfinite(azimuth_slack), azimuth_slack, 0.0)
    # ... and, at grazing wo, the sampler's own cancellations: t3 = sqrt(1 - t1^2 - t2^2) carries the two roundings of its O(1) terms
    # (1.2e-7) over 2 t3, and Nh.z = t2 T2.z + t3 Vh.z is a difference of terms that each round by an ulp; stretching by 1 / alpha then
    # divides that error by the length of (alpha Nh.x, alpha Nh.y, Nh.z), and reflecting about the half vector doubles it
    with np.errstate(divide="ignore", invalid="ignore"):
        nhz_error = 1.2e-7 / (2.0 * np.maximum(a3, 1e-4)) * vh[:, 2] + 1.2e-7 * (np.abs(a2 * t2[:, 2]) + np.abs(a3 * vh[:, 2]))
        stretched = np.sqrt((alpha_s * nh[:, 0]) ** 2 + (alpha_s * nh[:, 1]) ** 2 + np.maximum(nh[:, 2], 0.0) ** 2)
        vndf_slack = 2.0 * nhz_error / stretched
    azimuth_slack = azimuth_slack + np.where(coat & np.isfinite(vndf_slack), vndf_slack, 0.0)
    # Where one float32 rounding of that cosine (6e-8) moves D by half its size or more, a float32 D is no number to compare: at coat
    # roughness 0.02 the cosine of a sample at the peak rounds to 1 or past it, the denominator to 0 or below, D to infinity, the pdf to
    # the clamp's floor and the weight to 4e6 (clampThroughput bounds what the path makes of it).  The shader's float arithmetic does the
    # same.  In such rows weight and pdf are compared between float32 sides only; outcome, draws and direction as everywhere.
    ill_conditioned = coat & (6e-8 * d_cond >= 0.5)
    return dict(entry_slack=entry_slack, ill_conditioned=ill_conditioned, azimuth_free=azimuth_free, azimuth_slack=azimuth_slack, normal=n, d_cond=d_cond, outcome=outcome,
                direction=direction, weight=weight, pdf=pdf, position=position, states=np.where(coat, state3, state1).astype(np.uint32),
                draws=draws, margins=mg)


def step(material, max_steps, rows, states):
    """One pass of the loop body (4196-4304) on rows [n, 20] {walk position, direction, throughput, step (uint32 bits), hitBoundary, hitT,
    hit point, outward normal} (pt.SSS_STEP_IN_FIELDS) and random states [n].  Returns a dict: outcome, the walk state as the pass leaves it
    (position, direction, throughput, step), the exit sample (exit_direction, exit_weight, exit_point; outcome 1), states afterwards,
    draws taken, event (0 miss, 1 scatter, 2 boundary), margins."""
    m = material if isinstance(material, Material) else Material(material)
    raw = np.ascontiguousarray(rows, np.float32).reshape(-1, 20)
    x = raw.astype(np.float64)
    pos, d, thr = x[:, 0:3].copy(), x[:, 3:6].copy(), x[:, 6:9].copy()
    stp = raw.view(np.uint32)[:, 9].astype(np.int64)
    hit, hit_t, hit_p, normal = x[:, 10] != 0.0, x[:, 11], x[:, 12:15], x[:, 15:18]
    k = len(x)
    limit = max(int(max_steps), 1)
    u, state3 = lr.rng_draw(states, 3)
    _, state1 = lr.rng_draw(states, 1)
    mg = _margins(k)
    outcome = np.full(k, FALLBACK)
    exit_dir, exit_w, exit_p = np.zeros((k, 3)), np.zeros((k, 3)), np.zeros((k, 3))
    xi = np.clip(u[:, 0], XI_LO, XI_HI)
    distance = -np.log(1.0 - xi) / m.sigma_t_scalar
    with np.errstate(invalid="ignore"):
        boundary = np.maximum(hit_t, EPS)
    boundary = np.where(np.isnan(hit_t), EPS, boundary)   # max(NaN, x) = x
    mg["free_flight"] = np.where(hit, boundary - distance, np.nan)
    scatter = hit & (distance < boundary)
    at_boundary = hit & ~scatter
    travelled = np.where(scatter, distance, boundary)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        t_new = thr * np.exp(-m.sigma_t[None, :] * travelled[:, None]) * np.where(scatter[:, None], m.albedo[None, :], 1.0)
        thr = np.where(hit[:, None], t_new, thr)
        mg["cutoff"] = np.where(hit, thr.max(axis=1) - CUTOFF, np.nan)
        alive = hit & ~(thr.max(axis=1) < CUTOFF)

        # ---- a scattering event inside, 4228-4244
        sc = scatter & alive
        ref = _unit(-d)
        mg["hg_isotropic"] = np.where(sc, f32(1e-3) - abs(m.g), np.nan)
        if abs(m.g) < f32(1e-3):
            cos_t = 1.0 - 2.0 * u[:, 1]
        else:
            sq = (1.0 - m.g * m.g) / (1.0 - m.g + 2.0 * m.g * u[:, 1])
            cos_t = np.clip((1.0 + m.g * m.g - sq * sq) / (2.0 * m.g), -1.0, 1.0)
        sin_t, phi = np.sqrt(np.maximum(0.0, 1.0 - cos_t * cos_t)), 2.0 * PI * u[:, 2]
        # (1 + g^2 - s^2) / (2 g) subtracts numbers of size 1 that round by 6e-8 each, three of them, and divides by 2 |g|: for a small g
        # beyond the isotropic switch that is an error of 1.8e-7 / (2 |g|) of the cosine, 8e-5 at g = 1.1e-3, and 1 / sin as much of the
        # direction
        hg_slack = np.zeros(k) if abs(m.g) < f32(1e-3) else 1.8e-7 / (2.0 * abs(m.g)) / np.maximum(sin_t, 1e-3)
        t, b, fm = frame(ref)
        mg["frame"] = np.where(sc, fm, np.nan)
        world = _unit((sin_t * np.cos(phi))[:, None] * t + (sin_t * np.sin(phi))[:, None] * b + cos_t[:, None] * ref)
        sc_ok = sc & _finite3(world) & (_dot(world, world) > 0.0) & (_dot(ref, ref) > 0.0)
        pos = np.where(sc[:, None], pos + d * distance[:, None], pos)
        new_d = np.where(sc_ok[:, None], world, d)

        # ---- the boundary, 4246-4303
        bd = at_boundary & alive
        n_ok = _finite3(normal) & (_dot(np.nan_to_num(normal), np.nan_to_num(normal)) > 0.0)
        nrm = _unit(np.where(n_ok[:, None], normal, 0.0))
        bd = bd & n_ok
        cos_e = _dot(-d, nrm)
        mg["exit_cos"] = np.where(bd, cos_e, np.nan)
        fr, cos_tt = _fresnel(cos_e, m.eta, 1.0)
        refr, kk = _refract(d, nrm, m.eta)
        mg["tir"] = np.where(bd & (cos_e > 0.0), kk, np.nan)
        leaves = bd & (cos_e > 0.0) & _finite3(refr) & (_dot(refr, refr) > 0.0)
        back = bd & ~leaves
        pos = np.where(back[:, None], hit_p, pos)
        new_d = np.where(back[:, None], _unit(d - 2.0 * _dot(d, nrm)[:, None] * nrm), new_d)
        w = thr * (np.maximum(1.0 - fr, 0.0) * (1.0 / (m.eta * m.eta)) * (cos_tt / np.maximum(cos_e, f32(1e-6))))[:, None]
        if m.tinted:
            w = w * m.spec_tint[None, :]
        w = np.maximum(w, 0.0)
        out = leaves & _finite3(w)
    went_on = sc_ok | back
    stp = np.where(went_on, stp + 1, stp)
    outcome[went_on & (stp < limit)] = WALKING
    outcome[out] = SAMPLE
    exit_dir[out], exit_w[out], exit_p[out] = _unit(refr)[out], w[out], hit_p[out]
    took3 = sc   # the two Henyey-Greenstein draws follow the cut-off test
    return dict(hg_slack=np.where(sc, hg_slack, 0.0), outcome=outcome, position=pos, direction=new_d, throughput=thr, step=(stp & 0xFFFFFFFF).astype(np.uint32), exit_direction=exit_dir,
                exit_weight=exit_w, exit_point=exit_p, states=np.where(took3, state3, state1).astype(np.uint32), draws=np.where(took3, 3, 1),
                event=np.where(~hit, 0, np.where(scatter, 1, 2)), margins=mg, sigma_t_scalar=m.sigma_t_scalar, boundary=boundary)


def near_ties(result):
    """[n] bool: rows one of whose decisions lies inside its band (BANDS), so that a float32 evaluation may take the other branch."""
    mg = result["margins"]
    near = np.zeros(len(result["outcome"]), bool)
    # the coat's rejections in the shader's order: one counts only in the rows that pass those before it; and none of them in a row
    # whose wo is clearly below the surface, which falls back whatever the others decide (with the same three draws)
    with np.errstate(invalid="ignore"):
        reached = np.isfinite(mg["coat_wh"]) & ~(mg["coat_cos_o"] < -BANDS["coat_cos_o"][0])
        for name in COAT_ORDER:
            v = mg[name]
            near |= reached & (v != 0.0) & (np.abs(v) < BANDS[name][0])
            reached = reached & (v > 0.0)
    for name, (absolute, relative) in BANDS.items():
        if name in COAT_ORDER:
            continue
        v = mg[name]
        band = np.full(len(v), absolute)
        if name == "free_flight":
            if "boundary" not in result:   # (begin takes no such decision)
                continue
            band = band + 1.2e-7 / result["sigma_t_scalar"] + relative * result["boundary"]
        elif name == "cutoff":
            band = band + relative * CUTOFF
        with np.errstate(invalid="ignore"):
            near |= np.isfinite(v) & (v != 0.0) & (np.abs(v) < band)
    return near


def branches(result):
    """name -> [n] bool of the branches a batch took (test_sss_walk_host.py shows every one of them occupied)."""
    mg = result["margins"]
    with np.errstate(invalid="ignore"):
        out = {"lobe_coat": mg["lobe"] > 0.0, "lobe_medium": mg["lobe"] <= 0.0}
        for name in ("coat_wh", "coat_cos_i", "coat_cos_o", "coat_wi_wh", "coat_pdf", "entry_cos"):
            out[name + "_rejects"] = mg[name] <= 0.0
        out.update({"scatter": mg["free_flight"] > 0.0, "boundary": mg["free_flight"] <= 0.0, "cut_off": mg["cutoff"] < 0.0,
                    "exits_or_tir": mg["exit_cos"] > 0.0, "reflects_back": mg["exit_cos"] <= 0.0, "tir": mg["tir"] < 0.0,
                    "hg_isotropic": mg["hg_isotropic"] > 0.0, "hg_anisotropic": mg["hg_isotropic"] <= 0.0})
    return out


# ---------------------------------------------------------------- analytic closest hits (float64)
class AnalyticScene:
    """Spheres, axis-aligned rectangles and triangles with the closest hit beyond kRayOriginEpsilon in float64: (hit, t, point, the
    geometric normal as stored: outward for a sphere, +axis for a rectangle, (v1 - v0) x (v2 - v0) for a triangle)."""

    def __init__(self, spheres=(), triangles=(), rects=()):
        self.spheres = [(np.asarray(c, np.float64), float(r)) for c, r in spheres]
        self.triangles = [np.asarray(t, np.float64).reshape(3, 3) for t in triangles]
        self.rects = [(int(axis), float(at), np.asarray(lo, np.float64), np.asarray(hi, np.float64)) for axis, at, lo, hi in rects]

    def closest(self, origin, direction, tmin=EPS):
        o, d = np.asarray(origin, np.float64).reshape(-1, 3), np.asarray(direction, np.float64).reshape(-1, 3)
        k = len(o)
        best_t, best_n = np.full(k, np.inf), np.zeros((k, 3))
        with np.errstate(divide="ignore", invalid="ignore"):
            for c, r in self.spheres:
                oc = o - c
                a, hb, cc = _dot(d, d), _dot(oc, d), _dot(oc, oc) - r * r
                disc = hb * hb - a * cc
                sq = np.sqrt(np.maximum(disc, 0.0))
                for root in ((-hb - sq) / a, (-hb + sq) / a):
                    ok = (disc >= 0.0) & (root > tmin) & (root < best_t)
                    best_t = np.where(ok, root, best_t)
                    best_n = np.where(ok[:, None], (o + root[:, None] * d - c) / r, best_n)
            for tri in self.triangles:
                e1, e2 = tri[1] - tri[0], tri[2] - tri[0]
                p = np.cross(d, e2[None, :])
                det = p @ e1
                s = o - tri[0]
                uu = _dot(s, p) / det
                q = np.cross(s, e1[None, :])
                vv = _dot(d, q) / det
                tt = (q @ e2) / det
                ok = (det != 0.0) & (uu >= 0.0) & (vv >= 0.0) & (uu + vv <= 1.0) & (tt > tmin) & (tt < best_t)
                ng = np.cross(e1, e2)
                best_t = np.where(ok, tt, best_t)
                best_n = np.where(ok[:, None], (ng / np.linalg.norm(ng))[None, :], best_n)
            for axis, at, lo, hi in self.rects:
                tt = (at - o[:, axis]) / d[:, axis]
                p = o + tt[:, None] * d
                others = [a for a in range(3) if a != axis]
                ok = (tt > tmin) & (tt < best_t) & (p[:, others] >= lo[None, :]).all(axis=1) & (p[:, others] <= hi[None, :]).all(axis=1)
                best_t = np.where(ok, tt, best_t)
                best_n = np.where(ok[:, None], np.eye(3)[axis][None, :], best_n)
        hit = np.isfinite(best_t)
        t = np.where(hit, best_t, 0.0)
        return hit, t, o + t[:, None] * d, best_n


def cube_triangles(center, half, inward=False):
    """The 12 triangles of an axis-aligned cube, wound counter-clockwise seen from outside (from inside when `inward`): [12, 3, 3]."""
    c, h = np.asarray(center, np.float64), float(half)
    tris = []
    for axis in range(3):
        a, b = (axis + 1) % 3, (axis + 2) % 3
        for sign in (1.0, -1.0):
            def corner(sa, sb):
                p = c.copy()
                p[axis] += sign * h
                p[a] += sa * h
                p[b] += sb * h
                return p
            quad = [corner(-1, -1), corner(1, -1), corner(1, 1), corner(-1, 1)]
            if sign < 0:
                quad = quad[::-1]
            if inward:
                quad = quad[::-1]
            tris += [[quad[0], quad[1], quad[2]], [quad[0], quad[2], quad[3]]]
    return np.array(tris)


def cube_obj(center, half, inward=False):
    """The same cube as the text of an OBJ file.  Every corner carries the normal of a rounded cube (from the centre through the corner),
    so that the shading normal of a hit is not its geometric normal: what shadeSlot parks for the sample of an abandoned walk (the
    shading normal) can then be told from what sssWalkBegin entered with (the geometric one)."""
    tris = cube_triangles(center, half, inward)
    c = np.asarray(center, np.float64)
    lines = ["v %.9g %.9g %.9g" % tuple(v) for t in tris for v in t]
    lines += ["vn %.9g %.9g %.9g" % tuple((v - c) / np.linalg.norm(v - c)) for t in tris for v in t]
    lines += ["f %d//%d %d//%d %d//%d" % (3 * i + 1, 3 * i + 1, 3 * i + 2, 3 * i + 2, 3 * i + 3, 3 * i + 3) for i in range(len(tris))]
    return "\n".join(lines) + "\n"
