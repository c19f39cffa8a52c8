"""Inputs of the BSDF domain tests (test_bsdf_domain_host.py on the CPU, test_gpu_bsdf_domain.py on the device): every class of normal,
outgoing and incoming direction, material and mode that evalBsdf / sampleBsdf (csrc/kernels/bsdf.h) can meet, seeded, in one place;
and ORACLE_MEASURED, the oracle's own figures over that domain, from which the device tests take their bounds.

A sample class is (normal class, wo class): 3 x 3, plus 'horizon' (cos(wo) == 0 exactly, which only n = z can give).  An evaluation class
is (wo class, wi class); its rows take their normals from the three normal classes in turn (row i: NORMALS[i % 3]).  N rows per class.
"""
import importlib
import os
import tempfile

import numpy as np

pt = importlib.import_module("metal-pathtracer-arm64_amd")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

N = 4096      # rows per class
CAP = 0.002   # the cap of test_gpu_lights.py: share of a batch whose outcome may hang on a last-ulp difference
EVAL_TOL = dict(rtol=2e-4, atol=1e-6)     # test_gpu_parity.test_eval_bsdf_matches_oracle
SAMPLE_TOL = dict(rtol=5e-4, atol=2e-5)   # test_gpu_parity.test_sample_bsdf_matches_oracle
LOOSE_TOL = dict(rtol=5e-2, atol=1e-3)    # ... and its bound for car paint's narrow lobes

ALL_METAL = pt.PTR_METAL_SPECULAR | pt.PTR_METAL_SSS | pt.PTR_METAL_PBR
MODES = {"embree": 0, "specular": pt.PTR_METAL_SPECULAR, "sss": pt.PTR_METAL_SSS, "pbr": pt.PTR_METAL_PBR, "metal": ALL_METAL,
         "metal_clamps": ALL_METAL | pt.PTR_METAL_CLAMPS}

NORMALS = ("random", "axes", "band")
WO = ("regular", "grazing", "below")   # cos in [0.05, 1], in [1e-4, 0.05], in [-1, -1e-4]; 'horizon' (cos == 0) stands apart
WI = ("upper", "lower", "mirror", "same", "opposite", "lobe")
SAMPLE_CLASSES = tuple("%s/%s" % (a, b) for a in NORMALS for b in WO) + ("z/horizon",)
EVAL_CLASSES = tuple("%s/%s" % (a, b) for a in WO + ("horizon",) for b in WI)


# ---------------------------------------------------------------- directions
def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _basis(n):
    """Two float64 unit vectors orthogonal to n [k, 3] and to each other (not makeFrame's: any basis serves to place a cosine)."""
    a = np.where((np.abs(n[:, 0:1]) < 0.5), np.array([[1.0, 0.0, 0.0]]), np.array([[0.0, 1.0, 0.0]]))
    t = _unit(np.cross(a, n))
    return t, np.cross(n, t)


def normals(kind, k, rng):
    """[k, 3] float32, unit to one float32 ulp (rounded from a float64 unit vector)."""
    if kind == "random":
        n = _unit(rng.normal(size=(k, 3)))
    elif kind == "axes":
        n = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)[np.arange(k) % 6]
    elif kind == "band":   # |n.z| around makeFrame's 0.999: both of its branches, both signs
        z = rng.uniform(0.9985, 0.9995, k) * np.where(rng.random(k) < 0.5, -1.0, 1.0)
        phi = rng.uniform(0, 2 * np.pi, k)
        r = np.sqrt(1 - z * z)
        n = np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)
    elif kind == "z":
        n = np.tile(np.array([0.0, 0.0, 1.0]), (k, 1))
    else:
        raise ValueError(kind)
    return n.astype(np.float32)


def _at_cosine(n, c, rng):
    n = n.astype(np.float64)
    t, b = _basis(n)
    phi = rng.uniform(0, 2 * np.pi, len(n))[:, None]
    s = np.sqrt(np.maximum(1 - c * c, 0.0))[:, None]
    return (c[:, None] * n + s * (np.cos(phi) * t + np.sin(phi) * b)).astype(np.float32)


def _cosines(kind, k, rng):
    if kind == "regular":
        return rng.uniform(0.05, 1.0, k)
    if kind == "grazing":
        return np.exp(rng.uniform(np.log(1e-4), np.log(0.05), k))
    if kind == "below":
        return -np.exp(rng.uniform(np.log(1e-4), 0.0, k))
    raise ValueError(kind)


def outgoing(kind, n, rng):
    """wo [k, 3] float32 at the class's cosine to n.  'horizon': n must be z; wo.z is exactly 0, so the cosine is."""
    if kind == "horizon":
        assert (n == np.array([0, 0, 1], np.float32)).all()
        phi = rng.uniform(0, 2 * np.pi, len(n))
        return np.stack([np.cos(phi), np.sin(phi), np.zeros(len(n))], axis=1).astype(np.float32)
    return _at_cosine(n, _cosines(kind, len(n), rng), rng)


def incoming(kind, n, wo, rng, lobe=None):
    """wi [k, 3] float32.  'mirror' is wo mirrored about n (rounded once from float64: the half vector is n to an ulp); 'same' and
    'opposite' are wo and -wo bit for bit; 'lobe': the directions `lobe` [k, 3] the oracle's sampler returned, and the mirror direction
    in the rows where it returned none (all zeros)."""
    k = len(n)
    if kind == "upper":
        return _at_cosine(n, np.where(rng.random(k) < 0.25, _cosines("grazing", k, rng), rng.uniform(0.05, 1.0, k)), rng)
    if kind == "lower":
        return _at_cosine(n, _cosines("below", k, rng), rng)
    n64, wo64 = n.astype(np.float64), wo.astype(np.float64)
    mirror = (2.0 * np.einsum("ij,ij->i", n64, wo64)[:, None] * n64 - wo64).astype(np.float32)
    if kind == "mirror":
        return mirror
    if kind == "same":
        return wo.copy()
    if kind == "opposite":
        return -wo
    if kind == "lobe":
        none = ~np.any(lobe != 0, axis=1)
        return np.where(none[:, None], mirror, lobe).astype(np.float32)
    raise ValueError(kind)


def _seed(name):
    return [ord(c) for c in name]


def sample_inputs(cls, k=N):
    """(inputs [k, 9] {position, normal, wo}, front [k] of 0 and 1, states [k]) of one sample class."""
    nk, wk = cls.split("/")
    rng = np.random.default_rng(_seed("sample " + cls))
    n = normals(nk, k, rng)
    wo = outgoing(wk, n, rng)
    pos = rng.uniform(-2, 2, size=(k, 3)).astype(np.float32)
    front = (rng.random(k) < 0.5).astype(np.uint32)
    states = rng.integers(1, 2**32 - 1, size=k, dtype=np.uint64).astype(np.uint32)
    return np.concatenate([pos, n, wo], axis=1), front, states


def eval_geometry(cls, k=N):
    """(position, normal, wo, rng, normal class per row) of one evaluation class; the wi follows from incoming(), which for 'lobe' needs
    the material."""
    wk, _ = cls.split("/")
    rng = np.random.default_rng(_seed("eval " + cls))
    if wk == "horizon":
        n, kinds = normals("z", k, rng), np.array(["z"] * k)
    else:
        parts = {a: normals(a, k, rng) for a in NORMALS}
        kinds = np.array(NORMALS)[np.arange(k) % 3]
        n = np.where((np.arange(k) % 3 == 0)[:, None], parts["random"], np.where((np.arange(k) % 3 == 1)[:, None], parts["axes"], parts["band"]))
    wo = outgoing(wk, n, rng)
    pos = rng.uniform(-2, 2, size=(k, 3)).astype(np.float32)
    return pos, n, wo, rng, kinds


def eval_inputs(cls, lobe_sampler, k=N):
    """inputs [k, 12] {position, normal, wo, wi} of one evaluation class; lobe_sampler(inputs9, front, states) -> [k, 8] is asked for the
    'lobe' class only (the oracle's sampler with the material and mode under test)."""
    pos, n, wo, rng, kinds = eval_geometry(cls, k)
    wik = cls.split("/")[1]
    lobe = None
    if wik == "lobe":
        states = rng.integers(1, 2**32 - 1, size=k, dtype=np.uint64).astype(np.uint32)
        lobe = lobe_sampler(np.concatenate([pos, n, wo], axis=1), np.ones(k, np.uint32), states)[:, 0:3]
    wi = incoming(wik, n, wo, rng, lobe)
    return np.concatenate([pos, n, wo, wi], axis=1), kinds


def sample_batch():
    """All sample classes in one batch: (inputs [10 N, 9], front, states, {class: slice}), made once."""
    if "sample_batch" not in _cache:
        parts = [sample_inputs(c) for c in SAMPLE_CLASSES]
        where = {c: slice(i * N, (i + 1) * N) for i, c in enumerate(SAMPLE_CLASSES)}
        _cache["sample_batch"] = tuple(np.concatenate([p[j] for p in parts]) for j in range(3)) + (where,)
    return _cache["sample_batch"]


def eval_batch(lobe_sampler):
    """All evaluation classes in one batch: (inputs [24 N, 12], {class: slice}); the rows of the 'lobe' classes from lobe_sampler."""
    if "eval_batch" not in _cache:
        _cache["eval_batch"] = {c: eval_inputs(c, None)[0] for c in EVAL_CLASSES if not c.endswith("lobe")}
    parts = [_cache["eval_batch"][c] if c in _cache["eval_batch"] else eval_inputs(c, lobe_sampler)[0] for c in EVAL_CLASSES]
    return np.concatenate(parts), {c: slice(i * N, (i + 1) * N) for i, c in enumerate(EVAL_CLASSES)}


def one_ulp(v, up):
    """Every component of v moved by one float32 ulp: up where `up` [like v] is true, down elsewhere."""
    return np.nextafter(v, np.where(up, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)).astype(np.float32)


def rotations(k, rng):
    """k random rotation matrices [k, 3, 3] (float64, proper)."""
    q, r = np.linalg.qr(rng.normal(size=(k, 3, 3)))
    q = q * np.sign(np.einsum("kii->ki", r))[:, None, :]
    q[:, :, 0] *= np.sign(np.linalg.det(q))[:, None]
    return q


# ---------------------------------------------------------------- materials
_SSS_SCENE = ("camera target=0,0,0 distance=5\n"
              "material type=sss albedo=0.8,0.5,0.3 mfp=0.3 name=skin\n"
              "material type=sss albedo=0.3,0.6,0.8 mfp=0.15 g=0.3 sigma_a=0.4,0.2,0.1 sigma_s=3.0,4.0,5.0 coat=on name=jade\n"
              "sphere center=0,0,0 radius=1 material=0\n")

_cache = {}


def _copy(m):
    return pt.PtrMaterial.from_buffer_copy(bytes(m))


def host():
    """tests/golden/materials.scene, loaded once."""
    if "host" not in _cache:
        _cache["host"] = pt.HostScene.load(os.path.join(GOLDEN, "materials.scene"))
    return _cache["host"]


def materials():
    """[(name, group, material)]: the materials of materials.scene, then variants made as test_gpu_parity._all_materials makes its own,
    so that every threshold inside the functions has a material on either side of it.  The group names the entry of ORACLE_MEASURED."""
    if "materials" in _cache:
        return _cache["materials"]
    d = host().desc
    names = [l.split("name=")[1].strip() for l in open(os.path.join(GOLDEN, "materials.scene")) if l.startswith("material ")]
    groups = {"lambert": "lambert", "rough_metal": "metal_wide", "mirror": "metal_delta", "gold_like": "metal_wide", "glass": "dielectric",
              "plastic": "plastic_narrow", "thick_plastic": "plastic_wide", "skin": "sss", "carpaint": "carpaint",
              "carpaint_dielectric_base": "carpaint", "floor": "lambert"}
    out = [(nm, groups[nm], _copy(d.materials[i])) for i, nm in enumerate(names)]
    # metal: roughness on either side of the delta threshold 1e-3, a narrow and two wide lobes; Schlick and conductor Fresnel
    for rough in (0.0, 1e-3, 1.1e-3, 0.02, 0.2, 1.0):
        for src, tag in ((1, "schlick"), (3, "conductor")):
            m = _copy(d.materials[src])
            m.baseColorRoughness[3] = rough
            out.append(("metal_%s_%g" % (tag, rough), "metal_delta" if rough <= 1e-3 else ("metal_narrow" if rough < 0.1 else "metal_wide"), m))
    for rough in (0.04, 0.3, 1.0):
        m = _copy(d.materials[5])
        m.coatParams[0] = rough
        out.append(("plastic_coat_%g" % rough, "plastic_narrow" if rough < 0.2 else "plastic_wide", m))
    # type 7, the factor-only model (and, under PTR_METAL_PBR, the three-lobe model without transmission)
    for metallic in (0.0, 0.5, 1.0):
        for rough in (0.0, 1e-3, 0.05, 0.6, 1.0):
            m = _copy(d.materials[0])
            m.typeEta[0], m.typeEta[1] = 7.0, 1.5
            m.baseColorRoughness[3] = rough
            m.pbrParams[0] = metallic
            out.append(("pbr_m%g_r%g" % (metallic, rough), "pbr_narrow" if rough < 0.1 else "pbr_wide", m))
    # ... with transmission (read under PTR_METAL_PBR only: MODES_OF), ior 1 (roughTransmission's denomSq <= 1e-8) and 1.45, a thickness
    # and a non-zero sigmaA (transmissionTint)
    for transmission in (0.0, 0.7, 1.0):
        for ior in (1.0, 1.45):
            for rough in (0.0, 0.35):
                m = _copy(d.materials[0])
                m.typeEta[0], m.typeEta[1], m.typeEta[3] = 7.0, ior, 0.5
                m.baseColorRoughness[3] = rough
                m.pbrParams[0], m.pbrExtras[2] = 0.1, transmission
                m.dielectricSigmaA[0], m.dielectricSigmaA[1], m.dielectricSigmaA[2] = 0.2, 0.5, 1.0
                out.append(("pbr_t%g_ior%g_r%g" % (transmission, ior, rough), "pbr_transmissive", m))
    # both subsurface materials of test_gpu_parity.test_metal_subsurface_semantics
    with tempfile.TemporaryDirectory() as tmp:
        p = os.path.join(tmp, "sss.scene")
        with open(p, "w") as f:
            f.write(_SSS_SCENE)
        h = pt.HostScene.load(p)
        out += [("sss_skin", "sss", _copy(h.desc.materials[0])), ("sss_jade", "sss", _copy(h.desc.materials[1]))]
    assert len({nm for nm, _, _ in out}) == len(out)
    _cache["materials"] = out
    return out


def mtype(m):
    return int(m.typeEta[0])


def is_delta(m):
    """materialIsDelta (bsdf.h; E:849-861)."""
    return mtype(m) == 2 or (mtype(m) == 1 and np.float32(np.clip(np.float32(m.baseColorRoughness[3]), 0, 1)) <= np.float32(1e-3))


def transmits(m, mode):
    """The material has the Metal PBR transmission lobe in this mode: evaluation is non-zero across the surface."""
    return mtype(m) == 7 and bool(mode & pt.PTR_METAL_PBR) and m.pbrExtras[2] > 0 and m.pbrParams[0] < 1


def modes_of(group):
    """The modes a material group is run in.  'embree', 'metal' and 'metal_clamps' always; of the single bits only the one the group's
    type reads (bsdf.h: metalSpecular is read by type 1 alone, metalSss by type 5, metalPbr by type 7) - under another single bit a
    material runs the instructions of 'embree'.  The transmissive type-7 variants differ from the others only under PTR_METAL_PBR."""
    if group == "pbr_transmissive":
        return ("pbr", "metal", "metal_clamps")
    extra = {"metal": "specular", "sss": "sss", "pbr": "pbr"}.get(group.split("_")[0])
    return ("embree",) + ((extra,) if extra else ()) + ("metal", "metal_clamps")


def settings(mode):
    s = host().settings_for(width=16, height=16)
    s.metalSemantics = MODES[mode]
    if MODES[mode] & pt.PTR_METAL_SSS:
        s.sssMode = 1   # `renderer sss=separable`: sampleSeparableSss runs
    return s


GROUPS = ("lambert", "metal_delta", "metal_narrow", "metal_wide", "dielectric", "plastic_narrow", "plastic_wide", "sss", "carpaint",
          "pbr_narrow", "pbr_wide", "pbr_transmissive")

# The (group, mode) pairs whose sampler reports the pdf evaluation reports at the sampled direction, and weight = value cos / pdf
# (test_bsdf_domain_host.py says why the others do not), and the classes it is asked in: cos(wo) > 0.
IDENTITY = {("lambert", "embree"), ("sss", "embree"), ("metal_narrow", "embree"), ("metal_wide", "embree"), ("plastic_narrow", "embree"),
            ("plastic_wide", "embree"), ("lambert", "metal"), ("metal_narrow", "metal"), ("metal_wide", "metal"), ("plastic_narrow", "metal"),
            ("plastic_wide", "metal")}
IDENTITY_CLASSES = tuple(c for c in SAMPLE_CLASSES if c.split("/")[1] in ("regular", "grazing"))


def identity_errors(sample, ev):
    """Per row: (|pdf - evaluated pdf|, largest |weight - value cos / pdf| over the channels), each relative to the evaluated figure
    plus 1e-2 (the floor of test_gpu_parity._rel); cos is recovered as the caller gives it inside ev's weight.  sample [k, 8] are valid
    non-delta rows, ev [k, 4] = {value cos / pdf rgb, pdf} at the sampled direction."""
    s, e = sample.astype(np.float64), ev.astype(np.float64)
    pdf = np.abs(s[:, 6] - e[:, 3]) / (np.abs(e[:, 3]) + 1e-2)
    weight = (np.abs(s[:, 3:6] - e[:, 0:3]) / (np.abs(e[:, 0:3]) + 1e-2)).max(axis=1)
    return pdf, weight


def expected_weight(ev, normal, direction):
    """value cos / pdf of an evaluation [k, 5] at `direction`, with its pdf: [k, 4]; zeros where the pdf is."""
    cos = np.einsum("ij,ij->i", normal.astype(np.float64), direction.astype(np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(ev[:, 3:4] > 0, ev[:, 0:3].astype(np.float64) * cos[:, None] / ev[:, 3:4].astype(np.float64), 0.0)
    return np.concatenate([w, ev[:, 3:4].astype(np.float64)], axis=1)


def moved_share(a, b, tol, valid_column=None):
    """Share of rows of a that b does not match within tol (a row valid on one side only counts as moved)."""
    ok = np.isclose(a, b, **tol).all(axis=1)
    if valid_column is not None:
        ok &= (a[:, valid_column] > 0) == (b[:, valid_column] > 0)
    return float((~ok).mean())


# ---------------------------------------------------------------- the oracle's own figures
# Produced by `python tests/test_bsdf_domain_host.py --write` (CPU only, the oracle alone), which rewrites the lines between the two
# markers; test_bsdf_domain_host.py measures them again and holds them against what stands here.
#   ORACLE_MEASURED[group][class]: a sample class -> (share of rows a one-ulp move of wo carries past SAMPLE_TOL, worst pdf and worst
#     weight difference of sample against evaluate (identity_errors; None where the identity is not asked)); an evaluation class ->
#     (share of rows a one-ulp move of wo carries past EVAL_TOL, share of rows a common rotation of the inputs carries past it, worst
#     relative difference under that rotation); the worst over the group's materials and modes, rounded up to two digits.
#   ILL_CONDITIONED[material]: the classes in which that share is above CAP / 2 in one of the material's modes.
# BEGIN MEASURED
ORACLE_MEASURED = {
    'lambert': {
        'random/regular': (0.0, 1.7e-06, 6.5e-06),
        'random/grazing': (0.0, 7.1e-07, 2.3e-06),
        'random/below': (0.0, None, None),
        'axes/regular': (0.0, 2.2e-07, 3e-07),
        'axes/grazing': (0.0, 2.3e-07, 2.9e-07),
        'axes/below': (0.0, None, None),
        'band/regular': (0.0, 3.2e-07, 5.1e-07),
        'band/grazing': (0.0, 2.8e-07, 4.3e-07),
        'band/below': (0.0, None, None),
        'z/horizon': (0.0, None, None),
        'regular/upper': (0.0, 0.0, 2.6e-06),
        'regular/lower': (0.0, 0.0, 0.0),
        'regular/mirror': (0.0, 0.0, 5.9e-07),
        'regular/same': (0.0, 0.0, 7.9e-07),
        'regular/opposite': (0.0, 0.0, 0.0),
        'regular/lobe': (0.0, 0.0, 5.8e-07),
        'grazing/upper': (0.0, 0.0, 3.8e-06),
        'grazing/lower': (0.0, 0.0, 0.0),
        'grazing/mirror': (0.0, 0.0, 2.9e-06),
        'grazing/same': (0.0, 0.0, 2.9e-06),
        'grazing/opposite': (0.0, 0.0, 0.0),
        'grazing/lobe': (0.0, 0.0, 7.3e-07),
        'below/upper': (0.0, 0.0, 0.0),
        'below/lower': (0.0, 0.0, 0.0),
        'below/mirror': (0.0, 0.0, 0.0),
        'below/same': (0.0, 0.0, 0.0),
        'below/opposite': (0.0, 0.0, 0.0),
        'below/lobe': (0.0, 0.0, 0.0),
        'horizon/upper': (0.48, 0.32, 32.0),
        'horizon/lower': (0.0, 0.0, 0.0),
        'horizon/mirror': (0.0, 0.0, 0.0),
        'horizon/same': (0.0, 0.32, 26.0),
        'horizon/opposite': (0.0, 0.0, 0.0),
        'horizon/lobe': (0.5, 0.31, 32.0),
    },
    'metal_delta': {
        'random/regular': (0.0, None, None),
        'random/grazing': (0.0, None, None),
        'random/below': (0.0, None, None),
        'axes/regular': (0.0, None, None),
        'axes/grazing': (0.0, None, None),
        'axes/below': (0.0, None, None),
        'band/regular': (0.0, None, None),
        'band/grazing': (0.0, None, None),
        'band/below': (0.0, None, None),
        'z/horizon': (0.51, None, None),
        'regular/upper': (0.0, 0.0, 0.0),
        'regular/lower': (0.0, 0.0, 0.0),
        'regular/mirror': (0.0, 0.0, 0.0),
        'regular/same': (0.0, 0.0, 0.0),
        'regular/opposite': (0.0, 0.0, 0.0),
        'regular/lobe': (0.0, 0.0, 0.0),
        'grazing/upper': (0.0, 0.0, 0.0),
        'grazing/lower': (0.0, 0.0, 0.0),
        'grazing/mirror': (0.0, 0.0, 0.0),
        'grazing/same': (0.0, 0.0, 0.0),
        'grazing/opposite': (0.0, 0.0, 0.0),
        'grazing/lobe': (0.0, 0.0, 0.0),
        'below/upper': (0.0, 0.0, 0.0),
        'below/lower': (0.0, 0.0, 0.0),
        'below/mirror': (0.0, 0.0, 0.0),
        'below/same': (0.0, 0.0, 0.0),
        'below/opposite': (0.0, 0.0, 0.0),
        'below/lobe': (0.0, 0.0, 0.0),
        'horizon/upper': (0.0, 0.0, 0.0),
        'horizon/lower': (0.0, 0.0, 0.0),
        'horizon/mirror': (0.0, 0.0, 0.0),
        'horizon/same': (0.0, 0.0, 0.0),
        'horizon/opposite': (0.0, 0.0, 0.0),
        'horizon/lobe': (0.0, 0.0, 0.0),
    },
    'metal_narrow': {
        'random/regular': (0.51, 770000000.0, 42000000000.0),
        'random/grazing': (0.81, 400000000000.0, 2200000000.0),
        'random/below': (0.0, None, None),
        'axes/regular': (0.41, 2.3, 41000000000.0),
        'axes/grazing': (0.67, 400000000000.0, 280000000.0),
        'axes/below': (0.0, None, None),
        'band/regular': (0.47, 490000000.0, 42000000000.0),
        'band/grazing': (0.74, 520000000000.0, 2200000000.0),
        'band/below': (0.0, None, None),
        'z/horizon': (0.51, None, None),
        'regular/upper': (0.0, 0.00025, 0.0015),
        'regular/lower': (0.0, 0.0, 0.0),
        'regular/mirror': (0.28, 0.46, 13000000000.0),
        'regular/same': (0.00049, 0.00025, 0.00019),
        'regular/opposite': (0.0, 0.0, 0.0),
        'regular/lobe': (0.38, 0.6, 2900000000.0),
        'grazing/upper': (0.00098, 0.00049, 0.00024),
        'grazing/lower': (0.0, 0.0, 0.0),
        'grazing/mirror': (0.84, 0.81, 120000000000000.0),
        'grazing/same': (0.0062, 0.019, 0.00044),
        'grazing/opposite': (0.0, 0.0, 0.0),
        'grazing/lobe': (0.87, 0.87, 120000000000000.0),
        'below/upper': (0.0, 0.0, 0.0),
        'below/lower': (0.0, 0.0, 0.0),
        'below/mirror': (0.0, 0.0, 0.0),
        'below/same': (0.0, 0.0, 0.0),
        'below/opposite': (0.0, 0.0, 0.0),
        'below/lobe': (0.0, 0.0, 0.0),
        'horizon/upper': (0.015, 0.3, 0.55),
        'horizon/lower': (0.0, 0.0, 0.0),
        'horizon/mirror': (0.0, 0.0, 0.0),
        'horizon/same': (0.0, 0.0, 1e-06),
        'horizon/opposite': (0.0, 0.0, 0.0),
        'horizon/lobe': (0.0, 0.0, 0.0),
    },
    'metal_wide': {
        'random/regular': (0.0025, 0.00074, 0.00068),
        'random/grazing': (0.039, 0.11, 0.00097),
        'random/below': (0.0, None, None),
        'axes/regular': (0.0, 0.0003, 0.00025),
        'axes/grazing': (0.021, 0.34, 0.00026),
        'axes/below': (0.0, None, None),
        'band/regular': (0.0, 0.00058, 0.00041),
        'band/grazing': (0.021, 0.38, 0.0006),
        'band/below': (0.0, None, None),
        'z/horizon': (0.26, None, None),
        'regular/upper': (0.0, 0.0, 0.00018),
        'regular/lower': (0.0, 0.0, 0.0),
        'regular/mirror': (0.1, 0.2, 0.0006),
        'regular/same': (0.00025, 0.0, 0.00014),
        'regular/opposite': (0.0, 0.0, 0.0),
        'regular/lobe': (0.035, 0.068, 0.0006),
        'grazing/upper': (0.004, 0.004, 0.00066),
        'grazing/lower': (0.0, 0.0, 0.0),
        'grazing/mirror': (0.79, 0.74, 86000000.0),
        'grazing/same': (0.024, 0.068, 0.00095),
        'grazing/opposite': (0.0, 0.0, 0.0),
        'grazing/lobe': (0.52, 0.46, 45000000.0),
        'below/upper': (0.0, 0.0, 0.0),
        'below/lower': (0.0, 0.0, 0.0),
        'below/mirror': (0.0, 0.0, 0.0),
        'below/same': (0.0, 0.0, 0.0),
        'below/opposite': (0.0, 0.0, 0.0),
        'below/lobe': (0.0, 0.0, 0.0),
        'horizon/upper': (0.48, 0.32, 24000.0),
        'horizon/lower': (0.0, 0.0, 0.0),
        'horizon/mirror': (0.0, 0.0, 0.0),
        'horizon/same': (0.0, 0.0, 1.1e-06),
        'horizon/opposite': (0.0, 0.0, 0.0),
        'horizon/lobe': (0.0, 0.0, 0.0),
    },
    'dielectric': {
        'random/regular': (0.0, None, None),
        'random/grazing': (0.0, None, None),
        'random/below': (0.0, None, None),
        'axes/regular': (0.0, None, None),
        'axes/grazing': (0.0, None, None),
        'axes/below': (0.0, None, None),
        'band/regular': (0.0, None, None),
        'band/grazing': (0.0, None, None),
        'band/below': (0.0, None, None),
        'z/horizon': (0.0, None, None),
        'regular/upper': (0.0, 0.0, 0.0),
        'regular/lower': (0.0, 0.0, 0.0),
        'regular/mirror': (0.0, 0.0, 0.0),
        'regular/same': (0.0, 0.0, 0.0),
        'regular/opposite': (0.0, 0.0, 0.0),
        'regular/lobe': (0.0, 0.0, 0.0),
        'grazing/upper': (0.0, 0.0, 0.0),
        'grazing/lower': (0.0, 0.0, 0.0),
        'grazing/mirror': (0.0, 0.0, 0.0),
        'grazing/same': (0.0, 0.0, 0.0),
        'grazing/opposite': (0.0, 0.0, 0.0),
        'grazing/lobe': (0.0, 0.0, 0.0),
        'below/upper': (0.0, 0.0, 0.0),
        'below/lower': (0.0, 0.0, 0.0),
        'below/mirror': (0.0, 0.0, 0.0),
        'below/same': (0.0, 0.0, 0.0),
        'below/opposite': (0.0, 0.0, 0.0),
        'below/lobe': (0.0, 0.0, 0.0),
        'horizon/upper': (0.0, 0.0, 0.0),
        'horizon/lower': (0.0, 0.0, 0.0),
        'horizon/mirror': (0.0, 0.0, 0.0),
        'horizon/same': (0.0, 0.0, 0.0),
        'horizon/opposite': (0.0, 0.0, 0.0),
        'horizon/lobe': (0.0, 0.0, 0.0),
    },
    'plastic_narrow': {
        'random/regular': (0.13, 0.0, 6e-07),
        'random/grazing': (0.16, 0.0, 7.7e-07),
        'random/below': (0.0, None, None),
        'axes/regular': (0.11, 0.0, 1.1e-07),
        'axes/grazing': (0.14, 0.0, 8.9e-08),
        'axes/below': (0.0, None, None),
        'band/regular': (0.12, 0.0, 3.5e-07),
        'band/grazing': (0.14, 0.0, 1.7e-07),
        'band/below': (0.0, None, None),
        'z/horizon': (0.45, None, None),
        'regular/upper': (0.0, 0.00049, 0.0015),
        'regular/lower': (0.0, 0.0, 0.0),
        'regular/mirror': (0.28, 0.46, 0.51),
        'regular/same': (0.00049, 0.00025, 0.00023),
        'regular/opposite': (0.0, 0.0, 0.0),
        'regular/lobe': (0.11, 0.17, 0.3),
        'grazing/upper': (0.002, 0.0013, 0.00052),
        'grazing/lower': (0.0, 0.0, 0.0),
        'grazing/mirror': (0.85, 0.82, 230000000000.0),
        'grazing/same': (0.0, 0.00049, 0.00019),
        'grazing/opposite': (0.0, 0.0, 0.0),
        'grazing/lobe': (0.24, 0.24, 630000000000.0),
        'below/upper': (0.0, 0.0, 0.0),
        'below/lower': (0.0, 0.0, 0.0),
        'below/mirror': (0.0, 0.0, 0.0),
        'below/same': (0.0, 0.0, 0.0),
        'below/opposite': (0.0, 0.0, 0.0),
        'below/lobe': (0.0, 0.0, 0.0),
        'horizon/upper': (0.48, 0.32, 61.0),
        'horizon/lower': (0.0, 0.0, 0.0),
        'horizon/mirror': (0.0, 0.0, 0.0),
        'horizon/same': (0.0, 0.0, 2.4e-06),
        'horizon/opposite': (0.0, 0.0, 0.0),
        'horizon/lobe': (0.0, 0.0, 0.0),
    },
    'plastic_wide': {
        'random/regular': (0.0, 0.0, 7.5e-07),
        'random/grazing': (0.011, 0.0, 8.4e-07),
        'random/below': (0.0, None, None),
        'axes/regular': (0.0, 0.0, 1.1e-07),
        'axes/grazing': (0.0096, 0.0, 1.1e-07),
        'axes/below': (0.0, None, None),
        'band/regular': (0.0, 0.0, 5.3e-07),
        'band/grazing': (0.0088, 0.0, 2.3e-07),
        'band/below': (0.0, None, None),
        'z/horizon': (0.45, None, None),
        'regular/upper': (0.0, 0.0, 6.6e-05),
        'regular/lower': (0.0, 0.0, 0.0),
        'regular/mirror': (0.0, 0.0, 0.00012),
        'regular/same': (0.0, 0.0, 4.4e-05),
        'regular/opposite': (0.0, 0.0, 0.0),
        'regular/lobe': (0.0, 0.0, 9.1e-05),
        'grazing/upper': (0.0025, 0.0015, 0.00065),
        'grazing/lower': (0.0, 0.0, 0.0),
        'grazing/mirror': (0.75, 0.65, 5700000.0),
        'grazing/same': (0.0, 0.00074, 0.00021),
        'grazing/opposite': (0.0, 0.0, 0.0),
        'grazing/lobe': (0.14, 0.12, 17.0),
        'below/upper': (0.0, 0.0, 0.0),
        'below/lower': (0.0, 0.0, 0.0),
        'below/mirror': (0.0, 0.0, 0.0),
        'below/same': (0.0, 0.0, 0.0),
        'below/opposite': (0.0, 0.0, 0.0),
        'below/lobe': (0.0, 0.0, 0.0),
        'horizon/upper': (0.48, 0.32, 5100.0),
        'horizon/lower': (0.0, 0.0, 0.0),
        'horizon/mirror': (0.0, 0.0, 0.0),
        'horizon/same': (0.0, 0.0, 2.4e-06),
        'horizon/opposite': (0.0, 0.0, 0.0),
        'horizon/lobe': (0.0, 0.0, 0.0),
    },
    'sss': {
        'random/regular': (0.0, 1.7e-06, 6.5e-06),
        'random/grazing': (0.0, 7.1e-07, 2.3e-06),
        'random/below': (0.0, None, None),
        'axes/regular': (0.0, 2.2e-07, 3e-07),
        'axes/grazing': (0.0, 2.3e-07, 2.9e-07),
        'axes/below': (0.0, None, None),
        'band/regular': (0.0, 3.2e-07, 5.2e-07),
        'band/grazing': (0.0, 2.8e-07, 4.3e-07),
        'band/below': (0.0, None, None),
        'z/horizon': (0.0, None, None),
        'regular/upper': (0.0, 0.0, 2.6e-06),
        'regular/lower': (0.0, 0.0, 0.0),
        'regular/mirror': (0.0, 0.0, 5.9e-07),
        'regular/same': (0.0, 0.0, 7.9e-07),
        'regular/opposite': (0.0, 0.0, 0.0),
        'regular/lobe': (0.0, 0.0, 5.8e-07),
        'grazing/upper': (0.0, 0.0, 3.8e-06),
        'grazing/lower': (0.0, 0.0, 0.0),
        'grazing/mirror': (0.0, 0.0, 2.9e-06),
        'grazing/same': (0.0, 0.0, 2.9e-06),
        'grazing/opposite': (0.0, 0.0, 0.0),
        'grazing/lobe': (0.0, 0.0, 7.3e-07),
        'below/upper': (0.0, 0.0, 0.0),
        'below/lower': (0.0, 0.0, 0.0),
        'below/mirror': (0.0, 0.0, 0.0),
        'below/same': (0.0, 0.0, 0.0),
        'below/opposite': (0.0, 0.0, 0.0),
        'below/lobe': (0.0, 0.0, 0.0),
        'horizon/upper': (0.48, 0.32, 32.0),
        'horizon/lower': (0.0, 0.0, 0.0),
        'horizon/mirror': (0.0, 0.0, 0.0),
        'horizon/same': (0.0, 0.32, 26.0),
        'horizon/opposite': (0.0, 0.0, 0.0),
        'horizon/lobe': (0.5, 0.31, 32.0),
    },
    'carpaint': {
        'random/regular': (0.2, None, None),
        'random/grazing': (0.27, None, None),
        'random/below': (0.02, None, None),
        'axes/regular': (0.15, None, None),
        'axes/grazing': (0.23, None, None),
        'axes/below': (0.015, None, None),
        'band/regular': (0.17, None, None),
        'band/grazing': (0.24, None, None),
        'band/below': (0.013, None, None),
        'z/horizon': (0.21, None, None),
        'regular/upper': (0.00074, 0.91, 3400.0),
        'regular/lower': (0.0, 0.0, 0.0),
        'regular/mirror': (0.28, 0.96, 3.9),
        'regular/same': (0.00049, 0.93, 910.0),
        'regular/opposite': (0.0, 0.0, 0.0),
        'regular/lobe': (0.29, 0.98, 1800.0),
        'grazing/upper': (0.0025, 0.66, 1200.0),
        'grazing/lower': (0.0, 0.0, 0.0),
        'grazing/mirror': (0.85, 0.84, 64000000000.0),
        'grazing/same': (0.0066, 0.78, 2.9),
        'grazing/opposite': (0.0, 0.0, 0.0),
        'grazing/lobe': (0.54, 0.82, 63000000000.0),
        'below/upper': (0.0, 0.0, 0.0),
        'below/lower': (0.0, 0.0, 0.0),
        'below/mirror': (0.0, 0.0, 0.0),
        'below/same': (0.0, 0.0, 0.0),
        'below/opposite': (0.0, 0.0, 0.0),
        'below/lobe': (0.0, 0.0, 0.0),
        'horizon/upper': (0.48, 0.32, 6300.0),
        'horizon/lower': (0.0, 0.0, 0.0),
        'horizon/mirror': (0.0, 0.0, 0.0),
        'horizon/same': (0.0, 0.32, 11.0),
        'horizon/opposite': (0.0, 0.0, 0.0),
        'horizon/lobe': (0.13, 0.072, 49000.0),
    },
    'pbr_narrow': {
        'random/regular': (0.42, None, None),
        'random/grazing': (0.54, None, None),
        'random/below': (0.0, None, None),
        'axes/regular': (0.53, None, None),
        'axes/grazing': (0.41, None, None),
        'axes/below': (0.0, None, None),
        'band/regular': (0.5, None, None),
        'band/grazing': (0.46, None, None),
        'band/below': (0.0, None, None),
        'z/horizon': (0.41, None, None),
        'regular/upper': (0.00025, 0.00074, 0.0015),
        'regular/lower': (0.0, 0.0, 0.0),
        'regular/mirror': (0.28, 0.46, 2200000000.0),
        'regular/same': (0.00049, 0.00049, 0.00028),
        'regular/opposite': (0.0, 0.0, 0.0),
        'regular/lobe': (0.32, 0.5, 1700000000.0),
        'grazing/upper': (0.003, 0.003, 0.00042),
        'grazing/lower': (0.0, 0.0, 0.0),
        'grazing/mirror': (0.85, 0.82, 23000000000000.0),
        'grazing/same': (0.017, 0.053, 0.00064),
        'grazing/opposite': (0.0, 0.0, 0.0),
        'grazing/lobe': (0.7, 0.69, 23000000000000.0),
        'below/upper': (0.0, 0.0, 0.0),
        'below/lower': (0.0, 0.0, 0.0),
        'below/mirror': (0.0, 0.0, 0.0),
        'below/same': (0.0, 0.0, 0.0),
        'below/opposite': (0.0, 0.0, 0.0),
        'below/lobe': (0.0, 0.0, 0.0),
        'horizon/upper': (0.48, 0.32, 31.0),
        'horizon/lower': (0.0, 0.0, 0.0),
        'horizon/mirror': (0.0, 0.0, 0.0),
        'horizon/same': (0.0, 0.3, 26.0),
        'horizon/opposite': (0.0, 0.0, 0.0),
        'horizon/lobe': (0.48, 0.29, 31.0),
    },
    'pbr_wide': {
        'random/regular': (0.0, None, None),
        'random/grazing': (0.011, None, None),
        'random/below': (0.0, None, None),
        'axes/regular': (0.0, None, None),
        'axes/grazing': (0.0047, None, None),
        'axes/below': (0.0, None, None),
        'band/regular': (0.0, None, None),
        'band/grazing': (0.0057, None, None),
        'band/below': (0.0, None, None),
        'z/horizon': (0.21, None, None),
        'regular/upper': (0.0, 0.0, 9.1e-06),
        'regular/lower': (0.0, 0.0, 0.0),
        'regular/mirror': (0.0, 0.0, 1.1e-05),
        'regular/same': (0.0, 0.0, 4.2e-06),
        'regular/opposite': (0.0, 0.0, 0.0),
        'regular/lobe': (0.0, 0.0, 7.6e-06),
        'grazing/upper': (0.004, 0.004, 0.00066),
        'grazing/lower': (0.0, 0.0, 0.0),
        'grazing/mirror': (0.74, 0.65, 850000.0),
        'grazing/same': (0.024, 0.067, 0.0009),
        'grazing/opposite': (0.0, 0.0, 0.0),
        'grazing/lobe': (0.32, 0.27, 440000.0),
        'below/upper': (0.0, 0.0, 0.0),
        'below/lower': (0.0, 0.0, 0.0),
        'below/mirror': (0.0, 0.0, 0.0),
        'below/same': (0.0, 0.0, 0.0),
        'below/opposite': (0.0, 0.0, 0.0),
        'below/lobe': (0.0, 0.0, 0.0),
        'horizon/upper': (0.48, 0.32, 30000.0),
        'horizon/lower': (0.0, 0.0, 0.0),
        'horizon/mirror': (0.0, 0.0, 0.0),
        'horizon/same': (0.0, 0.3, 26.0),
        'horizon/opposite': (0.0, 0.0, 0.0),
        'horizon/lobe': (0.48, 0.29, 160.0),
    },
    'pbr_transmissive': {
        'random/regular': (0.00098, None, None),
        'random/grazing': (0.031, None, None),
        'random/below': (0.021, None, None),
        'axes/regular': (0.00025, None, None),
        'axes/grazing': (0.0, None, None),
        'axes/below': (0.0, None, None),
        'band/regular': (0.00049, None, None),
        'band/grazing': (0.032, None, None),
        'band/below': (0.018, None, None),
        'z/horizon': (0.46, None, None),
        'regular/upper': (0.0, 0.0, 0.00012),
        'regular/lower': (0.00025, 0.00025, 0.00026),
        'regular/mirror': (0.28, 0.45, 190000000.0),
        'regular/same': (0.0, 0.0, 2.4e-05),
        'regular/opposite': (0.0, 0.0, 5.7e-05),
        'regular/lobe': (0.033, 0.046, 85000000.0),
        'grazing/upper': (0.00025, 0.00025, 0.00062),
        'grazing/lower': (0.0049, 0.0027, 0.00032),
        'grazing/mirror': (0.74, 0.64, 17000000000000.0),
        'grazing/same': (0.0, 0.0, 6.1e-05),
        'grazing/opposite': (0.0, 0.0, 1.2e-05),
        'grazing/lobe': (0.67, 0.58, 5.7e+16),
        'below/upper': (0.0, 0.0, 0.0),
        'below/lower': (0.0, 0.0, 0.0),
        'below/mirror': (0.0, 0.0, 0.0),
        'below/same': (0.0, 0.0, 0.0),
        'below/opposite': (0.0, 0.0, 0.0),
        'below/lobe': (0.0, 0.0, 0.0),
        'horizon/upper': (0.2, 0.32, 76.0),
        'horizon/lower': (0.0, 0.066, 0.54),
        'horizon/mirror': (0.0, 0.0, 1e-06),
        'horizon/same': (0.0, 0.3, 23.0),
        'horizon/opposite': (0.0, 0.0, 1e-06),
        'horizon/lobe': (0.34, 0.28, 91.0),
    },
}
ILL_CONDITIONED = {
    'lambert': ('horizon/upper', 'horizon/lobe'),
    'rough_metal': ('random/grazing', 'axes/grazing', 'z/horizon', 'grazing/upper', 'grazing/mirror', 'grazing/same', 'grazing/lobe', 'horizon/upper'),
    'mirror': ('z/horizon',),
    'gold_like': ('random/regular', 'random/grazing', 'axes/grazing', 'band/grazing', 'z/horizon', 'regular/mirror', 'regular/lobe', 'grazing/upper', 'grazing/mirror', 'grazing/same', 'grazing/lobe', 'horizon/upper'),
    'glass': (),
    'plastic': ('random/regular', 'random/grazing', 'axes/regular', 'axes/grazing', 'band/regular', 'band/grazing', 'z/horizon', 'regular/mirror', 'regular/lobe', 'grazing/upper', 'grazing/mirror', 'grazing/lobe', 'horizon/upper'),
    'thick_plastic': ('random/grazing', 'axes/grazing', 'band/grazing', 'z/horizon', 'grazing/upper', 'grazing/mirror', 'grazing/lobe', 'horizon/upper'),
    'skin': ('horizon/upper', 'horizon/lobe'),
    'carpaint': ('random/regular', 'random/grazing', 'random/below', 'axes/regular', 'axes/grazing', 'axes/below', 'band/regular', 'band/grazing', 'band/below', 'z/horizon', 'regular/mirror', 'regular/lobe', 'grazing/upper', 'grazing/mirror', 'grazing/same', 'grazing/lobe', 'horizon/upper', 'horizon/lobe'),
    'carpaint_dielectric_base': ('random/regular', 'random/grazing', 'random/below', 'axes/regular', 'axes/grazing', 'axes/below', 'band/regular', 'band/grazing', 'band/below', 'z/horizon', 'regular/mirror', 'regular/lobe', 'grazing/mirror', 'grazing/lobe', 'horizon/upper', 'horizon/lobe'),
    'floor': ('horizon/upper', 'horizon/lobe'),
    'metal_schlick_0': ('z/horizon',),
    'metal_conductor_0': ('z/horizon',),
    'metal_schlick_0.001': ('z/horizon',),
    'metal_conductor_0.001': ('z/horizon',),
    'metal_schlick_0.0011': ('random/regular', 'random/grazing', 'axes/regular', 'axes/grazing', 'band/regular', 'band/grazing', 'z/horizon', 'regular/mirror', 'regular/lobe', 'grazing/mirror', 'grazing/lobe'),
    'metal_conductor_0.0011': ('random/regular', 'random/grazing', 'axes/regular', 'axes/grazing', 'band/regular', 'band/grazing', 'z/horizon', 'regular/mirror', 'regular/lobe', 'grazing/mirror', 'grazing/lobe'),
    'metal_schlick_0.02': ('random/regular', 'random/grazing', 'axes/regular', 'axes/grazing', 'band/regular', 'band/grazing', 'z/horizon', 'regular/mirror', 'regular/lobe', 'grazing/mirror', 'grazing/same', 'grazing/lobe', 'horizon/upper'),
    'metal_conductor_0.02': ('random/regular', 'random/grazing', 'axes/regular', 'axes/grazing', 'band/regular', 'band/grazing', 'z/horizon', 'regular/mirror', 'regular/lobe', 'grazing/mirror', 'grazing/same', 'grazing/lobe', 'horizon/upper'),
    'metal_schlick_0.2': ('random/regular', 'random/grazing', 'axes/grazing', 'band/grazing', 'z/horizon', 'regular/mirror', 'regular/lobe', 'grazing/upper', 'grazing/mirror', 'grazing/same', 'grazing/lobe', 'horizon/upper'),
    'metal_conductor_0.2': ('random/regular', 'random/grazing', 'axes/grazing', 'band/grazing', 'z/horizon', 'regular/mirror', 'regular/lobe', 'grazing/upper', 'grazing/mirror', 'grazing/same', 'grazing/lobe', 'horizon/upper'),
    'metal_schlick_1': ('random/grazing', 'z/horizon', 'grazing/upper', 'grazing/mirror', 'grazing/same', 'grazing/lobe', 'horizon/upper'),
    'metal_conductor_1': ('random/grazing', 'z/horizon', 'grazing/upper', 'grazing/mirror', 'grazing/same', 'grazing/lobe', 'horizon/upper'),
    'plastic_coat_0.04': ('random/regular', 'random/grazing', 'axes/regular', 'axes/grazing', 'band/regular', 'band/grazing', 'z/horizon', 'regular/mirror', 'regular/lobe', 'grazing/upper', 'grazing/mirror', 'grazing/lobe', 'horizon/upper'),
    'plastic_coat_0.3': ('random/grazing', 'axes/grazing', 'band/grazing', 'z/horizon', 'grazing/upper', 'grazing/mirror', 'grazing/lobe', 'horizon/upper'),
    'plastic_coat_1': ('band/grazing', 'z/horizon', 'grazing/upper', 'grazing/mirror', 'grazing/lobe', 'horizon/upper'),
    'pbr_m0_r0': ('z/horizon', 'regular/mirror', 'regular/lobe', 'grazing/mirror', 'grazing/lobe', 'horizon/upper', 'horizon/lobe'),
    'pbr_m0_r0.001': ('z/horizon', 'regular/mirror', 'regular/lobe', 'grazing/mirror', 'grazing/lobe', 'horizon/upper', 'horizon/lobe'),
    'pbr_m0_r0.05': ('random/regular', 'random/grazing', 'axes/regular', 'axes/grazing', 'band/regular', 'band/grazing', 'z/horizon', 'regular/mirror', 'regular/lobe', 'grazing/mirror', 'grazing/lobe', 'horizon/upper', 'horizon/lobe'),
    'pbr_m0_r0.6': ('z/horizon', 'grazing/mirror', 'grazing/lobe', 'horizon/upper', 'horizon/lobe'),
    'pbr_m0_r1': ('z/horizon', 'grazing/mirror', 'grazing/lobe', 'horizon/upper', 'horizon/lobe'),
    'pbr_m0.5_r0': ('z/horizon', 'regular/mirror', 'regular/lobe', 'grazing/mirror', 'grazing/lobe', 'horizon/upper', 'horizon/lobe'),
    'pbr_m0.5_r0.001': ('z/horizon', 'regular/mirror', 'regular/lobe', 'grazing/mirror', 'grazing/lobe', 'horizon/upper', 'horizon/lobe'),
    'pbr_m0.5_r0.05': ('random/regular', 'random/grazing', 'axes/regular', 'axes/grazing', 'band/regular', 'band/grazing', 'z/horizon', 'regular/mirror', 'regular/lobe', 'grazing/mirror', 'grazing/lobe', 'horizon/upper', 'horizon/lobe'),
    'pbr_m0.5_r0.6': ('random/grazing', 'axes/grazing', 'band/grazing', 'z/horizon', 'grazing/upper', 'grazing/mirror', 'grazing/lobe', 'horizon/upper', 'horizon/lobe'),
    'pbr_m0.5_r1': ('random/grazing', 'axes/grazing', 'band/grazing', 'z/horizon', 'grazing/upper', 'grazing/mirror', 'grazing/lobe', 'horizon/upper', 'horizon/lobe'),
    'pbr_m1_r0': ('z/horizon', 'regular/mirror', 'regular/lobe', 'grazing/mirror', 'grazing/lobe', 'horizon/upper', 'horizon/lobe'),
    'pbr_m1_r0.001': ('z/horizon', 'regular/mirror', 'regular/lobe', 'grazing/mirror', 'grazing/lobe', 'horizon/upper', 'horizon/lobe'),
    'pbr_m1_r0.05': ('random/regular', 'random/grazing', 'axes/regular', 'axes/grazing', 'band/regular', 'band/grazing', 'z/horizon', 'regular/mirror', 'regular/lobe', 'grazing/upper', 'grazing/mirror', 'grazing/same', 'grazing/lobe', 'horizon/upper', 'horizon/lobe'),
    'pbr_m1_r0.6': ('random/grazing', 'axes/grazing', 'band/grazing', 'z/horizon', 'grazing/upper', 'grazing/mirror', 'grazing/same', 'grazing/lobe', 'horizon/upper', 'horizon/lobe'),
    'pbr_m1_r1': ('random/grazing', 'axes/grazing', 'band/grazing', 'z/horizon', 'grazing/upper', 'grazing/mirror', 'grazing/same', 'grazing/lobe', 'horizon/upper', 'horizon/lobe'),
    'pbr_t0_ior1_r0': ('z/horizon', 'regular/mirror', 'regular/lobe', 'grazing/mirror', 'grazing/lobe', 'horizon/upper', 'horizon/lobe'),
    'pbr_t0_ior1_r0.35': ('random/grazing', 'grazing/mirror', 'horizon/upper', 'horizon/lobe'),
    'pbr_t0_ior1.45_r0': ('z/horizon', 'regular/mirror', 'regular/lobe', 'grazing/mirror', 'grazing/lobe', 'horizon/upper', 'horizon/lobe'),
    'pbr_t0_ior1.45_r0.35': ('random/grazing', 'grazing/mirror', 'horizon/upper', 'horizon/lobe'),
    'pbr_t0.7_ior1_r0': ('random/grazing', 'random/below', 'band/grazing', 'band/below', 'z/horizon', 'regular/mirror', 'regular/lobe', 'grazing/mirror', 'grazing/lobe', 'horizon/upper', 'horizon/lobe'),
    'pbr_t0.7_ior1_r0.35': ('grazing/mirror', 'grazing/lobe', 'horizon/upper', 'horizon/lobe'),
    'pbr_t0.7_ior1.45_r0': ('z/horizon', 'regular/mirror', 'regular/lobe', 'grazing/mirror', 'grazing/lobe', 'horizon/upper', 'horizon/lobe'),
    'pbr_t0.7_ior1.45_r0.35': ('random/grazing', 'grazing/lower', 'grazing/mirror', 'grazing/lobe', 'horizon/upper', 'horizon/lobe'),
    'pbr_t1_ior1_r0': ('random/grazing', 'random/below', 'band/grazing', 'band/below', 'z/horizon', 'regular/mirror', 'regular/lobe', 'grazing/mirror', 'grazing/lobe', 'horizon/upper', 'horizon/lobe'),
    'pbr_t1_ior1_r0.35': ('grazing/mirror', 'grazing/lobe', 'horizon/upper', 'horizon/lobe'),
    'pbr_t1_ior1.45_r0': ('z/horizon', 'regular/mirror', 'regular/lobe', 'grazing/mirror', 'grazing/lobe', 'horizon/upper', 'horizon/lobe'),
    'pbr_t1_ior1.45_r0.35': ('random/grazing', 'grazing/lower', 'grazing/mirror', 'grazing/lobe', 'horizon/upper', 'horizon/lobe'),
    'sss_skin': ('horizon/upper', 'horizon/lobe'),
    'sss_jade': ('horizon/upper', 'horizon/lobe'),
}
# END MEASURED
