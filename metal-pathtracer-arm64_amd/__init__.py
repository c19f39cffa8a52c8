"""MI355X wavefront path tracer — Python host bindings over the C-ABI (include/ptr_abi.h, include/ptr_post.h, include/ptr_stats.h).

The package is only plumbing: it loads ``libptr_hip.so`` (hand-written HIP kernels + C++ host layer) with
ctypes and mirrors the POD structs of the ABI.  There is no CPU fallback: every render entry point needs the
HIP library and a GPU, and raises if either is missing.

Reference surface mirrored here (paths relative to the reference checkout):
  HostScene.load      <- SceneManager::loadSceneFromPath      src/renderer/SceneManager.mm:677-722
  DeviceScene         <- SceneResources::rebuildAccelerationStructures  src/renderer/SceneResources.mm:2055-2259
  DeviceScene.render  <- IHeadlessRenderer::render            include/headless/IHeadlessRenderer.h:42-52
  write_image         <- WriteImage                           src/renderer/ImageWriter.mm:609-627
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Tuple

import numpy as np

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG_DIR, "libptr_hip.so")
CLI_PATH = os.path.join(_PKG_DIR, "PathTracerHeadless")

# ----------------------------------------------------------------------------- ABI structs


class PtrSphere(C.Structure):
    _fields_ = [("centerRadius", C.c_float * 4), ("materialIndex", C.c_uint32 * 4)]


class PtrRect(C.Structure):
    _fields_ = [
        ("corner", C.c_float * 4),
        ("edgeU", C.c_float * 4),
        ("edgeV", C.c_float * 4),
        ("normalAndPlane", C.c_float * 4),
        ("materialTwoSided", C.c_uint32 * 4),
    ]


class PtrMaterial(C.Structure):
    _fields_ = [
        ("baseColorRoughness", C.c_float * 4),
        ("typeEta", C.c_float * 4),
        ("emission", C.c_float * 4),
        ("conductorEta", C.c_float * 4),
        ("conductorK", C.c_float * 4),
        ("coatParams", C.c_float * 4),
        ("coatTint", C.c_float * 4),
        ("coatAbsorption", C.c_float * 4),
        ("dielectricSigmaA", C.c_float * 4),
        ("sssSigmaA", C.c_float * 4),
        ("sssSigmaS", C.c_float * 4),
        ("sssParams", C.c_float * 4),
        ("carpaintBaseParams", C.c_float * 4),
        ("carpaintFlakeParams", C.c_float * 4),
        ("carpaintBaseEta", C.c_float * 4),
        ("carpaintBaseK", C.c_float * 4),
        ("carpaintBaseTint", C.c_float * 4),
        ("textureIndices0", C.c_uint32 * 4),
        ("textureIndices1", C.c_uint32 * 4),
        ("materialFlags", C.c_uint32),
        ("materialPad", C.c_uint32 * 3),
        ("pbrParams", C.c_float * 4),
        ("pbrExtras", C.c_float * 4),
        ("textureUvSet0", C.c_uint32 * 4),
        ("textureUvSet1", C.c_uint32 * 4),
        ("textureTransform", (C.c_float * 4) * 12),
    ]


class PtrMeshDesc(C.Structure):
    _fields_ = [
        ("positions", C.POINTER(C.c_float)),
        ("normals", C.POINTER(C.c_float)),
        ("indices", C.POINTER(C.c_uint32)),
        ("vertexCount", C.c_uint32),
        ("indexCount", C.c_uint32),
        ("localToWorld", C.c_float * 16),
        ("materialIndex", C.c_uint32),
        ("pad", C.c_uint32),
        ("uv0", C.POINTER(C.c_float)),
        ("uv1", C.POINTER(C.c_float)),
        ("tangents", C.POINTER(C.c_float)),
    ]


class PtrTexture(C.Structure):
    _fields_ = [
        ("rgba", C.POINTER(C.c_float)),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("wrapS", C.c_uint32),
        ("wrapT", C.c_uint32),
        ("filter", C.c_uint32),
        ("pad", C.c_uint32),
    ]


class PtrSceneDesc(C.Structure):
    _fields_ = [
        ("spheres", C.POINTER(PtrSphere)),
        ("rects", C.POINTER(PtrRect)),
        ("materials", C.POINTER(PtrMaterial)),
        ("meshes", C.POINTER(PtrMeshDesc)),
        ("envRgba", C.POINTER(C.c_float)),
        ("sphereCount", C.c_uint32),
        ("rectCount", C.c_uint32),
        ("materialCount", C.c_uint32),
        ("meshCount", C.c_uint32),
        ("envWidth", C.c_uint32),
        ("envHeight", C.c_uint32),
        ("textures", C.POINTER(PtrTexture)),
        ("textureCount", C.c_uint32),
        ("pad", C.c_uint32),
    ]


class PtrSettings(C.Structure):
    _fields_ = [
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("maxDepth", C.c_uint32),
        ("seed", C.c_uint32),
        ("enableRussianRoulette", C.c_uint32),
        ("enableSpecularNee", C.c_uint32),
        ("enableMnee", C.c_uint32),
        ("enableMneeSecondary", C.c_uint32),
        ("cameraTarget", C.c_float * 3),
        ("cameraDistance", C.c_float),
        ("cameraYaw", C.c_float),
        ("cameraPitch", C.c_float),
        ("cameraVerticalFov", C.c_float),
        ("cameraDefocusAngle", C.c_float),
        ("cameraFocusDistance", C.c_float),
        ("backgroundMode", C.c_uint32),
        ("backgroundColor", C.c_float * 3),
        ("environmentRotation", C.c_float),
        ("environmentIntensity", C.c_float),
        ("fireflyClampEnabled", C.c_uint32),
        ("fireflyClampFactor", C.c_float),
        ("fireflyClampFloor", C.c_float),
        ("throughputClamp", C.c_float),
        ("specularTailClampBase", C.c_float),
        ("specularTailClampRoughnessScale", C.c_float),
        ("minSpecularPdf", C.c_float),
        ("fireflyClampMaxContribution", C.c_float),
        ("emissionScale", C.c_float),
        ("metalSemantics", C.c_uint32),
        ("sssMode", C.c_uint32),
        ("sssMaxSteps", C.c_uint32),
        ("debugShadowSlack", C.c_float),
    ]

    def copy(self) -> "PtrSettings":
        out = PtrSettings()
        C.memmove(C.byref(out), C.byref(self), C.sizeof(PtrSettings))
        return out


class PtrRenderStats(C.Structure):
    _fields_ = [
        ("totalSeconds", C.c_double),
        ("avgMsPerSample", C.c_double),
        ("uploadSeconds", C.c_double),
        ("traceKernelMs", C.c_double),
        ("shadeKernelMs", C.c_double),
        ("shadowKernelMs", C.c_double),
        ("traceLaunches", C.c_uint64),
        ("samples", C.c_uint64),
        ("primaryRays", C.c_uint64),
        ("extendRays", C.c_uint64),
        ("shadowRays", C.c_uint64),
        ("nodesVisited", C.c_uint64),
        ("leafPrimTests", C.c_uint64),
        ("extendNodesVisited", C.c_uint64),
        ("extendLeafPrimTests", C.c_uint64),
        ("shadedHits", C.c_uint64),
        ("triangleHits", C.c_uint64),
        ("shadowEarlyExits", C.c_uint64),
        ("tailKernelMs", C.c_double),
    ]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


class PtrHit(C.Structure):
    _fields_ = [
        ("t", C.c_float),
        ("u", C.c_float),
        ("v", C.c_float),
        ("primType", C.c_uint32),
        ("geomIndex", C.c_uint32),
        ("primIndex", C.c_uint32),
        ("ng", C.c_float * 3),
        ("pad", C.c_uint32),
    ]


HIT_DTYPE = np.dtype(
    [("t", "<f4"), ("u", "<f4"), ("v", "<f4"), ("primType", "<u4"), ("geomIndex", "<u4"), ("primIndex", "<u4"),
     ("ng", "<f4", (3,)), ("pad", "<u4")]
)

class PtrDenoiseParams(C.Structure):
    """include/ptr_post.h PtrDenoiseParams; PtrDenoiseParams.defaults() asks the library for its defaults."""
    _fields_ = [
        ("iterations", C.c_uint32),
        ("sigmaLuminance", C.c_float),
        ("sigmaNormal", C.c_float),
        ("sigmaDepth", C.c_float),
        ("flags", C.c_uint32),
    ]

    @classmethod
    def defaults(cls, **overrides) -> "PtrDenoiseParams":
        p = cls()
        load_library().ptr_denoise_default_params(C.byref(p))
        for k, v in overrides.items():
            setattr(p, k, v)
        return p


PTR_DENOISE_DEMODULATE = 1   # PtrDenoiseParams.flags bit 0


class PtrAdaptiveParams(C.Structure):
    """include/ptr_adaptive.h PtrAdaptiveParams; PtrAdaptiveParams.defaults(max_spp) asks the library for its defaults."""
    _fields_ = [
        ("minSpp", C.c_uint32),
        ("maxSpp", C.c_uint32),
        ("stepSpp", C.c_uint32),
        ("threshold", C.c_float),
    ]

    @classmethod
    def defaults(cls, max_spp: int, **overrides) -> "PtrAdaptiveParams":
        p = cls()
        load_library().ptr_adaptive_default_params(C.byref(p), max_spp)
        for k, v in overrides.items():
            setattr(p, k, v)
        return p


ADAPTIVE_INFO_ROUNDS = 32   # PTR_ADAPTIVE_INFO_ROUNDS


class PtrAdaptiveInfo(C.Structure):
    """include/ptr_adaptive.h PtrAdaptiveInfo."""
    _fields_ = [
        ("rounds", C.c_uint32),
        ("pixelsAtMax", C.c_uint32),
        ("totalSamples", C.c_uint64),
        ("activeAfter", C.c_uint32 * ADAPTIVE_INFO_ROUNDS),
    ]

    def active_counts(self) -> list:
        """the length of the active list after each round (the first 32)"""
        return [int(v) for v in self.activeAfter[: min(self.rounds, ADAPTIVE_INFO_ROUNDS)]]


MULTI_MAX_PARTS = 64   # PTR_MULTI_MAX_PARTS


class PtrMultiInfo(C.Structure):
    """include/ptr_multi.h PtrMultiInfo."""
    _fields_ = [
        ("parts", C.c_uint32),
        ("stagedParts", C.c_uint32),
        ("partSamples", C.c_uint64 * MULTI_MAX_PARTS),
        ("partRenderSeconds", C.c_double * MULTI_MAX_PARTS),
        ("partWaitSeconds", C.c_double * MULTI_MAX_PARTS),
    ]

    def per_part(self) -> list:
        """[(samples, render seconds, wait seconds)] of the partitions the frame ran on"""
        return [(int(self.partSamples[p]), float(self.partRenderSeconds[p]), float(self.partWaitSeconds[p])) for p in range(self.parts)]


assert C.sizeof(PtrSphere) == 32 and C.sizeof(PtrRect) == 80 and C.sizeof(PtrMaterial) == 576
assert C.sizeof(PtrHit) == HIT_DTYPE.itemsize == 40

# PtrSettings.metalSemantics bits (include/ptr_abi.h PTR_METAL_*)
PTR_METAL_MEDIA = 1
PTR_METAL_THIN = 2
PTR_METAL_FACE_NORMAL = 4
PTR_METAL_SPECULAR = 8
PTR_METAL_SSS = 16
PTR_METAL_PBR = 32
PTR_METAL_CLAMPS = 64
PTR_METAL_ENV_LOD = 128    # prefiltered environment lookups (environment_color_lod of the Metal kernel)
PTR_METAL_RAY_DIFF = 256   # first-hit ray differentials of textured lookups (with PTR_METAL_PBR)

# The C signature of every function of include/ptr_abi.h and include/ptr_debug.h, in header order: name -> (restype, argtypes).  The one
# place they are declared: load_library() applies it, tests/test_host.py holds its argument counts against the headers.
_int, _u32, _u64, _vp, _cp = C.c_int, C.c_uint32, C.c_uint64, C.c_void_p, C.c_char_p
_fp, _up, _u64p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
_desc, _settings, _material, _stats = C.POINTER(PtrSceneDesc), C.POINTER(PtrSettings), C.POINTER(PtrMaterial), C.POINTER(PtrRenderStats)
_err = [_cp, C.c_size_t]   # the trailing (char* err, size_t err_cap)
_SIGNATURES = {
    "ptr_device_count": (_int, []),
    "ptr_scene_upload": (_int, [_desc, _int, C.POINTER(_vp)] + _err),
    "ptr_scene_release": (None, [_vp]),
    "ptr_scene_info": (_int, [_vp, _u64p]),
    "ptr_scene_timings": (_int, [_vp, C.POINTER(C.c_double)]),
    "ptr_scene_prepare_geometry": (_int, [_desc, _cp, C.POINTER(C.c_double)] + _err),
    "ptr_scene_upload_prepared": (_int, [_desc, _cp, _int, C.POINTER(_vp)] + _err),
    "ptr_render": (_int, [_desc, _settings, _u32, _int, _fp, _stats] + _err),
    "ptr_render_multi": (_int, [_desc, _settings, _u32, _int, _int, _fp, _stats] + _err),
    "ptr_render_bands_device": (_int, [_vp, _settings, _u32, _u32, _u32, _vp, _vp, _int, _stats] + _err),
    "ptr_part_band_count": (_u32, [_u32, _u32, _u32]),
    "ptr_render_bands": (_int, [_vp, _settings, _u32, _u32, _u32, _fp, _int, _stats] + _err),
    "ptr_render_aovs": (_int, [_vp, _settings, _u32, _fp, _fp] + _err),
    "ptr_trace_rays": (_int, [_vp, _fp, _u64, _int, _vp, _stats] + _err),
    "ptr_host_scene_load": (_int, [_cp, _cp, C.POINTER(_vp)] + _err),
    "ptr_host_scene_free": (None, [_vp]),
    "ptr_host_scene_desc": (_int, [_vp, _desc, _settings]),
    "ptr_host_write_image": (_int, [_cp, _cp, _fp, _u32, _u32, _int, _u32, _u32, C.c_float, C.c_float] + _err),
    "ptr_host_write_exr_multilayer": (_int, [_cp, _fp, _u32, _u32, _fp, _cp] + _err),
    "ptr_host_write_exr_aovs": (_int, [_cp, _fp, _fp, _fp, _u32, _u32] + _err),
    "ptr_host_decode_image": (_int, [_cp, _u64, C.POINTER(C.c_uint8), _u64, _up, _up] + _err),
    "ptr_host_read_pfm": (_int, [_cp, _fp, _u32, _up, _up]),
    "ptr_version": (_cp, []),
    # include/ptr_debug.h (test-only device-function probes)
    "ptr_debug_eval_bsdf": (_int, [_material, _settings, _fp, _u64, _fp] + _err),
    "ptr_debug_sample_bsdf": (_int, [_material, _settings, _fp, _up, _up, _u64, _fp, _up] + _err),
    "ptr_debug_sample_lobes": (_int, [_material, _settings, _fp, _up, _up, _u64, _fp, _fp, _up, _fp] + _err),
    "ptr_debug_env_lookup": (_int, [_vp, _settings, _fp, _u64, _fp] + _err),
    "ptr_debug_env_mips": (_int, [_fp, _u32, _u32, _fp, _u64, _up]),
    "ptr_debug_env_sample": (_int, [_vp, _settings, _fp, _u64, _fp] + _err),
    "ptr_debug_env_eval": (_int, [_vp, _settings, _fp, _u64, _fp] + _err),
    "ptr_debug_rect_light_nee": (_int, [_vp, _settings, _material, _fp, _fp, _up, _u64, _fp, _up] + _err),
    "ptr_debug_light_connection": (_int, [_vp, _settings, _fp, _u64, _fp, _up] + _err),
    "ptr_debug_first_hit_textures": (_int, [_vp, _settings, _up, _u64, _fp] + _err),
    "ptr_debug_texture_sample_grad": (_int, [_vp, _u32, _fp, _u64, _fp] + _err),
    "ptr_debug_camera_rays": (_int, [_settings, _up, _u64, _fp, _up] + _err),
    "ptr_debug_render_signatures": (_int, [_vp, _settings, _fp, _up] + _err),
    "ptr_debug_texture_sample": (_int, [_vp, _u32, _fp, _u64, _fp] + _err),
    "ptr_debug_surface_hits": (_int, [_vp, _fp, _u64, _fp] + _err),
    "ptr_debug_extend_rays": (_int, [_vp, _fp, _u64, _int, _vp, _up] + _err),
    "ptr_debug_connect_rays": (_int, [_vp, _fp, _up, _u64, _u32, _up, _up] + _err),
    "ptr_debug_walk_counts": (_int, [_desc, _fp, _u64, _u32, _u64p] + _err),
    "ptr_debug_walk_stack_depths": (_int, [_desc, _fp, _u64, _up] + _err),
    "ptr_debug_exact_division": (_int, [_u32, _up, _u64, _up]),
    "ptr_debug_shade_kernel_set": (_int, [_vp, _settings, _int, _up]),
    "ptr_debug_render_multi_on": (_int, [_desc, _settings, _u32, C.POINTER(_int), _int, _fp, _stats] + _err),
    "ptr_debug_env_distribution": (_int, [_fp, _u32, _u32, _fp, _up, _fp, _up, _fp, _fp]),
    "ptr_debug_scene_geometry": (_int, [_desc, _u32, _u64p] + _err),
    "ptr_debug_generate_tangents": (_int, [_fp, _fp, _fp, _u64, _fp]),
}
DEBUG_SYMBOLS = tuple(name for name in _SIGNATURES if name.startswith("ptr_debug_"))
ABI_SYMBOLS = tuple(name for name in _SIGNATURES if name not in DEBUG_SYMBOLS)

# ... of include/ptr_debug_pbr.h (the per-hit material probe), a table of its own: tests/test_pbr_hit_host.py holds it against that header
_PBR_HIT_SIGNATURES = {
    "ptr_debug_pbr_hits": (_int, [_vp, _fp, _u64, _fp] + _err),
}
PBR_HIT_SYMBOLS = tuple(_PBR_HIT_SIGNATURES)

# ... of include/ptr_debug_sss.h (the random-walk subsurface probes), a table of its own: tests/test_sss_walk_host.py holds it against that header
_SSS_WALK_SIGNATURES = {
    "ptr_debug_sss_walk_begin": (_int, [_material, _settings, _fp, _up, _u64, _fp, _up] + _err),
    "ptr_debug_sss_walk_step": (_int, [_material, _settings, _fp, _up, _u64, _fp, _up] + _err),
    "ptr_debug_sss_walks": (_int, [_vp, _settings, _up, _u64, _u32, _fp, _fp] + _err),
}
SSS_WALK_SYMBOLS = tuple(_SSS_WALK_SIGNATURES)
# columns of their rows (the oracle's oracle_sss_* report the same rows); "u:" marks a uint32 word
SSS_BEGIN_FIELDS = {"outcome": 0, "direction": slice(1, 4), "weight": slice(4, 7), "pdf": 7, "is_delta": 8, "position": slice(9, 12)}
SSS_STEP_IN_FIELDS = {"position": slice(0, 3), "direction": slice(3, 6), "throughput": slice(6, 9), "u:step": 9, "hit": 10, "t": 11,
                      "point": slice(12, 15), "normal": slice(15, 18)}
SSS_STEP_FIELDS = {"outcome": 0, "position": slice(1, 4), "direction": slice(4, 7), "throughput": slice(7, 10), "u:step": 10,
                   "exit_direction": slice(11, 14), "exit_weight": slice(14, 17), "exit_pdf": 17, "has_exit": 18, "exit_point": slice(19, 22)}
SSS_WALK_STEP_FIELDS = dict(SSS_STEP_IN_FIELDS, **{"u:state_before": 18, "outcome": 19, "u:state_after": 20})
SSS_WALK_FINAL_FIELDS = {"first_hit": 0, "started": 1, "queries": 2, "outcome": 3, "goes_on": 4, "next_origin": slice(5, 8),
                         "next_direction": slice(8, 11), "throughput": slice(11, 14), "u:state": 14, "escapes": 15, "unsupported": 16,
                         "parked_normal": slice(17, 20), "u:camera_state": 20}
SSS_MAX_STEPS = 64   # PTR_SSS_MAX_STEPS


def sss_fields(rows: np.ndarray, fields: dict) -> dict:
    """name -> columns of [..., k] float32 rows of the random-walk probes (a "u:" field as uint32, without the mark), and the rows themselves as "raw"."""
    words = rows.view(np.uint32)
    res = {k[2:] if k.startswith("u:") else k: (words if k.startswith("u:") else rows)[..., v] for k, v in fields.items()}
    res["raw"] = rows
    return res


# ... of include/ptr_debug_path.h (the stepping probe of the path state), a table of its own: tests/test_path_state_host.py holds it against that header
_PATH_STATE_SIGNATURES = {
    "ptr_debug_path_states": (_int, [_vp, _settings, _up, _u64, _u32, _u32, _up, _up, _fp] + _err),
}
PATH_STATE_SYMBOLS = tuple(_PATH_STATE_SIGNATURES)
PATH_STATE_WORDS = 48   # PTR_PATH_STATE_WORDS
# words of a slot's snapshot; "u:" marks a uint32 word
PATH_STATE_FIELDS = {"origin": slice(0, 3), "direction": slice(3, 6), "last_pdf": 6, "u:flags": 7, "t": 8, "u:hit_word": 9, "throughput": slice(10, 13),
                     "u:rng": 13, "accum": slice(14, 17), "u:item": 17, "u:medium": slice(18, 22), "cone": slice(22, 24), "u:record_kind": slice(24, 29),
                     "u:flush_item": 29, "record_value": slice(32, 47)}


# ... and of include/ptr_post.h (the denoiser), a table of its own: tests/test_post_host.py holds it against that header
_denoise = C.POINTER(PtrDenoiseParams)
_POST_SIGNATURES = {
    "ptr_denoise_default_params": (None, [_denoise]),
    "ptr_denoise": (_int, [_fp, _fp, _fp, _u32, _u32, _denoise, _int, _fp, C.POINTER(C.c_double)] + _err),
    "ptr_denoise_device": (_int, [_vp, _vp, _vp, _u32, _u32, _denoise, _vp, _vp] + _err),
    "ptr_denoise_timed": (_int, [_vp, _vp, _vp, _u32, _u32, _denoise, _vp, _u32, _u32, C.POINTER(C.c_double), _up] + _err),
}
POST_SYMBOLS = tuple(_POST_SIGNATURES)

# ... and of include/ptr_stats.h (per-pixel sample covariance), again a table of its own: tests/test_stats_host.py holds it against that header
_STATS_SIGNATURES = {
    "ptr_render_bands_cov_device": (_int, [_vp, _settings, _u32, _u32, _u32, _vp, _vp, _vp, _int, _stats] + _err),
    "ptr_render_bands_cov": (_int, [_vp, _settings, _u32, _u32, _u32, _fp, _fp, _int, _stats] + _err),
    "ptr_denoise_cov": (_int, [_fp, _fp, _fp, _fp, _u32, _u32, _denoise, _int, _fp, C.POINTER(C.c_double)] + _err),
    "ptr_denoise_cov_device": (_int, [_vp, _vp, _vp, _vp, _u32, _u32, _denoise, _vp, _vp] + _err),
    "ptr_stats_debug_samples": (_int, [_vp, _settings, _u32, _fp] + _err),
}
STATS_SYMBOLS = tuple(_STATS_SIGNATURES)

# ... and of include/ptr_adaptive.h (adaptive sampling): tests/test_adaptive_host.py holds it against that header
_adaptive, _adaptive_info = C.POINTER(PtrAdaptiveParams), C.POINTER(PtrAdaptiveInfo)
_ADAPTIVE_SIGNATURES = {
    "ptr_adaptive_default_params": (None, [_adaptive, _u32]),
    "ptr_render_adaptive_device": (_int, [_vp, _settings, _adaptive, _vp, _vp, _vp, _vp, _stats, _adaptive_info] + _err),
    "ptr_render_adaptive": (_int, [_vp, _settings, _adaptive, _fp, _fp, _up, _stats, _adaptive_info] + _err),
    "ptr_adaptive_debug_round": (_int, [_u32, _u32, _adaptive, _u32, _u32, _int, _up, _u32, _fp, _fp, _fp, _fp, _up, _fp, _up, _up] + _err),
}
ADAPTIVE_SYMBOLS = tuple(_ADAPTIVE_SIGNATURES)

# ... and of include/ptr_multi.h (covariance and adaptive sampling on several devices): tests/test_multi_host.py holds it against that header
_multi_info, _ids = C.POINTER(PtrMultiInfo), C.POINTER(_int)
_MULTI_SIGNATURES = {
    "ptr_render_multi_cov": (_int, [_desc, _settings, _u32, _int, _int, _fp, _fp, _fp, _fp, _stats, _multi_info] + _err),
    "ptr_render_multi_adaptive": (_int, [_desc, _settings, _adaptive, _int, _int, _fp, _fp, _up, _fp, _fp, _stats, _adaptive_info, _multi_info] + _err),
    "ptr_multi_debug_cov_on": (_int, [_desc, _settings, _u32, _ids, _int, _fp, _fp, _fp, _fp, _stats, _multi_info] + _err),
    "ptr_multi_debug_adaptive_on": (_int, [_desc, _settings, _adaptive, _ids, _int, _fp, _fp, _up, _fp, _fp, _stats, _adaptive_info, _multi_info] + _err),
    "ptr_multi_debug_adaptive_frame": (_int, [_u32, _u32, _adaptive, _fp, _ids, _int, _fp, _fp, _up, _adaptive_info] + _err),
}
MULTI_SYMBOLS = tuple(_MULTI_SIGNATURES)



class PtrFrameInfo(C.Structure):
    """include/ptr_frame.h PtrFrameInfo."""
    _fields_ = [
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("minCount", C.c_uint32),
        ("maxCount", C.c_uint32),
        ("totalSamples", C.c_uint64),
        ("uniform", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


# ... and of include/ptr_frame.h (resumable frames): tests/test_frame_host.py holds it against that header
_frame_info = C.POINTER(PtrFrameInfo)
_FRAME_SIGNATURES = {
    "ptr_frame_create": (_int, [_vp, _settings, C.POINTER(_vp)] + _err),
    "ptr_frame_release": (None, [_vp]),
    "ptr_frame_reset": (_int, [_vp, _settings] + _err),
    "ptr_frame_accumulate": (_int, [_vp, _u32, _vp, _stats] + _err),
    "ptr_frame_refine": (_int, [_vp, _adaptive, _vp, _stats, _adaptive_info] + _err),
    "ptr_frame_resolve_device": (_int, [_vp, _vp, _vp, _vp, _vp] + _err),
    "ptr_frame_resolve": (_int, [_vp, _fp, _fp, _up] + _err),
    "ptr_frame_info": (_int, [_vp, _frame_info]),
    "ptr_frame_export": (_int, [_vp, _fp, _fp, _fp, _up, _fp] + _err),
    "ptr_frame_import": (_int, [_vp, _fp, _fp, _fp, _up, _fp] + _err),
    "ptr_frame_debug_create": (_int, [_u32, _u32, _fp, _u32, _int, C.POINTER(_vp)] + _err),
}
FRAME_SYMBOLS = tuple(_FRAME_SIGNATURES)

# ... and of include/ptr_multi_frame.h (resumable frames on several devices): tests/test_multi_frame_host.py holds it against that header
_MULTI_FRAME_SIGNATURES = {
    "ptr_multi_frame_create": (_int, [_desc, _settings, _int, C.POINTER(_vp)] + _err),
    "ptr_multi_frame_release": (None, [_vp]),
    "ptr_multi_frame_reset": (_int, [_vp, _settings] + _err),
    "ptr_multi_frame_accumulate": (_int, [_vp, _u32, _stats] + _err),
    "ptr_multi_frame_refine": (_int, [_vp, _adaptive, _stats, _adaptive_info] + _err),
    "ptr_multi_frame_resolve": (_int, [_vp, _fp, _fp, _up, _fp, _fp] + _err),
    "ptr_multi_frame_resolve_device": (_int, [_vp, _vp, _vp, _vp, _vp] + _err),
    "ptr_multi_frame_info": (_int, [_vp, _frame_info, _multi_info]),
    "ptr_multi_frame_export": (_int, [_vp, _fp, _fp, _fp, _up, _fp] + _err),
    "ptr_multi_frame_import": (_int, [_vp, _fp, _fp, _fp, _up, _fp] + _err),
    "ptr_multi_frame_debug_create_on": (_int, [_desc, _settings, _ids, _int, C.POINTER(_vp)] + _err),
    "ptr_multi_frame_debug_create": (_int, [_u32, _u32, _fp, _u32, _ids, _int, C.POINTER(_vp)] + _err),
}
MULTI_FRAME_SYMBOLS = tuple(_MULTI_FRAME_SIGNATURES)



class PtrMeshTransform(C.Structure):
    """include/ptr_dynamic.h PtrMeshTransform."""
    _fields_ = [("meshIndex", C.c_uint32), ("pad", C.c_uint32), ("localToWorld", C.c_float * 16)]


class PtrUpdateInfo(C.Structure):
    """include/ptr_dynamic.h PtrUpdateInfo."""
    _fields_ = [
        ("totalSeconds", C.c_double),
        ("bakeMs", C.c_double),
        ("refitMs", C.c_double),
        ("quantiseMs", C.c_double),
        ("wideMs", C.c_double),
        ("trianglesMoved", C.c_uint64),
        ("nodes", C.c_uint64),
        ("levels", C.c_uint64),
        ("wideNodes", C.c_uint64),
        ("sceneLo", C.c_float * 3),
        ("sceneHi", C.c_float * 3),
        ("gridOrigin", C.c_float * 3),
        ("gridCell", C.c_float * 3),
        ("cellOverExtent", C.c_float),
        ("pad", C.c_uint32),
    ]

    def as_dict(self) -> dict:
        return {name: (list(getattr(self, name)) if hasattr(getattr(self, name), "__len__") else getattr(self, name))
                for name, _ in self._fields_ if name != "pad"}


# ... and of include/ptr_dynamic.h (dynamic scenes): tests/test_dynamic_host.py holds it against that header
_DYNAMIC_SIGNATURES = {
    "ptr_scene_upload_dynamic": (_int, [_desc, _int, C.POINTER(_vp)] + _err),
    "ptr_scene_set_mesh_transforms": (_int, [_vp, C.POINTER(PtrMeshTransform), _u32, _vp, C.POINTER(PtrUpdateInfo)] + _err),
    "ptr_scene_is_dynamic": (_int, [_vp]),
    # its test-only probes
    "ptr_debug_scene_arrays": (_int, [_vp, _u32, _vp, _u64, _u64p]),
    "ptr_debug_dynamic_tables": (_int, [_desc, _u32, _vp, _u64, _u64p] + _err),
}
DYNAMIC_SYMBOLS = tuple(_DYNAMIC_SIGNATURES)

# ... and of include/ptr_deform.h (deforming meshes, moving spheres and rectangles): tests/test_dynamic_deform_host.py holds it against that header
PTR_DYNAMIC_DEFORMABLE = 1
PTR_DYNAMIC_PRIMITIVES = 2


class PtrMeshVertices(C.Structure):
    """include/ptr_deform.h PtrMeshVertices."""
    _fields_ = [("meshIndex", C.c_uint32), ("vertexCount", C.c_uint32), ("positions", C.POINTER(C.c_float)), ("normals", C.POINTER(C.c_float)),
                ("tangents", C.POINTER(C.c_float))]


class PtrSphereUpdate(C.Structure):
    """include/ptr_deform.h PtrSphereUpdate."""
    _fields_ = [("sphereIndex", C.c_uint32), ("pad", C.c_uint32 * 3), ("centerRadius", C.c_float * 4)]


class PtrRectUpdate(C.Structure):
    """include/ptr_deform.h PtrRectUpdate."""
    _fields_ = [("rectIndex", C.c_uint32), ("pad", C.c_uint32 * 3), ("corner", C.c_float * 4), ("edgeU", C.c_float * 4), ("edgeV", C.c_float * 4),
                ("normalAndPlane", C.c_float * 4)]


_DEFORM_SIGNATURES = {
    "ptr_scene_upload_dynamic_ex": (_int, [_desc, _int, _u32, C.POINTER(_vp)] + _err),
    "ptr_scene_dynamic_flags": (_u32, [_vp]),
    "ptr_scene_set_mesh_vertices": (_int, [_vp, C.POINTER(PtrMeshVertices), _u32, _vp, C.POINTER(PtrUpdateInfo)] + _err),
    "ptr_scene_set_spheres": (_int, [_vp, C.POINTER(PtrSphereUpdate), _u32, _vp, C.POINTER(PtrUpdateInfo)] + _err),
    "ptr_scene_set_rects": (_int, [_vp, C.POINTER(PtrRectUpdate), _u32, _vp, C.POINTER(PtrUpdateInfo)] + _err),
    # its test-only probe
    "ptr_debug_dynamic_update_rows": (_int, [_desc, _u32, _vp, _vp, _u64, _u64p] + _err),
}
DEFORM_SYMBOLS = tuple(_DEFORM_SIGNATURES)
# ptr_debug_dynamic_update_rows: the arrays a destination word names, (array << 28) | row
SCATTER_ARRAYS = ("tris", "triNormals", "triBounds", "spheres", "sphereBounds", "rects", "rectLights")

# ... and of include/ptr_deform_device.h (deforming meshes from device-resident arrays, vertex normals on the device):
# tests/test_deform_device_host.py holds it against that header
PTR_DYNAMIC_VERTEX_NORMALS = 4


class PtrMeshVerticesDevice(C.Structure):
    """include/ptr_deform_device.h PtrMeshVerticesDevice: the pointers are device addresses."""
    _fields_ = [("meshIndex", C.c_uint32), ("vertexCount", C.c_uint32), ("positions", C.c_void_p), ("normals", C.c_void_p), ("tangents", C.c_void_p)]


_DEFORM_DEVICE_SIGNATURES = {
    "ptr_scene_upload_deformable": (_int, [_desc, _int, _u32, C.POINTER(_vp)] + _err),
    "ptr_scene_set_mesh_vertices_device": (_int, [_vp, C.POINTER(PtrMeshVerticesDevice), _u32, _vp, C.POINTER(PtrUpdateInfo)] + _err),
    # its test-only probe
    "ptr_debug_vertex_adjacency": (_int, [_desc, _u32, _vp, _u64, _u64p] + _err),
}
DEFORM_DEVICE_SYMBOLS = tuple(_DEFORM_DEVICE_SIGNATURES)

# ... and of include/ptr_background.h (the primary-ray bounds cull): tests/test_background_cull_host.py holds it against that header
_BACKGROUND_SIGNATURES = {
    "ptr_background_debug_cull": (_int, [_vp, _desc, _settings, _u32, _u32, _int, _up, C.POINTER(C.c_double)] + _err),
}
BACKGROUND_SYMBOLS = tuple(_BACKGROUND_SIGNATURES)

# ... and of include/ptr_temporal.h (temporal accumulation for sequences): tests/test_temporal_host.py holds it against that header
class PtrTemporalParams(C.Structure):
    """include/ptr_temporal.h PtrTemporalParams; PtrTemporalParams.defaults() asks the library for its defaults."""
    _fields_ = [("maxHistory", C.c_uint32), ("normalCos", C.c_float), ("planeTolerance", C.c_float), ("flags", C.c_uint32)]

    @classmethod
    def defaults(cls, **overrides) -> "PtrTemporalParams":
        p = cls()
        load_library().ptr_temporal_default_params(C.byref(p))
        for k, v in overrides.items():
            setattr(p, k, v)
        return p


class PtrTemporalInfo(C.Structure):
    """include/ptr_temporal.h PtrTemporalInfo."""
    _fields_ = [("frameIndex", C.c_uint32), ("hadHistory", C.c_uint32), ("surfaceMs", C.c_double), ("accumulateMs", C.c_double),
                ("snapshotMs", C.c_double)]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_}


_temporal, _temporal_info = C.POINTER(PtrTemporalParams), C.POINTER(PtrTemporalInfo)
_TEMPORAL_SIGNATURES = {
    "ptr_temporal_default_params": (None, [_temporal]),
    "ptr_temporal_check_params": (_int, [_temporal] + _err),
    "ptr_temporal_create": (_int, [_vp, _u32, _u32, _temporal, C.POINTER(_vp)] + _err),
    "ptr_temporal_release": (None, [_vp]),
    "ptr_temporal_reset": (_int, [_vp]),
    "ptr_temporal_step_device": (_int, [_vp, _settings, _vp, _vp, _vp, _vp, _vp, _vp, _temporal_info] + _err),
    "ptr_temporal_step": (_int, [_vp, _settings, _fp, _fp, _fp, _fp, _fp, _temporal_info] + _err),
    # its test-only probes
    "ptr_debug_temporal_accumulate": (_int, [_u32, _u32, _temporal, _int, _fp, _fp, _fp, _fp, _fp, _fp, _int, _fp, _fp, _fp] + _err),
    "ptr_debug_temporal_records": (_int, [_vp, _fp, _fp, _fp] + _err),
    "ptr_debug_temporal_camera": (_int, [_settings, _fp]),
}
TEMPORAL_SYMBOLS = tuple(_TEMPORAL_SIGNATURES)


# ... and of include/ptr_temporal_cov.h (the same handle carrying the covariance of its colour): tests/test_temporal_cov_host.py
class PtrTemporalCovParams(C.Structure):
    """include/ptr_temporal_cov.h PtrTemporalCovParams; PtrTemporalCovParams.defaults() asks the library for its defaults."""
    _fields_ = [("rejectSigma", C.c_float), ("flags", C.c_uint32)]

    @classmethod
    def defaults(cls, **overrides) -> "PtrTemporalCovParams":
        p = cls()
        load_library().ptr_temporal_cov_default_params(C.byref(p))
        for k, v in overrides.items():
            setattr(p, k, v)
        return p


_temporal_cov = C.POINTER(PtrTemporalCovParams)
_TEMPORAL_COV_SIGNATURES = {
    "ptr_temporal_cov_default_params": (None, [_temporal_cov]),
    "ptr_temporal_cov_check_params": (_int, [_temporal_cov] + _err),
    "ptr_temporal_create_cov": (_int, [_vp, _u32, _u32, _temporal, _temporal_cov, C.POINTER(_vp)] + _err),
    "ptr_temporal_step_cov_device": (_int, [_vp, _settings, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _temporal_info] + _err),
    "ptr_temporal_step_cov": (_int, [_vp, _settings, _fp, _fp, _fp, _fp, _fp, _fp, _fp, _temporal_info] + _err),
    # its test-only probe
    "ptr_debug_temporal_accumulate_cov": (_int, [_u32, _u32, _temporal, _temporal_cov, _int] + [_fp] * 8 + [_int] + [_fp] * 5 + _err),
}
TEMPORAL_COV_SYMBOLS = tuple(_TEMPORAL_COV_SIGNATURES)

PTR_REBUILD_KEEP_IF_BETTER = 1


class PtrRebuildInfo(C.Structure):
    """include/ptr_rebuild.h PtrRebuildInfo."""
    _fields_ = [
        ("totalSeconds", C.c_double),
        ("costBefore", C.c_double),
        ("costAfter", C.c_double),
        ("keysSortMs", C.c_double),
        ("topologyMs", C.c_double),
        ("fitMs", C.c_double),
        ("quantiseMs", C.c_double),
        ("wideMs", C.c_double),
        ("nodes", C.c_uint64),
        ("levels", C.c_uint64),
        ("wideNodes", C.c_uint64),
        ("wideDepth", C.c_uint64),
        ("leaves", C.c_uint64),
        ("installed", C.c_uint32),
        ("pad", C.c_uint32),
    ]

    def as_dict(self) -> dict:
        return {name: getattr(self, name) for name, _ in self._fields_ if name != "pad"}


# ... and of include/ptr_rebuild.h (tree cost and the rebuild above the leaves): tests/test_rebuild_host.py holds it against that header
_REBUILD_SIGNATURES = {
    "ptr_scene_tree_cost": (_int, [_vp, _vp, C.POINTER(C.c_double)] + _err),
    "ptr_scene_rebuild_tree": (_int, [_vp, _u32, _vp, C.POINTER(PtrRebuildInfo)] + _err),
    # its test-only probes
    "ptr_debug_rebuild_arrays": (_int, [_vp, _u32, _vp, _u64, _u64p]),
    "ptr_debug_rebuild_tables": (_int, [_fp, _u32, _u32, _vp, _u64, _u64p] + _err),
}
REBUILD_SYMBOLS = tuple(_REBUILD_SIGNATURES)
# ptr_debug_rebuild_arrays / ptr_debug_rebuild_tables: name -> (selector, dtype, trailing shape)
REBUILD_ARRAYS = {"schedule": (0, np.uint32, ()), "levelOffsets": (1, np.uint32, ()), "wideSource": (2, np.uint32, (4,)), "info": (3, np.uint32, ()),
                  "leafTable": (4, np.uint32, ()), "pointers": (5, np.uint64, ())}
REBUILD_ARRAY_INFO = ("nodes", "levels", "wide_nodes", "wide_depth", "stack_limit", "leaves")
REBUILD_TABLES = {"schedule": (0, np.uint32, ()), "levelOffsets": (1, np.uint32, ()), "grid": (2, np.float32, (3,)), "qnodes": (3, np.uint32, (2, 4)),
                  "wnodes": (4, np.uint32, (4, 4)), "wideSource": (5, np.uint32, (4,)), "wideDepth": (6, np.uint32, ()), "sah": (7, np.float64, ()),
                  "leafTable": (8, np.uint32, ()), "depthCheck": (9, np.uint32, ())}


class PtrMultiUpdateInfo(C.Structure):
    """include/ptr_multi_dynamic.h PtrMultiUpdateInfo."""
    _fields_ = [("parts", C.c_uint32), ("stagedParts", C.c_uint32), ("totalSeconds", C.c_double), ("distributeSeconds", C.c_double),
                ("partSeconds", C.c_double * MULTI_MAX_PARTS), ("first", PtrUpdateInfo)]

    def as_dict(self) -> dict:
        """PtrUpdateInfo of partition 0 as DeviceScene's update calls return it, with the figures of the fan-out beside it."""
        out = self.first.as_dict()
        out.update(parts=int(self.parts), stagedParts=int(self.stagedParts), totalSeconds=self.totalSeconds, distributeSeconds=self.distributeSeconds,
                   partSeconds=list(self.partSeconds[:self.parts]), partTotalSeconds=self.first.totalSeconds)
        return out


# ... and of include/ptr_multi_dynamic.h (dynamic scenes on several devices): tests/test_multi_dynamic_host.py holds it against that header
_multi_update = C.POINTER(PtrMultiUpdateInfo)
_MULTI_DYNAMIC_SIGNATURES = {
    "ptr_multi_frame_create_dynamic": (_int, [_desc, _settings, _int, _u32, C.POINTER(_vp)] + _err),
    "ptr_multi_frame_debug_create_dynamic_on": (_int, [_desc, _settings, _u32, _ids, _int, C.POINTER(_vp)] + _err),
    "ptr_multi_frame_is_dynamic": (_int, [_vp]),
    "ptr_multi_frame_dynamic_flags": (_u32, [_vp]),
    "ptr_multi_frame_set_mesh_transforms": (_int, [_vp, C.POINTER(PtrMeshTransform), _u32, _multi_update] + _err),
    "ptr_multi_frame_set_mesh_vertices": (_int, [_vp, C.POINTER(PtrMeshVertices), _u32, _multi_update] + _err),
    "ptr_multi_frame_set_spheres": (_int, [_vp, C.POINTER(PtrSphereUpdate), _u32, _multi_update] + _err),
    "ptr_multi_frame_set_rects": (_int, [_vp, C.POINTER(PtrRectUpdate), _u32, _multi_update] + _err),
    "ptr_multi_frame_set_mesh_vertices_device": (_int, [_vp, C.POINTER(PtrMeshVerticesDevice), _u32, _int, _vp, _multi_update] + _err),
    "ptr_multi_frame_tree_cost": (_int, [_vp, C.POINTER(C.c_double)] + _err),
    "ptr_multi_frame_rebuild_tree": (_int, [_vp, _u32, C.POINTER(PtrRebuildInfo)] + _err),
    "ptr_multi_frame_part_scene": (_vp, [_vp, _u32]),
    # its test-only probe
    "ptr_multi_frame_debug_check_update": (_int, [_desc, _u32, _u32, _vp, _u32] + _err),
}
MULTI_DYNAMIC_SYMBOLS = tuple(_MULTI_DYNAMIC_SIGNATURES)


# ... and of include/ptr_appearance.h (materials, textures and the environment of a resident scene): tests/test_appearance_host.py holds
# it against that header
PTR_APPEARANCE_ENV_MAX_DIM = 4096


class PtrAppearanceInfo(C.Structure):
    """include/ptr_appearance.h PtrAppearanceInfo."""
    _fields_ = [
        ("totalSeconds", C.c_double),
        ("stagingMs", C.c_double),
        ("kernelMs", C.c_double * 6),
        ("rowsRekeyed", C.c_uint64),
        ("texelsWritten", C.c_uint64),
        ("lightsBefore", C.c_uint32),
        ("lightsAfter", C.c_uint32),
        ("envSampling", C.c_uint32),
        ("pad", C.c_uint32),
    ]

    def as_dict(self) -> dict:
        return {name: (list(getattr(self, name)) if hasattr(getattr(self, name), "__len__") else getattr(self, name))
                for name, _ in self._fields_ if name != "pad"}


class PtrTextureUpdate(C.Structure):
    """include/ptr_appearance.h PtrTextureUpdate: rgba is a host address for set_textures, a device address for set_textures_device."""
    _fields_ = [("textureIndex", C.c_uint32), ("width", C.c_uint32), ("height", C.c_uint32), ("wrapS", C.c_uint32), ("wrapT", C.c_uint32),
                ("filter", C.c_uint32), ("rgba", C.c_void_p)]


_appearance_info = C.POINTER(PtrAppearanceInfo)
_APPEARANCE_SIGNATURES = {
    "ptr_scene_set_materials": (_int, [_vp, _up, _material, _u32, _vp, _appearance_info] + _err),
    "ptr_scene_set_textures": (_int, [_vp, C.POINTER(PtrTextureUpdate), _u32, _vp, _appearance_info] + _err),
    "ptr_scene_set_textures_device": (_int, [_vp, C.POINTER(PtrTextureUpdate), _u32, _vp, _appearance_info] + _err),
    "ptr_scene_set_environment": (_int, [_vp, _vp, _u32, _u32, _vp, _appearance_info] + _err),
    "ptr_scene_set_environment_device": (_int, [_vp, _vp, _u32, _u32, _vp, _appearance_info] + _err),
    # its test-only probe
    "ptr_debug_appearance_arrays": (_int, [_vp, _u32, _vp, _u64, _u64p]),
}
APPEARANCE_SYMBOLS = tuple(_APPEARANCE_SIGNATURES)


class PtrMultiAppearanceInfo(C.Structure):
    """include/ptr_multi_appearance.h PtrMultiAppearanceInfo."""
    _fields_ = [("parts", C.c_uint32), ("stagedParts", C.c_uint32), ("hostStagedBytes", C.c_uint64), ("totalSeconds", C.c_double),
                ("distributeSeconds", C.c_double), ("partSeconds", C.c_double * MULTI_MAX_PARTS), ("first", PtrAppearanceInfo)]

    def as_dict(self) -> dict:
        """PtrAppearanceInfo of partition 0 as DeviceScene's appearance calls return it, with the figures of the fan-out beside it."""
        out = self.first.as_dict()
        out.update(parts=int(self.parts), stagedParts=int(self.stagedParts), hostStagedBytes=int(self.hostStagedBytes), totalSeconds=self.totalSeconds,
                   distributeSeconds=self.distributeSeconds, partSeconds=list(self.partSeconds[:self.parts]), partTotalSeconds=self.first.totalSeconds)
        return out


# ... and of include/ptr_multi_appearance.h (the same calls on a frame on several devices): tests/test_multi_appearance_host.py holds it
# against that header.  (MULTI_APPEARANCE_FUNCTIONS, not ..._SYMBOLS: tests/test_appearance_host.py holds the set of *_SYMBOLS tables fixed.)
_multi_appearance = C.POINTER(PtrMultiAppearanceInfo)
_MULTI_APPEARANCE_SIGNATURES = {
    "ptr_multi_frame_set_materials": (_int, [_vp, _up, _material, _u32, _multi_appearance] + _err),
    "ptr_multi_frame_set_textures": (_int, [_vp, C.POINTER(PtrTextureUpdate), _u32, _multi_appearance] + _err),
    "ptr_multi_frame_set_environment": (_int, [_vp, _vp, _u32, _u32, _multi_appearance] + _err),
    "ptr_multi_frame_set_textures_device": (_int, [_vp, C.POINTER(PtrTextureUpdate), _u32, _int, _vp, _multi_appearance] + _err),
    "ptr_multi_frame_set_environment_device": (_int, [_vp, _vp, _u32, _u32, _int, _vp, _multi_appearance] + _err),
    # its test-only probe
    "ptr_multi_frame_debug_check_appearance": (_int, [_desc, _u32, _u32, _vp, _material, _u32, _u32, _u32] + _err),
}
MULTI_APPEARANCE_FUNCTIONS = tuple(_MULTI_APPEARANCE_SIGNATURES)
# ptr_debug_appearance_arrays: name -> (selector, dtype, trailing shape).  Words that hold bit patterns beside floats (texture indices,
# alias entries) are read as uint32, so comparisons are of the raw words.
APPEARANCE_ARRAYS = {"materials": (0, np.uint32, (16, 4)), "materialTex": (1, np.uint32, (16, 4)), "rectLights": (2, np.uint32, (11, 4)),
                     "lightIndexByRect": (3, np.int32, ()), "texels": (4, np.uint32, (4,)), "texInfo": (5, np.uint32, (20,)),
                     "envRgba": (6, np.uint32, (4,)), "envCond": (7, np.uint32, (2,)), "envMarg": (8, np.uint32, (2,)), "envPdf": (9, np.uint32, ()),
                     "envMips": (10, np.uint32, (4,)), "scalars": (11, np.uint32, ())}
APPEARANCE_SCALARS = ("materialTypes", "rectLightCount", "settleRectLights", "hasRandomWalkMaterial", "envSampling", "envMipLevels")

# ptr_debug_scene_arrays / ptr_debug_dynamic_tables: name -> (selector, dtype, trailing shape)
SCENE_ARRAYS = {"tris": (0, np.float32, (3, 4)), "triNormals": (1, np.float32, (3, 4)), "triUv": (2, np.float32, (4, 4)),
                "triTangent": (3, np.float32, (3, 4)), "triBounds": (4, np.float32, (2, 4)), "sphereBounds": (5, np.float32, (2, 4)),
                "boxes": (6, np.float32, (4, 4)), "qnodes": (7, np.uint32, (2, 4)), "wnodes": (8, np.uint32, (4, 4)), "grid": (9, np.float32, (3,)),
                "rects": (10, np.float32, (5, 4)), "rectLights": (11, np.float32, (11, 4)), "spheres": (12, np.float32, (4,)),
                "objPos": (13, np.float32, (3, 4)), "objNrm": (14, np.float32, (3, 4)), "objTan": (15, np.float32, (3, 4))}
DYNAMIC_TABLES = {"nodes": (0, np.float32, (4, 4)), "qnodes": (1, np.uint32, (2, 4)), "wnodes": (2, np.uint32, (4, 4)),
                  "triBounds": (3, np.float32, (2, 4)), "sphereBounds": (4, np.float32, (2, 4)), "schedule": (5, np.uint32, ()),
                  "levelOffsets": (6, np.uint32, ()), "wideSource": (7, np.uint32, (4,)), "grid": (8, np.float32, (3,)),
                  "requantised": (9, np.uint32, (2, 4)), "meshTriOffsets": (10, np.uint32, ()), "meshTris": (11, np.uint32, ()),
                  "info": (12, np.uint32, ()), "meshCorners": (13, np.uint32, (3,)), "rectTriLeaf": (14, np.uint32, (2,)),
                  "sphereLeaf": (15, np.uint32, ()), "tris": (16, np.float32, (3, 4)), "triNormals": (17, np.float32, (3, 4)),
                  "spheres": (18, np.float32, (4,)), "rects": (19, np.float32, (5, 4)), "rectLights": (20, np.float32, (11, 4))}
DYNAMIC_TABLE_INFO = ("nodes", "levels", "wide_nodes", "quantized", "triangles", "spheres", "max_depth", "root_ref", "oversize_ref", "wide_depth")

_lib: Optional[C.CDLL] = None


class PtrError(RuntimeError):
    pass


def load_library() -> C.CDLL:
    """Load libptr_hip.so (built in-tree by __graft_entry__.build()).  No fallback: raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    path = os.environ.get("PTR_HIP_LIBRARY", LIB_PATH)   # override: A/B builds of the same library (tools/)
    if not os.path.exists(path):
        raise PtrError(f"{path} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` first")
    lib = C.CDLL(path)
    for name, (restype, argtypes) in list(_SIGNATURES.items()) + list(_POST_SIGNATURES.items()) + list(_STATS_SIGNATURES.items()) + \
            list(_ADAPTIVE_SIGNATURES.items()) + list(_MULTI_SIGNATURES.items()) + list(_FRAME_SIGNATURES.items()) + list(_MULTI_FRAME_SIGNATURES.items()) + \
            list(_DYNAMIC_SIGNATURES.items()) + list(_DEFORM_SIGNATURES.items()) + list(_DEFORM_DEVICE_SIGNATURES.items()) + \
            list(_BACKGROUND_SIGNATURES.items()) + list(_TEMPORAL_SIGNATURES.items()) + list(_TEMPORAL_COV_SIGNATURES.items()) + list(_PBR_HIT_SIGNATURES.items()) + \
            list(_SSS_WALK_SIGNATURES.items()) + list(_PATH_STATE_SIGNATURES.items()) + list(_REBUILD_SIGNATURES.items()) + list(_MULTI_DYNAMIC_SIGNATURES.items()) + \
            list(_APPEARANCE_SIGNATURES.items()) + list(_MULTI_APPEARANCE_SIGNATURES.items()):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


def _err_buf():
    return C.create_string_buffer(1024)


def _check(rc: int, err) -> None:
    if rc != 0:
        raise PtrError(err.value.decode("utf-8", "replace") or f"libptr_hip call failed ({rc})")


def _fptr(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _uptr(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def _batch(fn, lead, inp, dtype, cols, outs, more=(), tail=()):
    """The batch pattern of the probes, fn(*lead, in, *more, n, *out, *tail, err, err_cap): `inp` as a contiguous [n, cols] array of
    `dtype` (float32 or uint32) and one zeroed [n, *shape] array per (shape, dtype) of `outs`.  Returns the output array or arrays."""
    ptr = lambda a: _uptr(a) if a.dtype == np.uint32 else _fptr(a)
    inp = np.ascontiguousarray(inp, dtype=dtype).reshape(-1, cols)
    res = [np.zeros((inp.shape[0],) + shape, dtype=dt) for shape, dt in outs]
    err = _err_buf()
    _check(fn(*lead, ptr(inp), *more, inp.shape[0], *map(ptr, res), *tail, err, len(err)), err)
    return res[0] if len(res) == 1 else tuple(res)


def device_count() -> int:
    return int(load_library().ptr_device_count())


BAND_ROWS = 8   # PTR_BAND_ROWS of include/ptr_abi.h


def band_count(height: int, part: int = 0, parts: int = 1) -> int:
    return int(load_library().ptr_part_band_count(height, part, parts))


# ----------------------------------------------------------------------------- host scene layer


class HostScene:
    """A parsed `.scene` file: SceneResources arrays + RenderSettings (host memory, no GPU needed)."""

    def __init__(self, handle: C.c_void_p):
        self._h = handle
        self.desc = PtrSceneDesc()
        self.settings = PtrSettings()
        load_library().ptr_host_scene_desc(self._h, C.byref(self.desc), C.byref(self.settings))

    @classmethod
    def load(cls, scene_path: str, asset_dir: Optional[str] = None) -> "HostScene":
        lib = load_library()
        h = C.c_void_p()
        err = _err_buf()
        rc = lib.ptr_host_scene_load(os.fsencode(scene_path), os.fsencode(asset_dir) if asset_dir else None,
                                     C.byref(h), err, len(err))
        _check(rc, err)
        return cls(h)

    def settings_for(self, width: Optional[int] = None, height: Optional[int] = None, max_depth: Optional[int] = None,
                     seed: Optional[int] = None, **overrides) -> PtrSettings:
        """CLI-style overrides applied after the scene file (main_headless.mm:418-449); size defaults 1280x720."""
        s = self.settings.copy()
        if width:
            s.width = width
        if height:
            s.height = height
        if max_depth is not None:
            s.maxDepth = max_depth
        if seed is not None:
            s.seed = seed
        for k, v in overrides.items():
            setattr(s, k, v)
        if s.width == 0:
            s.width = 1280
        if s.height == 0:
            s.height = 720
        return s

    def close(self) -> None:
        if self._h:
            load_library().ptr_host_scene_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ----------------------------------------------------------------------------- device path


def prepare_geometry(desc: PtrSceneDesc, path: str) -> float:
    """Host-only: bake the scene, build the BVH and write the device-independent arrays to `path` (a file under /dev/shm) for
    DeviceScene(..., prepared=path) in this or another process.  No GPU call.  Returns the seconds it took."""
    lib = load_library()
    err = _err_buf()
    seconds = C.c_double(0.0)
    _check(lib.ptr_scene_prepare_geometry(C.byref(desc), path.encode(), C.byref(seconds), err, len(err)), err)
    return float(seconds.value)


def _transform_items(transforms: dict):
    """{mesh index: 4x4 array (row, column)} as the PtrMeshTransform list of the set_mesh_transforms calls."""
    items = (PtrMeshTransform * max(len(transforms), 1))()
    for k, (index, matrix) in enumerate(transforms.items()):
        items[k].meshIndex = int(index)
        m = np.asarray(matrix, np.float32).reshape(4, 4)
        items[k].localToWorld[:] = m.T.reshape(-1).tolist()   # column-major
    return items


def _vertex_items(meshes: dict):
    """{mesh index: (positions, normals[, tangents])} as the PtrMeshVertices list of the set_mesh_vertices calls, and the arrays it points into."""
    items = (PtrMeshVertices * max(len(meshes), 1))()
    keep = []
    fp = C.POINTER(C.c_float)
    for k, (index, data) in enumerate(meshes.items()):
        arrays = [np.ascontiguousarray(a, np.float32).reshape(-1, w) for a, w in zip(data, (3, 3, 4))]
        keep.append(arrays)
        items[k].meshIndex, items[k].vertexCount = int(index), len(arrays[0])
        items[k].positions, items[k].normals = arrays[0].ctypes.data_as(fp), arrays[1].ctypes.data_as(fp)
        items[k].tangents = arrays[2].ctypes.data_as(fp) if len(arrays) > 2 else None
    return items, keep


def _vertex_device_items(meshes: dict, scene_device: Optional[int]):
    """{mesh index: (positions, normals or None[, tangents])} of torch tensors as the PtrMeshVerticesDevice list of the
    set_mesh_vertices_device calls, and the device they are on: scene_device, or with None the one device all of them share."""
    items = (PtrMeshVerticesDevice * max(len(meshes), 1))()
    found = scene_device
    for k, (index, data) in enumerate(meshes.items()):
        data = tuple(data)
        if not 2 <= len(data) <= 3:
            raise PtrError("set_mesh_vertices_device: mesh %s needs (positions, normals or None[, tangents])" % (index,))
        for name, t, width in zip(("positions", "normals", "tangents"), data, (3, 3, 4)):
            if t is None and name == "normals":
                continue
            device = getattr(t, "device", None)
            if not hasattr(t, "data_ptr") or device is None:
                raise PtrError("set_mesh_vertices_device: the %s of mesh %s are not a torch tensor" % (name, index))
            if found is None and device.type == "cuda":
                found = device.index
            if device.type != "cuda" or device.index != found:
                where = "of the scene" if scene_device is not None else "like the arrays before them"
                raise PtrError("set_mesh_vertices_device: the %s of mesh %s are on %s, not on device %s %s" % (name, index, device, found, where))
            if str(t.dtype) != "torch.float32":
                raise PtrError("set_mesh_vertices_device: the %s of mesh %s are %s, not float32" % (name, index, t.dtype))
            if t.dim() != 2 or t.shape[1] != width or (name != "positions" and t.shape[0] != data[0].shape[0]):
                raise PtrError("set_mesh_vertices_device: the %s of mesh %s have shape %s, not [n, %d]" % (name, index, tuple(t.shape), width))
            if not t.is_contiguous():
                raise PtrError("set_mesh_vertices_device: the %s of mesh %s are not contiguous" % (name, index))
            setattr(items[k], name, t.data_ptr())
        items[k].meshIndex, items[k].vertexCount = int(index), int(data[0].shape[0])
    return items, found


def _sphere_items(spheres: dict):
    items = (PtrSphereUpdate * max(len(spheres), 1))()
    for k, (index, row) in enumerate(spheres.items()):
        items[k].sphereIndex = int(index)
        items[k].centerRadius[:] = np.asarray(row, np.float32).reshape(4).tolist()
    return items


def _rect_items(rects: dict):
    items = (PtrRectUpdate * max(len(rects), 1))()
    for k, (index, r) in enumerate(rects.items()):
        items[k] = rect_update(index, **r)
    return items


class DeviceScene:
    """A scene resident in HBM: SAH BVH + SoA primitive/material/light arrays (ptr_scene_upload)."""

    def __init__(self, desc: PtrSceneDesc, device: int = 0, keepalive=None, prepared: Optional[str] = None, dynamic: bool = False,
                 deformable: bool = False, primitives: bool = False, vertex_normals: bool = False):
        """prepared: a geometry cache written by prepare_geometry() for this description - the BVH is read, not built
        (the processes of a multi-GPU render build it once).  dynamic: ptr_scene_upload_dynamic - the scene also keeps what
        set_mesh_transforms needs to move its meshes on the device (not with `prepared`).  deformable / primitives (with dynamic):
        ptr_scene_upload_dynamic_ex with PTR_DYNAMIC_DEFORMABLE / PTR_DYNAMIC_PRIMITIVES, for set_mesh_vertices / set_spheres and set_rects.
        vertex_normals (with deformable): ptr_scene_upload_deformable with PTR_DYNAMIC_VERTEX_NORMALS as well - set_mesh_vertices_device may
        then be given positions alone."""
        lib = load_library()
        if lib.ptr_device_count() <= 0:
            raise PtrError("no HIP device visible: the HIP render path has no CPU fallback")
        self._keepalive = keepalive
        self._h = C.c_void_p()
        self._device = int(device)
        err = _err_buf()
        if dynamic and prepared:
            raise PtrError("a dynamic scene is not read from a geometry cache")
        if (deformable or primitives) and not dynamic:
            raise PtrError("deformable / primitives need dynamic=True")
        if vertex_normals and not deformable:
            raise PtrError("vertex_normals needs deformable=True")
        flags = (PTR_DYNAMIC_DEFORMABLE if deformable else 0) | (PTR_DYNAMIC_PRIMITIVES if primitives else 0)
        if vertex_normals:
            _check(lib.ptr_scene_upload_deformable(C.byref(desc), device, flags | PTR_DYNAMIC_VERTEX_NORMALS, C.byref(self._h), err, len(err)), err)
        elif deformable or primitives:
            _check(lib.ptr_scene_upload_dynamic_ex(C.byref(desc), device, flags, C.byref(self._h), err, len(err)), err)
        elif dynamic:
            _check(lib.ptr_scene_upload_dynamic(C.byref(desc), device, C.byref(self._h), err, len(err)), err)
        elif prepared:
            _check(lib.ptr_scene_upload_prepared(C.byref(desc), prepared.encode(), device, C.byref(self._h), err, len(err)), err)
        else:
            _check(lib.ptr_scene_upload(C.byref(desc), device, C.byref(self._h), err, len(err)), err)

    @property
    def is_dynamic(self) -> bool:
        return bool(load_library().ptr_scene_is_dynamic(self._h))

    def set_mesh_transforms(self, transforms: dict, stream: int = 0) -> dict:
        """ptr_scene_set_mesh_transforms: {mesh index: 4x4 array (row, column), the new localToWorld}; returns PtrUpdateInfo as a dict."""
        items = _transform_items(transforms)
        info = PtrUpdateInfo()
        err = _err_buf()
        _check(load_library().ptr_scene_set_mesh_transforms(self._h, items, len(transforms), C.c_void_p(stream), C.byref(info), err, len(err)), err)
        return info.as_dict()

    @property
    def dynamic_flags(self) -> int:
        return int(load_library().ptr_scene_dynamic_flags(self._h))

    def set_mesh_vertices(self, meshes: dict, stream: int = 0) -> dict:
        """ptr_scene_set_mesh_vertices: {mesh index: (positions [n, 3], normals [n, 3][, tangents [n, 4]])}, object space; returns
        PtrUpdateInfo as a dict."""
        items, keep = _vertex_items(meshes)
        info = PtrUpdateInfo()
        err = _err_buf()
        _check(load_library().ptr_scene_set_mesh_vertices(self._h, items, len(meshes), C.c_void_p(stream), C.byref(info), err, len(err)), err)
        return info.as_dict()

    def set_mesh_vertices_device(self, meshes: dict, stream=None) -> dict:
        """ptr_scene_set_mesh_vertices_device: {mesh index: (positions [n, 3], normals [n, 3] or None[, tangents [n, 4]])} of torch tensors
        on the scene's device, float32 and contiguous, passed by data_ptr(); None for the normals has them computed on the device (a
        scene made with vertex_normals=True).  The tensors are read on `stream` (a raw stream handle; None: torch's current stream of the
        scene's device): whatever produces them is enqueued there before the call, or has finished.  Returns PtrUpdateInfo as a dict."""
        items, _ = _vertex_device_items(meshes, self._device)
        if stream is None:
            import torch   # (only here: the module itself does not need torch)

            stream = torch.cuda.current_stream(self._device).cuda_stream
        info = PtrUpdateInfo()
        err = _err_buf()
        _check(load_library().ptr_scene_set_mesh_vertices_device(self._h, items, len(meshes), C.c_void_p(stream), C.byref(info), err, len(err)), err)
        return info.as_dict()

    def set_spheres(self, spheres: dict, stream: int = 0) -> dict:
        """ptr_scene_set_spheres: {sphere index: (cx, cy, cz, radius)}; returns PtrUpdateInfo as a dict."""
        items = _sphere_items(spheres)
        info = PtrUpdateInfo()
        err = _err_buf()
        _check(load_library().ptr_scene_set_spheres(self._h, items, len(spheres), C.c_void_p(stream), C.byref(info), err, len(err)), err)
        return info.as_dict()

    def set_rects(self, rects: dict, stream: int = 0) -> dict:
        """ptr_scene_set_rects: {rectangle index: dict(corner=, edgeU=, edgeV=, normal=)}, three components each; the w words are filled
        as the scene loader fills them (rect_update).  Returns PtrUpdateInfo as a dict."""
        items = _rect_items(rects)
        info = PtrUpdateInfo()
        err = _err_buf()
        _check(load_library().ptr_scene_set_rects(self._h, items, len(rects), C.c_void_p(stream), C.byref(info), err, len(err)), err)
        return info.as_dict()

    def _appearance_call(self, name: str, *args, stream=0) -> dict:
        info = PtrAppearanceInfo()
        err = _err_buf()
        _check(getattr(load_library(), name)(self._h, *args, C.c_void_p(stream), C.byref(info), err, len(err)), err)
        return info.as_dict()

    def _current_stream(self, stream):
        if stream is not None:
            return stream
        import torch   # (only here: the module itself does not need torch)

        return torch.cuda.current_stream(self._device).cuda_stream

    def set_materials(self, materials: dict, stream: int = 0) -> dict:
        """ptr_scene_set_materials: {material index: PtrMaterial}, each replacing the whole material; returns PtrAppearanceInfo as a dict.
        A Frame or a Temporal of the scene is not told: reset them."""
        indices, items = self._material_items(materials)
        return self._appearance_call("ptr_scene_set_materials", indices, items, len(materials), stream=stream)

    @staticmethod
    def _material_items(materials: dict):
        indices = (C.c_uint32 * max(len(materials), 1))(*[int(i) for i in materials])
        items = (PtrMaterial * max(len(materials), 1))()
        for k, m in enumerate(materials.values()):
            C.memmove(C.byref(items[k]), C.byref(m), C.sizeof(PtrMaterial))
        return indices, items

    @staticmethod
    def _texture_items(name: str, textures: dict, address):
        items = (PtrTextureUpdate * max(len(textures), 1))()
        keep = []
        for k, (index, value) in enumerate(textures.items()):
            pixels, wrap_s, wrap_t, filt = value if isinstance(value, tuple) else (value, 0, 0, 1)
            data, (h, w) = address(name, "texture %s" % (index,), pixels)
            keep.append(data)
            items[k].textureIndex, items[k].width, items[k].height = int(index), w, h
            items[k].wrapS, items[k].wrapT, items[k].filter = int(wrap_s), int(wrap_t), int(filt)
            items[k].rgba = data.data_ptr() if hasattr(data, "data_ptr") else data.ctypes.data
        return items, keep

    @staticmethod
    def _host_pixels(name: str, what: str, pixels):
        a = np.ascontiguousarray(pixels, dtype=np.float32)
        if a.ndim != 3 or a.shape[2] != 4:
            raise PtrError("%s: the pixels of %s have shape %s, not [height, width, 4]" % (name, what, a.shape))
        return a, a.shape[:2]

    def _device_pixels(self, name: str, what: str, t):
        device = getattr(t, "device", None)
        if not hasattr(t, "data_ptr") or device is None:
            raise PtrError("%s: the pixels of %s are not a torch tensor" % (name, what))
        if device.type != "cuda" or (self._device is not None and device.index != self._device):   # (None: a MultiFrame, which takes any device)
            where = "a HIP device" if self._device is None else "device %d of the scene" % self._device
            raise PtrError("%s: the pixels of %s are on %s, not on %s" % (name, what, device, where))
        if str(t.dtype) != "torch.float32":
            raise PtrError("%s: the pixels of %s are %s, not float32" % (name, what, t.dtype))
        if t.dim() != 3 or t.shape[2] != 4:
            raise PtrError("%s: the pixels of %s have shape %s, not [height, width, 4]" % (name, what, tuple(t.shape)))
        if not t.is_contiguous():
            raise PtrError("%s: the pixels of %s are not contiguous" % (name, what))
        return t, (int(t.shape[0]), int(t.shape[1]))

    def set_textures(self, textures: dict, stream: int = 0) -> dict:
        """ptr_scene_set_textures: {texture index: pixels [height, width, 4] linear float32, or (pixels, wrapS, wrapT, filter)} at the
        upload's size (pixels alone: repeat, repeat, linear); the mip chain is rebuilt on the device.  Returns PtrAppearanceInfo as a dict."""
        items, keep = self._texture_items("set_textures", textures, self._host_pixels)
        return self._appearance_call("ptr_scene_set_textures", items, len(textures), stream=stream)

    def set_textures_device(self, textures: dict, stream=None) -> dict:
        """ptr_scene_set_textures_device: set_textures from torch tensors on the scene's device (float32, contiguous), read where they are
        on `stream` (a raw stream handle; None: torch's current stream of the scene's device)."""
        items, keep = self._texture_items("set_textures_device", textures, self._device_pixels)
        return self._appearance_call("ptr_scene_set_textures_device", items, len(textures), stream=self._current_stream(stream))

    def set_environment(self, pixels, stream: int = 0) -> dict:
        """ptr_scene_set_environment: new pixels [height, width, 4] (linear float32) for the environment map at the upload's size; the
        importance tables are rebuilt on the device.  Returns PtrAppearanceInfo as a dict."""
        a, (h, w) = self._host_pixels("set_environment", "the map", pixels)
        return self._appearance_call("ptr_scene_set_environment", a.ctypes.data_as(C.c_void_p), w, h, stream=stream)

    def set_environment_device(self, pixels, stream=None) -> dict:
        """ptr_scene_set_environment_device: set_environment from a torch tensor on the scene's device, read where it is on `stream`
        (None: torch's current stream of the scene's device)."""
        t, (h, w) = self._device_pixels("set_environment_device", "the map", pixels)
        return self._appearance_call("ptr_scene_set_environment_device", C.c_void_p(t.data_ptr()), w, h, stream=self._current_stream(stream))

    def appearance_arrays(self, names=None) -> dict:
        """ptr_debug_appearance_arrays: the named arrays (all of APPEARANCE_ARRAYS by default) as raw words; "scalars" as a dict."""
        probe = load_library().ptr_debug_appearance_arrays
        out = {}
        for name in (names or APPEARANCE_ARRAYS):
            which, dtype, shape = APPEARANCE_ARRAYS[name]
            out[name] = _sized_array(lambda o, cap, size: probe(self._h, which, o, cap, size), dtype, "ptr_debug_appearance_arrays(%s)" % name).reshape((-1,) + shape)
        if "scalars" in out:
            out["scalars"] = dict(zip(APPEARANCE_SCALARS, (int(v) for v in out["scalars"])))
        return out

    def tree_cost(self, stream: int = 0) -> float:
        """ptr_scene_tree_cost: the builder's SAH figure of the scene's current tree, computed on the device in float64."""
        cost = C.c_double(0.0)
        err = _err_buf()
        _check(load_library().ptr_scene_tree_cost(self._h, C.c_void_p(stream), C.byref(cost), err, len(err)), err)
        return float(cost.value)

    def rebuild_tree(self, keep_if_better: bool = True, stream: int = 0) -> dict:
        """ptr_scene_rebuild_tree: a new tree above the upload's leaves, built on the device from the current geometry; with keep_if_better
        it is installed only when its tree_cost() is below the current tree's.  Returns PtrRebuildInfo as a dict."""
        info = PtrRebuildInfo()
        err = _err_buf()
        flags = PTR_REBUILD_KEEP_IF_BETTER if keep_if_better else 0
        _check(load_library().ptr_scene_rebuild_tree(self._h, flags, C.c_void_p(stream), C.byref(info), err, len(err)), err)
        return info.as_dict()

    def rebuild_arrays(self, names=None) -> dict:
        """ptr_debug_rebuild_arrays: the schedule, level offsets, wide-source table, leaf table and SceneView pointers of a dynamic scene as
        it is now; "info" as a dict."""
        probe = load_library().ptr_debug_rebuild_arrays
        out = {}
        for name in (names or REBUILD_ARRAYS):
            which, dtype, shape = REBUILD_ARRAYS[name]

            def ask(o, cap, size):   # (this probe's failures carry no code)
                if probe(self._h, which, o, cap, size) != 0:
                    raise PtrError("ptr_debug_rebuild_arrays(%s) failed" % name)
            out[name] = _sized_array(ask, dtype).reshape((-1,) + shape)
        if "info" in out:
            out["info"] = dict(zip(REBUILD_ARRAY_INFO, (int(v) for v in out["info"])))
        return out

    def arrays(self, names=None) -> dict:
        """ptr_debug_scene_arrays: the named device arrays (all of SCENE_ARRAYS by default) as numpy arrays."""
        probe = load_library().ptr_debug_scene_arrays
        out = {}
        for name in (names or SCENE_ARRAYS):
            which, dtype, shape = SCENE_ARRAYS[name]
            out[name] = _sized_array(lambda o, cap, size: probe(self._h, which, o, cap, size), dtype, "ptr_debug_scene_arrays(%s)" % name).reshape((-1,) + shape)
        return out

    def timings(self) -> dict:
        """Seconds of the upload: geometry preparation (or cache read), shading tables, copies to the device."""
        out = (C.c_double * 4)()
        load_library().ptr_scene_timings(self._h, out)
        return {"geometry_s": out[0], "shading_tables_s": out[1], "copy_s": out[2], "geometry_from_cache": bool(out[3])}

    def info(self) -> dict:
        out = (C.c_uint64 * 8)()
        load_library().ptr_scene_info(self._h, out)
        keys = ("nodes", "leaves", "triangles", "spheres", "max_depth", "max_leaf", "sah_cost_x1000", "rect_lights")
        return dict(zip(keys, [int(v) for v in out]))

    def shade_kernel_set(self, settings: PtrSettings, count: bool = False) -> int:
        """ptr_debug_shade_kernel_set: the material / feature mask of the k_shade instantiation a render launches (0x3FF = full)."""
        out = C.c_uint32(0)
        if load_library().ptr_debug_shade_kernel_set(self._h, C.byref(settings), int(count), C.byref(out)) != 0:
            raise PtrError("ptr_debug_shade_kernel_set failed")
        return int(out.value)

    def surface_hits(self, rays) -> np.ndarray:
        """ptr_debug_surface_hits: rays [n, 9] {origin, direction, next direction} -> [n, 16]."""
        return _batch(load_library().ptr_debug_surface_hits, (self._h,), rays, np.float32, 9, [((16,), np.float32)])

    def render(self, settings: PtrSettings, spp: int, part: int = 0, parts: int = 1, count: bool = False
               ) -> Tuple[np.ndarray, PtrRenderStats]:
        """Render one partition to host memory.  Returns ([bands*BAND_ROWS, W, 3] float32, stats)."""
        lib = load_library()
        bands = band_count(settings.height, part, parts)
        out = np.zeros((bands * BAND_ROWS, settings.width, 3), dtype=np.float32)
        stats = PtrRenderStats()
        err = _err_buf()
        _check(lib.ptr_render_bands(self._h, C.byref(settings), spp, part, parts, _fptr(out), int(count),
                                    C.byref(stats), err, len(err)), err)
        return out, stats

    def render_image(self, settings: PtrSettings, spp: int, count: bool = False) -> Tuple[np.ndarray, PtrRenderStats]:
        out, stats = self.render(settings, spp, 0, 1, count)
        return out[: settings.height], stats

    def render_device(self, settings: PtrSettings, spp: int, d_out_ptr: int, stream: int = 0, part: int = 0,
                      parts: int = 1, count: bool = False, want_stats: bool = True, solo: bool = False
                      ) -> Optional[PtrRenderStats]:
        """Render into a caller-owned DEVICE buffer (e.g. a torch tensor's data_ptr()) on `stream`.
        solo=True runs the pool as one group (no concurrent kernels) so per-kernel timings are clean."""
        lib = load_library()
        stats = PtrRenderStats()
        err = _err_buf()
        _check(lib.ptr_render_bands_device(self._h, C.byref(settings), spp, part, parts, C.c_void_p(d_out_ptr),
                                           C.c_void_p(stream), int(count) | (2 if solo else 0), C.byref(stats) if want_stats else None,
                                           err, len(err)), err)
        return stats if want_stats else None

    def render_cov(self, settings: PtrSettings, spp: int, part: int = 0, parts: int = 1, count: bool = False
                   ) -> Tuple[np.ndarray, np.ndarray, PtrRenderStats]:
        """render() plus the covariance of every pixel's mean (include/ptr_stats.h; spp >= 2).  Returns ([bands*BAND_ROWS, W, 3],
        [bands*BAND_ROWS, W, 6] {rr, gg, bb, rg, rb, gb}, stats)."""
        lib = load_library()
        bands = band_count(settings.height, part, parts)
        out = np.zeros((bands * BAND_ROWS, settings.width, 3), dtype=np.float32)
        cov = np.zeros((bands * BAND_ROWS, settings.width, 6), dtype=np.float32)
        stats = PtrRenderStats()
        err = _err_buf()
        _check(lib.ptr_render_bands_cov(self._h, C.byref(settings), spp, part, parts, _fptr(out), _fptr(cov), int(count),
                                        C.byref(stats), err, len(err)), err)
        return out, cov, stats

    def render_image_cov(self, settings: PtrSettings, spp: int) -> Tuple[np.ndarray, np.ndarray, PtrRenderStats]:
        """([H, W, 3] image - the bits of render_image - , [H, W, 6] covariance of the pixel means, stats)."""
        out, cov, stats = self.render_cov(settings, spp)
        return out[: settings.height], cov[: settings.height], stats

    def render_cov_device(self, settings: PtrSettings, spp: int, d_out_ptr: int, d_cov_ptr: int, stream: int = 0, part: int = 0,
                          parts: int = 1, count: bool = False, want_stats: bool = True) -> Optional[PtrRenderStats]:
        """render_device() with a second caller-owned DEVICE buffer for the covariance (bands * BAND_ROWS * W * 6 floats)."""
        stats = PtrRenderStats()
        err = _err_buf()
        _check(load_library().ptr_render_bands_cov_device(self._h, C.byref(settings), spp, part, parts, C.c_void_p(d_out_ptr),
                                                          C.c_void_p(d_cov_ptr), C.c_void_p(stream), int(count),
                                                          C.byref(stats) if want_stats else None, err, len(err)), err)
        return stats if want_stats else None

    def debug_samples(self, settings: PtrSettings, spp: int) -> np.ndarray:
        """ptr_stats_debug_samples (tests): the frame's per-sample accumulators, [spp, H, W, 3] in sample order."""
        out = np.zeros((spp, settings.height, settings.width, 3), dtype=np.float32)
        err = _err_buf()
        _check(load_library().ptr_stats_debug_samples(self._h, C.byref(settings), spp, _fptr(out), err, len(err)), err)
        return out

    def render_adaptive(self, settings: PtrSettings, params: PtrAdaptiveParams, want_cov: bool = True, want_count: bool = True
                        ) -> Tuple[np.ndarray, Optional[np.ndarray], Optional[np.ndarray], PtrRenderStats, PtrAdaptiveInfo]:
        """An adaptive frame (include/ptr_adaptive.h): ([H, W, 3] image, [H, W, 6] covariance of the pixel means, [H, W] uint32 samples per
        pixel, stats, info), all in image order."""
        h, w = settings.height, settings.width
        rgb = np.zeros((h, w, 3), dtype=np.float32)
        cov = np.zeros((h, w, 6), dtype=np.float32) if want_cov else None
        count = np.zeros((h, w), dtype=np.uint32) if want_count else None
        stats, info = PtrRenderStats(), PtrAdaptiveInfo()
        err = _err_buf()
        _check(load_library().ptr_render_adaptive(self._h, C.byref(settings), C.byref(params), _fptr(rgb), _fptr(cov) if want_cov else None,
                                                  _uptr(count) if want_count else None, C.byref(stats), C.byref(info), err, len(err)), err)
        return rgb, cov, count, stats, info

    def render_adaptive_device(self, settings: PtrSettings, params: PtrAdaptiveParams, d_rgb_ptr: int, d_cov_ptr: int = 0, d_count_ptr: int = 0,
                               stream: int = 0, want_stats: bool = True) -> Tuple[Optional[PtrRenderStats], PtrAdaptiveInfo]:
        """render_adaptive() into caller-owned DEVICE buffers (e.g. torch tensors' data_ptr(); W*H*3 floats, W*H*6 floats or 0, W*H
        uint32 or 0) on `stream`.  Returns (stats, info)."""
        stats, info = PtrRenderStats(), PtrAdaptiveInfo()
        err = _err_buf()
        _check(load_library().ptr_render_adaptive_device(self._h, C.byref(settings), C.byref(params), C.c_void_p(d_rgb_ptr),
                                                         C.c_void_p(d_cov_ptr or None), C.c_void_p(d_count_ptr or None), C.c_void_p(stream or None),
                                                         C.byref(stats) if want_stats else None, C.byref(info), err, len(err)), err)
        return (stats if want_stats else None), info

    def frame(self, settings: PtrSettings) -> "Frame":
        """A resumable frame on this scene (include/ptr_frame.h): its per-pixel sample state stays on the device between calls."""
        h = C.c_void_p()
        err = _err_buf()
        _check(load_library().ptr_frame_create(self._h, C.byref(settings), C.byref(h), err, len(err)), err)
        return Frame(h, keepalive=self)

    def temporal(self, width: int, height: int, params: Optional["PtrTemporalParams"] = None, cov=None) -> "Temporal":
        """ptr_temporal_create: a temporal-accumulation handle for width x height frames of this scene (include/ptr_temporal.h).
        cov=True or a PtrTemporalCovParams: ptr_temporal_create_cov, a handle that carries covariance (include/ptr_temporal_cov.h)."""
        h = C.c_void_p()
        err = _err_buf()
        p = C.byref(params) if params is not None else None
        if cov is None or cov is False:
            _check(load_library().ptr_temporal_create(self._h, width, height, p, C.byref(h), err, len(err)), err)
            return Temporal(h, width, height, self._device, keepalive=self)
        if cov is not True and not isinstance(cov, PtrTemporalCovParams):
            raise PtrError("DeviceScene.temporal: cov is True or a PtrTemporalCovParams")
        _check(load_library().ptr_temporal_create_cov(self._h, width, height, p, None if cov is True else C.byref(cov), C.byref(h), err, len(err)), err)
        return Temporal(h, width, height, self._device, keepalive=self, carries_cov=True)

    def render_aovs(self, settings: PtrSettings, sample_index: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """First-hit feature buffers: ([H, W, 4] albedo rgb | hit flag, [H, W, 4] encoded normal | distance) of the first surface the
        path of sample `sample_index` shades under settings.metalSemantics (include/ptr_abi.h: the rule at ptr_render_aovs)."""
        albedo = np.zeros((settings.height, settings.width, 4), dtype=np.float32)
        normal = np.zeros((settings.height, settings.width, 4), dtype=np.float32)
        err = _err_buf()
        _check(load_library().ptr_render_aovs(self._h, C.byref(settings), sample_index, _fptr(albedo), _fptr(normal), err, len(err)), err)
        return albedo, normal

    def render_signatures(self, settings: PtrSettings) -> Tuple[np.ndarray, np.ndarray]:
        """One sample per pixel with the path signature of every pixel (include/ptr_debug.h): ([H, W, 3] image, [H, W] uint32)."""
        img = np.zeros((settings.height, settings.width, 3), dtype=np.float32)
        sig = np.zeros((settings.height, settings.width), dtype=np.uint32)
        err = _err_buf()
        _check(load_library().ptr_debug_render_signatures(self._h, C.byref(settings), _fptr(img), sig.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                          err, len(err)), err)
        return img, sig

    def texture_sample(self, texture: int, uv_lod: np.ndarray) -> np.ndarray:
        """Filtered texture lookups on the device (include/ptr_debug.h): uv_lod [n, 3] -> [n, 4] RGBA."""
        return _batch(load_library().ptr_debug_texture_sample, (self._h, texture), uv_lod, np.float32, 3, [((4,), np.float32)])

    def texture_sample_grad(self, texture: int, uv_grad: np.ndarray) -> np.ndarray:
        """ptr_debug_texture_sample_grad: the anisotropic gradient sample of PTR_METAL_RAY_DIFF (csrc/kernels/texture.h):
        uv_grad [n, 6] {u, v, dudx, dvdx, dudy, dvdy} -> [n, 4] RGBA."""
        return _batch(load_library().ptr_debug_texture_sample_grad, (self._h, texture), uv_grad, np.float32, 6, [((4,), np.float32)])

    # field -> column slice of the rows first_hit_textures returns (include/ptr_debug.h ptr_debug_first_hit_textures)
    FIRST_HIT_FIELDS = {"textured": 0, "t": 1, "uv0": slice(2, 4), "uv1": slice(4, 6), "grad0": slice(6, 10), "grad1": slice(10, 14),
                        "valid0": 14, "valid1": 15, "base_uv": slice(16, 18), "base_grad": slice(18, 22), "base_valid": 22,
                        "base_color": slice(23, 26), "roughness": 26, "emissive": slice(27, 30), "normal": slice(30, 33), "metallic": 33,
                        "discard": 34}

    def first_hit_textures(self, settings: PtrSettings, xys: np.ndarray) -> dict:
        """ptr_debug_first_hit_textures: the first hit of the camera rays of xys [n, 3] {x, y, sample} as k_shade textures it (with
        PTR_METAL_RAY_DIFF in settings.metalSemantics: the first-hit gradients).  Returns FIRST_HIT_FIELDS -> arrays (grad*: {dudx, dvdx,
        dudy, dvdy}), plus "raw" [n, 36]."""
        out = _batch(load_library().ptr_debug_first_hit_textures, (self._h, C.byref(settings)), xys, np.uint32, 3, [((36,), np.float32)])
        res = {k: out[:, v] for k, v in self.FIRST_HIT_FIELDS.items()}
        res["raw"] = out
        return res

    # field -> (columns, dtype) of the rows of ptr_debug_pbr_hits (include/ptr_debug_pbr.h); the oracle's oracle_pbr_hits reports the same rows
    PBR_HIT_FIELDS = {"hit": (0, np.float32), "t": (1, np.float32), "mesh": (2, np.uint32), "triangle": (3, np.uint32), "bu": (4, np.float32),
                      "bv": (5, np.float32), "front_face": (6, np.float32), "geometric_normal": (slice(7, 10), np.float32),
                      "hit_normal": (slice(10, 13), np.float32), "textured": (13, np.float32), "base_color": (slice(14, 17), np.float32),
                      "roughness": (17, np.float32), "emissive": (slice(18, 21), np.float32), "metallic": (21, np.float32),
                      "transmission": (22, np.float32), "occlusion": (23, np.float32), "normal": (slice(24, 27), np.float32),
                      "two_sided": (27, np.float32), "discard": (28, np.float32), "state": (29, np.uint32), "basis": (30, np.uint32)}

    @staticmethod
    def pbr_hit_rows(rays, cones, states, materials=None, instantiation=0, grads=None, valid=None) -> np.ndarray:
        """The [n, 20] input rows of ptr_debug_pbr_hits: rays [n, 6] {origin, direction}, cones [n, 2] {width, spread}, random states [n],
        material indices [n] (None: the hit's own), the instantiation (0 / 1, a scalar or [n]), grads [n, 8] and valid bits [n]."""
        rays = np.asarray(rays, dtype=np.float32).reshape(-1, 6)
        n = rays.shape[0]
        rows = np.zeros((n, 20), dtype=np.float32)
        words = rows.view(np.uint32)
        rows[:, 0:6] = rays
        rows[:, 6:8] = np.asarray(cones, dtype=np.float32).reshape(-1, 2)
        words[:, 8] = np.asarray(states, dtype=np.uint32)
        words[:, 9] = 0xFFFFFFFF if materials is None else np.asarray(materials, dtype=np.uint32)
        words[:, 10] = np.asarray(instantiation, dtype=np.uint32)
        if grads is not None:
            rows[:, 11:19] = np.asarray(grads, dtype=np.float32).reshape(-1, 8)
        if valid is not None:
            words[:, 19] = np.asarray(valid, dtype=np.uint32)
        return rows

    @classmethod
    def pbr_hit_fields(cls, out: np.ndarray) -> dict:
        words = out.view(np.uint32)
        res = {k: (words if dt == np.uint32 else out)[:, cols] for k, (cols, dt) in cls.PBR_HIT_FIELDS.items()}
        res["raw"] = out
        return res

    def pbr_hits(self, rows: np.ndarray) -> dict:
        """ptr_debug_pbr_hits: the per-hit material of the textured metallic-roughness model (applyPbrTextures) at the closest hit of
        the rays of rows [n, 20] (pbr_hit_rows).  Returns PBR_HIT_FIELDS -> arrays, plus "raw" [n, 32]."""
        return self.pbr_hit_fields(_batch(load_library().ptr_debug_pbr_hits, (self._h,), rows, np.float32, 20, [((32,), np.float32)]))

    def sss_walks(self, settings: PtrSettings, xys: np.ndarray, step_cap: int = SSS_MAX_STEPS):
        """ptr_debug_sss_walks: the first bounce of the camera samples xys [n, 3] {x, y, sample} with its whole subsurface random walk, by
        the device code shadeSlot calls (include/ptr_debug_sss.h; meaningful only on scenes without lights and sampled environment).
        Returns (SSS_WALK_STEP_FIELDS -> [n, step_cap, ..] arrays, SSS_WALK_FINAL_FIELDS -> [n, ..] arrays), each with its "raw" rows."""
        xys = np.ascontiguousarray(xys, dtype=np.uint32).reshape(-1, 3)
        steps = np.zeros((xys.shape[0], step_cap, 24), dtype=np.float32)
        final = np.zeros((xys.shape[0], 24), dtype=np.float32)
        err = _err_buf()
        _check(load_library().ptr_debug_sss_walks(self._h, C.byref(settings), _uptr(xys), xys.shape[0], step_cap, _fptr(steps), _fptr(final),
                                                  err, len(err)), err)
        return sss_fields(steps, SSS_WALK_STEP_FIELDS), sss_fields(final, SSS_WALK_FINAL_FIELDS)

    def path_states(self, settings: PtrSettings, pixels: np.ndarray, sample: int = 0, max_iterations: int = 64):
        """ptr_debug_path_states: sample `sample` of the pixels [n] (y * width + x) through the production kernels, one iteration at a
        time over a pool of one slot per pixel (include/ptr_debug_path.h).  Returns (PATH_STATE_FIELDS -> [iterations recorded, n, ..]
        arrays plus "raw", the iterations the loop ran, itemAccum [n, 4])."""
        pixels = np.ascontiguousarray(pixels, dtype=np.uint32).reshape(-1)
        states = np.zeros((max_iterations, pixels.shape[0], PATH_STATE_WORDS), dtype=np.uint32)
        items = np.zeros((pixels.shape[0], 4), dtype=np.float32)
        ran = C.c_uint32(0)
        err = _err_buf()
        _check(load_library().ptr_debug_path_states(self._h, C.byref(settings), _uptr(pixels), pixels.shape[0], sample, max_iterations,
                                                    _uptr(states), C.byref(ran), _fptr(items), err, len(err)), err)
        rows = states[: min(int(ran.value), max_iterations)].view(np.float32)
        return sss_fields(rows, PATH_STATE_FIELDS), int(ran.value), items

    def env_lookup(self, settings: PtrSettings, dir_roughness: np.ndarray) -> np.ndarray:
        """ptr_debug_env_lookup: the PTR_METAL_ENV_LOD lookup of the scene's environment map with the settings' rotation and intensity:
        dir_roughness [n, 4] {direction, roughness} -> [n, 4] {LOD, rgb}."""
        return _batch(load_library().ptr_debug_env_lookup, (self._h, C.byref(settings)), dir_roughness, np.float32, 4, [((4,), np.float32)])

    def env_sample(self, settings: PtrSettings, u: np.ndarray) -> np.ndarray:
        """ptr_debug_env_sample: u [n, 3] {marginal, conditional, jitter} -> [n, 8] {envSample's direction and pdf, then envLookup's rgb and
        envPdfOf's pdf along that direction}."""
        return _batch(load_library().ptr_debug_env_sample, (self._h, C.byref(settings)), u, np.float32, 3, [((8,), np.float32)])

    def env_eval(self, settings: PtrSettings, directions: np.ndarray) -> np.ndarray:
        """ptr_debug_env_eval: directions [n, 3] (any length) -> [n, 4] {envLookup's level-0 rgb, envPdfOf's pdf}."""
        return _batch(load_library().ptr_debug_env_eval, (self._h, C.byref(settings)), directions, np.float32, 3, [((4,), np.float32)])

    def rect_light_nee(self, settings: PtrSettings, rays: np.ndarray, thr: np.ndarray, states: np.ndarray,
                       material: Optional[PtrMaterial] = None) -> Tuple[np.ndarray, np.ndarray]:
        """ptr_debug_rect_light_nee: rectLightNee at the hits of rays [n, 6] {origin, direction} with throughput thr [n, 3] and random
        states [n]; material: an override for the hit's own.  Returns ([n, 16] {hit, queued, shadow origin, direction, tmax, contribution,
        0...}, the random states afterwards)."""
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
        thr = np.ascontiguousarray(thr, dtype=np.float32).reshape(-1, 3)
        states = np.ascontiguousarray(states, dtype=np.uint32).reshape(-1)
        if thr.shape[0] != rays.shape[0] or states.shape[0] != rays.shape[0]:
            raise ValueError("thr and states need one entry per ray")
        return _batch(load_library().ptr_debug_rect_light_nee, (self._h, C.byref(settings), None if material is None else C.byref(material)),
                      rays, np.float32, 6, [((16,), np.float32), ((), np.uint32)], more=(_fptr(thr), _uptr(states)))

    def light_connection(self, settings: PtrSettings, inputs: np.ndarray) -> Tuple[np.ndarray, dict]:
        """ptr_debug_light_connection: inputs [n, 14] {origin, direction, bsdf weight, bsdf pdf, throughput, 0} -> ([n, 12] {found, t, light,
        half, ignore word bits, contribution, pdf, front face, 0, 0}, {settles, lights})."""
        info = (C.c_uint32 * 2)()
        out = _batch(load_library().ptr_debug_light_connection, (self._h, C.byref(settings)), inputs, np.float32, 14, [((12,), np.float32)],
                     tail=(info,))
        return out, {"settles": bool(info[0]), "lights": int(info[1])}

    def trace_rays(self, rays: np.ndarray, any_hit: bool = False) -> Tuple[np.ndarray, PtrRenderStats]:
        """rays: [n, 8] float32 {ox,oy,oz,tmin,dx,dy,dz,tmax}; returns a structured array of PtrHit."""
        lib = load_library()
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        out = np.zeros(rays.shape[0], dtype=HIT_DTYPE)
        stats = PtrRenderStats()
        err = _err_buf()
        _check(lib.ptr_trace_rays(self._h, _fptr(rays), rays.shape[0], int(any_hit), out.ctypes.data_as(C.c_void_p),
                                  C.byref(stats), err, len(err)), err)
        return out, stats

    # node formats of the persistent traversal kernels (ptr_debug_extend_rays info[0])
    NODE_FORMATS = {0: "float", 1: "quantised binary", 2: "four-wide", 3: "counting build"}

    @staticmethod
    def _probe_info(info) -> dict:
        return {"format": int(info[0]), "stack_limit": int(info[1]), "wide_depth": int(info[2]), "lds_levels": int(info[3])}

    def extend_rays(self, rays: np.ndarray, count: bool = False) -> Tuple[np.ndarray, dict]:
        """ptr_debug_extend_rays: closest hits through the production k_extend (the render's launcher and node format).  rays [n, 8]
        {origin, 1e-4, direction, inf}; returns (PtrHit records as trace_rays returns them, {format, stack_limit, wide_depth, lds_levels})."""
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        out = np.zeros(rays.shape[0], dtype=HIT_DTYPE)
        info = (C.c_uint32 * 4)()
        err = _err_buf()
        _check(load_library().ptr_debug_extend_rays(self._h, _fptr(rays), rays.shape[0], int(count), out.ctypes.data_as(C.c_void_p), info,
                                                    err, len(err)), err)
        return out, self._probe_info(info)

    def connect_rays(self, rays: np.ndarray, ignore_light: Optional[np.ndarray] = None, records_per_slot: int = 1
                     ) -> Tuple[np.ndarray, dict]:
        """ptr_debug_connect_rays: any-hit queries through the production k_connect as queued light connections.  rays [n, 8] {origin,
        1e-4, direction, tmax}; ignore_light [n] (optional): 0xFFFFFFFF or the rectangle light whose own triangles the query ignores (a
        kind-3 record).  Returns (occluded [n] bool, info as extend_rays)."""
        rays = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        occ = np.zeros(rays.shape[0], dtype=np.uint32)
        ign = None if ignore_light is None else np.ascontiguousarray(ignore_light, dtype=np.uint32).reshape(-1)
        if ign is not None and ign.shape[0] != rays.shape[0]:
            raise ValueError("ignore_light needs one entry per ray")
        info = (C.c_uint32 * 4)()
        err = _err_buf()
        _check(load_library().ptr_debug_connect_rays(self._h, _fptr(rays), None if ign is None else _uptr(ign), rays.shape[0],
                                                     records_per_slot, _uptr(occ), info, err, len(err)), err)
        return occ.astype(bool), self._probe_info(info)

    def close(self) -> None:
        if self._h:
            load_library().ptr_scene_release(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _BorrowedScene(DeviceScene):
    """A partition's scene of a MultiFrame (MultiFrame.part_scene): not owned, never released here, never updated but through the frame."""

    def __init__(self, handle: C.c_void_p, device: int, frame):
        self._h, self._device, self._keepalive = handle, int(device), frame

    def _through_the_frame(self, *args, **kwargs):
        raise PtrError("a partition's scene is updated through its MultiFrame: a call on one partition would desynchronise them")

    set_mesh_transforms = set_mesh_vertices = set_mesh_vertices_device = set_spheres = set_rects = rebuild_tree = _through_the_frame
    set_materials = set_textures = set_textures_device = set_environment = set_environment_device = _through_the_frame

    def close(self) -> None:
        pass


FRAME_STATE = (("sum", 3, np.float32), ("mean", 3, np.float32), ("m", 6, np.float32), ("n", 0, np.uint32), ("e", 0, np.float32))


class Frame:
    """include/ptr_frame.h: the sample state of a frame, continued call by call; made by DeviceScene.frame() or debug_frame().  It keeps
    its scene alive (a scene closed by hand must be closed after its frames)."""

    def __init__(self, handle: C.c_void_p, keepalive=None):
        self._h = handle
        self._keepalive = keepalive

    def _handle(self):
        if not self._h:
            raise PtrError("the frame is closed")
        return self._h

    def accumulate(self, spp: int, stream: int = 0) -> PtrRenderStats:
        """Every pixel gets `spp` more samples (the frame must be uniform)."""
        stats = PtrRenderStats()
        err = _err_buf()
        _check(load_library().ptr_frame_accumulate(self._handle(), spp, C.c_void_p(stream or None), C.byref(stats), err, len(err)), err)
        return stats

    def refine(self, params: PtrAdaptiveParams, stream: int = 0) -> Tuple[PtrRenderStats, PtrAdaptiveInfo]:
        """The resumable adaptive loop: pixels whose dilated error is above params.threshold go on, each from its own count, up to
        params.maxSpp.  Returns (stats, info) of this call."""
        stats, info = PtrRenderStats(), PtrAdaptiveInfo()
        err = _err_buf()
        _check(load_library().ptr_frame_refine(self._handle(), C.byref(params), C.c_void_p(stream or None), C.byref(stats), C.byref(info), err,
                                               len(err)), err)
        return stats, info

    def info(self) -> PtrFrameInfo:
        out = PtrFrameInfo()
        if load_library().ptr_frame_info(self._handle(), C.byref(out)) != 0:
            raise PtrError("ptr_frame_info failed")
        return out

    def resolve(self, want_cov: bool = True, want_count: bool = True) -> Tuple[np.ndarray, Optional[np.ndarray], Optional[np.ndarray]]:
        """([H, W, 3] image, [H, W, 6] covariance of the pixel means, [H, W] uint32 samples per pixel), image order; the state stays."""
        i = self.info()
        rgb = np.zeros((i.height, i.width, 3), dtype=np.float32)
        cov = np.zeros((i.height, i.width, 6), dtype=np.float32) if want_cov else None
        count = np.zeros((i.height, i.width), dtype=np.uint32) if want_count else None
        err = _err_buf()
        _check(load_library().ptr_frame_resolve(self._handle(), _fptr(rgb), _fptr(cov) if want_cov else None, _uptr(count) if want_count else None,
                                                err, len(err)), err)
        return rgb, cov, count

    def resolve_device(self, d_rgb: int, d_cov: int = 0, d_count: int = 0, stream: int = 0) -> None:
        """resolve() into caller-owned DEVICE buffers (W*H*3 floats, W*H*6 floats or 0, W*H uint32 or 0) on `stream`."""
        err = _err_buf()
        _check(load_library().ptr_frame_resolve_device(self._handle(), C.c_void_p(d_rgb), C.c_void_p(d_cov or None), C.c_void_p(d_count or None),
                                                       C.c_void_p(stream or None), err, len(err)), err)

    def export_state(self) -> dict:
        """The checkpoint: {"sum" [P, 3], "mean" [P, 3], "m" [P, 6], "n" [P] uint32, "e" [P]}, image order."""
        i = self.info()
        pixels = i.width * i.height
        st = {k: np.zeros((pixels, cols) if cols else pixels, dtype=dt) for k, cols, dt in FRAME_STATE}
        err = _err_buf()
        _check(load_library().ptr_frame_export(self._handle(), _fptr(st["sum"]), _fptr(st["mean"]), _fptr(st["m"]), _uptr(st["n"]), _fptr(st["e"]),
                                               err, len(err)), err)
        return st

    def import_state(self, state: dict) -> None:
        i = self.info()
        pixels = i.width * i.height
        st = {k: np.ascontiguousarray(state[k], dtype=dt).reshape((pixels, cols) if cols else pixels) for k, cols, dt in FRAME_STATE}
        err = _err_buf()
        _check(load_library().ptr_frame_import(self._handle(), _fptr(st["sum"]), _fptr(st["mean"]), _fptr(st["m"]), _uptr(st["n"]), _fptr(st["e"]),
                                               err, len(err)), err)

    def reset(self, settings: Optional[PtrSettings] = None) -> None:
        """The state back to zero; `settings` of the same size replace the stored ones."""
        err = _err_buf()
        _check(load_library().ptr_frame_reset(self._handle(), C.byref(settings) if settings is not None else None, err, len(err)), err)

    def close(self) -> None:
        if self._h:
            load_library().ptr_frame_release(self._h)
            self._h = None
        self._keepalive = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Temporal:
    """Temporal accumulation over the frames of a sequence (include/ptr_temporal.h): each step blends a frame with the history of the
    surfaces it shows.  Made by DeviceScene.temporal(); the scene must be in the pose of the frame a step is given.  A handle made with
    cov carries the covariance of its colour (include/ptr_temporal_cov.h): its steps take the frame's covariance and return the blend's;
    the library refuses a step of the other kind."""

    def __init__(self, handle: C.c_void_p, width: int, height: int, device: int, keepalive=None, carries_cov: bool = False):
        self._h, self._keepalive, self.carries_cov = handle, keepalive, bool(carries_cov)
        self.width, self.height, self._device = int(width), int(height), int(device)

    def _handle(self):
        if not self._h:
            raise PtrError("the temporal handle is closed")
        return self._h

    def step(self, settings: PtrSettings, rgb: np.ndarray, cov: Optional[np.ndarray] = None, want_length: bool = True,
             want_aovs: bool = False) -> dict:
        """ptr_temporal_step on a host image [H, W, 3]: {"rgb", "info", and when asked for "length" [H, W], "albedo" and "normal" [H, W, 4]}.
        With cov [H, W, 6] (a handle that carries covariance needs it): ptr_temporal_step_cov, and "cov" [H, W, 6] beside them."""
        rgb = np.ascontiguousarray(rgb, np.float32)
        if rgb.size != self.width * self.height * 3:
            raise PtrError("Temporal.step: the image has %d floats, not %d x %d x 3" % (rgb.size, self.height, self.width))
        h, w = self.height, self.width
        out = {"rgb": np.zeros((h, w, 3), np.float32)}
        if cov is not None:
            cov = np.ascontiguousarray(cov, np.float32)
            if cov.size != w * h * 6:
                raise PtrError("Temporal.step: the covariance has %d floats, not %d x %d x 6" % (cov.size, h, w))
            out["cov"] = np.zeros((h, w, 6), np.float32)
        if want_length:
            out["length"] = np.zeros((h, w), np.float32)
        if want_aovs:
            out["albedo"], out["normal"] = np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32)
        opt = lambda key: _fptr(out[key]) if key in out else None
        info = PtrTemporalInfo()
        err = _err_buf()
        if cov is not None:
            _check(load_library().ptr_temporal_step_cov(self._handle(), C.byref(settings), _fptr(rgb), _fptr(cov), _fptr(out["rgb"]), _fptr(out["cov"]),
                                                        opt("length"), opt("albedo"), opt("normal"), C.byref(info), err, len(err)), err)
        else:
            _check(load_library().ptr_temporal_step(self._handle(), C.byref(settings), _fptr(rgb), _fptr(out["rgb"]), opt("length"), opt("albedo"),
                                                    opt("normal"), C.byref(info), err, len(err)), err)
        out["info"] = info.as_dict()
        return out

    def step_device(self, settings: PtrSettings, rgb, out_rgb=None, out_length=None, out_albedo=None, out_normal=None, stream=None,
                    want_info: bool = False, cov=None, out_cov=None) -> Optional[dict]:
        """ptr_temporal_step_device on torch tensors of the scene's device, float32 and contiguous, passed by data_ptr(): rgb [H, W, 3];
        out_rgb (None: rgb itself, filtered in place); out_length [H, W], out_albedo and out_normal [H, W, 4] may be None.  The step is
        enqueued on `stream` (a raw stream handle; None: torch's current stream of the scene's device) and the call returns at once,
        unless want_info: then it waits and returns PtrTemporalInfo as a dict.  With cov [H, W, 6] (a handle that carries covariance needs
        it): ptr_temporal_step_cov_device; out_cov [H, W, 6] (None: cov itself, in place) goes as it is into denoise_device(d_cov=...)."""
        if out_rgb is None:
            out_rgb = rgb
        if cov is not None and out_cov is None:
            out_cov = cov
        if cov is None and out_cov is not None:
            raise PtrError("Temporal.step_device: out_cov without cov")
        pixels = self.width * self.height
        ptrs = []
        for name, t, floats in (("rgb", rgb, 3), ("cov", cov, 6), ("out_rgb", out_rgb, 3), ("out_cov", out_cov, 6), ("out_length", out_length, 1),
                                ("out_albedo", out_albedo, 4), ("out_normal", out_normal, 4)):
            if t is None and name in ("cov", "out_cov"):
                continue
            if t is None:
                ptrs.append(None)
                continue
            device = getattr(t, "device", None)
            if not hasattr(t, "data_ptr") or device is None:
                raise PtrError("Temporal.step_device: %s is not a torch tensor" % name)
            if device.type != "cuda" or device.index != self._device:
                raise PtrError("Temporal.step_device: %s is on %s, not on device %d of the scene" % (name, device, self._device))
            if str(t.dtype) != "torch.float32" or not t.is_contiguous() or t.numel() != pixels * floats:
                raise PtrError("Temporal.step_device: %s must be contiguous float32 with %d elements" % (name, pixels * floats))
            ptrs.append(C.c_void_p(t.data_ptr()))
        if stream is None:
            import torch   # (only here: the module itself does not need torch)

            stream = torch.cuda.current_stream(self._device).cuda_stream
        info = PtrTemporalInfo()
        err = _err_buf()
        fn = load_library().ptr_temporal_step_device if cov is None else load_library().ptr_temporal_step_cov_device
        _check(fn(self._handle(), C.byref(settings), *ptrs, C.c_void_p(stream), C.byref(info) if want_info else None, err, len(err)), err)
        return info.as_dict() if want_info else None

    def records(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """ptr_debug_temporal_records: R0, R1, R2 of the last step, [H, W, 4] float32 each."""
        out = [np.zeros((self.height, self.width, 4), np.float32) for _ in range(3)]
        err = _err_buf()
        _check(load_library().ptr_debug_temporal_records(self._handle(), *map(_fptr, out), err, len(err)), err)
        return tuple(out)

    def reset(self) -> None:
        """ptr_temporal_reset: the next step is a first step."""
        load_library().ptr_temporal_reset(self._handle())

    def close(self) -> None:
        if self._h:
            load_library().ptr_temporal_release(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def debug_temporal_camera(settings: PtrSettings) -> np.ndarray:
    """ptr_debug_temporal_camera: [4, 3] origin, lowerLeft, horizontal, vertical of the renderer's camera."""
    out = np.zeros((4, 3), np.float32)
    if load_library().ptr_debug_temporal_camera(C.byref(settings), _fptr(out)) != 0:
        raise PtrError("ptr_debug_temporal_camera failed")
    return out


def debug_temporal_accumulate(rgb: np.ndarray, cur_records, prev_records, history: np.ndarray, cam_cur, cam_prev,
                              params: Optional[PtrTemporalParams] = None, has_history: bool = True, device: int = 0):
    """ptr_debug_temporal_accumulate: k_temporal_accumulate alone.  rgb [H, W, 3]; cur_records (R0, R1, R2) and prev_records (R0, R1) of
    [H, W, 4]; history [H, W, 4]; cameras [4, 3].  Returns (rgb [H, W, 3], length [H, W], history [H, W, 4])."""
    rgb = np.ascontiguousarray(rgb, np.float32)
    h, w = rgb.shape[:2]
    cur = np.ascontiguousarray(np.stack([np.asarray(r, np.float32).reshape(h, w, 4) for r in cur_records]))
    prev = np.ascontiguousarray(np.stack([np.asarray(r, np.float32).reshape(h, w, 4) for r in prev_records]))
    history = np.ascontiguousarray(history, np.float32).reshape(h, w, 4)
    cams = [np.ascontiguousarray(c, np.float32).reshape(12) for c in (cam_cur, cam_prev)]
    if len(cur) != 3 or len(prev) != 2:
        raise PtrError("debug_temporal_accumulate: three current and two previous records")
    p = params if params is not None else PtrTemporalParams.defaults()
    out, length, hist = np.zeros((h, w, 3), np.float32), np.zeros((h, w), np.float32), np.zeros((h, w, 4), np.float32)
    err = _err_buf()
    _check(load_library().ptr_debug_temporal_accumulate(w, h, C.byref(p), int(has_history), _fptr(rgb), _fptr(cur), _fptr(prev), _fptr(history),
                                                        _fptr(cams[0]), _fptr(cams[1]), device, _fptr(out), _fptr(length), _fptr(hist), err,
                                                        len(err)), err)
    return out, length, hist


def debug_temporal_accumulate_cov(rgb: np.ndarray, cov: np.ndarray, cur_records, prev_records, history: np.ndarray, cov_history: np.ndarray,
                                  cam_cur, cam_prev, params: Optional[PtrTemporalParams] = None,
                                  cov_params: Optional[PtrTemporalCovParams] = None, has_history: bool = True, device: int = 0):
    """ptr_debug_temporal_accumulate_cov: k_temporal_accumulate_cov alone.  The arguments of debug_temporal_accumulate, and cov and
    cov_history [H, W, 6].  Returns (rgb [H, W, 3], length [H, W], history [H, W, 4], cov [H, W, 6], cov history [H, W, 6])."""
    rgb = np.ascontiguousarray(rgb, np.float32)
    h, w = rgb.shape[:2]
    cov = np.ascontiguousarray(cov, np.float32).reshape(h, w, 6)
    cov_history = np.ascontiguousarray(cov_history, np.float32).reshape(h, w, 6)
    cur = np.ascontiguousarray(np.stack([np.asarray(r, np.float32).reshape(h, w, 4) for r in cur_records]))
    prev = np.ascontiguousarray(np.stack([np.asarray(r, np.float32).reshape(h, w, 4) for r in prev_records]))
    history = np.ascontiguousarray(history, np.float32).reshape(h, w, 4)
    cams = [np.ascontiguousarray(c, np.float32).reshape(12) for c in (cam_cur, cam_prev)]
    if len(cur) != 3 or len(prev) != 2:
        raise PtrError("debug_temporal_accumulate_cov: three current and two previous records")
    p = params if params is not None else PtrTemporalParams.defaults()
    cp = cov_params if cov_params is not None else PtrTemporalCovParams.defaults()
    out, length, hist = np.zeros((h, w, 3), np.float32), np.zeros((h, w), np.float32), np.zeros((h, w, 4), np.float32)
    out_cov, cov_hist = np.zeros((h, w, 6), np.float32), np.zeros((h, w, 6), np.float32)
    err = _err_buf()
    _check(load_library().ptr_debug_temporal_accumulate_cov(w, h, C.byref(p), C.byref(cp), int(has_history), _fptr(rgb), _fptr(cov), _fptr(cur),
                                                            _fptr(prev), _fptr(history), _fptr(cov_history), _fptr(cams[0]), _fptr(cams[1]), device,
                                                            _fptr(out), _fptr(out_cov), _fptr(length), _fptr(hist), _fptr(cov_hist), err,
                                                            len(err)), err)
    return out, length, hist, out_cov, cov_hist


def debug_frame(samples: np.ndarray, device: int = 0) -> Frame:
    """ptr_frame_debug_create (tests): a frame without a scene whose samples are `samples` [S, H, W, 3 or 4]."""
    samples = np.asarray(samples, dtype=np.float32)
    count, h, w = samples.shape[:3]
    x4 = np.zeros((count, h, w, 4), dtype=np.float32)
    x4[..., :3] = samples[..., :3]
    handle = C.c_void_p()
    err = _err_buf()
    _check(load_library().ptr_frame_debug_create(w, h, _fptr(x4), count, device, C.byref(handle), err, len(err)), err)
    return Frame(handle)


def render_multi(desc: PtrSceneDesc, settings: PtrSettings, spp: int, n_devices: int = 0, device_ids=None, verbose: bool = False
                 ) -> Tuple[np.ndarray, PtrRenderStats]:
    """The frame spread over several devices of this node (ptr_render_multi): [H, W, 3] float32 + stats.  `device_ids` (tests) names the
    devices explicitly; an id may repeat, so a one-GPU box can run the whole multi-device path."""
    lib = load_library()
    img = np.zeros((settings.height, settings.width, 3), dtype=np.float32)
    stats = PtrRenderStats()
    err = _err_buf()
    if device_ids is not None:
        ids = (C.c_int * len(device_ids))(*device_ids)
        _check(lib.ptr_debug_render_multi_on(C.byref(desc), C.byref(settings), spp, ids, len(device_ids), _fptr(img), C.byref(stats), err, len(err)), err)
    else:
        _check(lib.ptr_render_multi(C.byref(desc), C.byref(settings), spp, n_devices, int(verbose), _fptr(img), C.byref(stats), err, len(err)), err)
    return img, stats


def _aov_pair(settings: PtrSettings, want: bool):
    if not want:
        return None, None
    return (np.zeros((settings.height, settings.width, 4), dtype=np.float32), np.zeros((settings.height, settings.width, 4), dtype=np.float32))


def _opt(a, ptr):
    return None if a is None else ptr(a)


def render_multi_cov(desc: PtrSceneDesc, settings: PtrSettings, spp: int, n_devices: int = 0, device_ids=None, want_aovs: bool = False,
                     verbose: bool = False) -> dict:
    """A uniform frame over several devices with the covariance of the pixel means (include/ptr_multi.h ptr_render_multi_cov): a dict
    with rgb [H, W, 3], cov [H, W, 6], albedo / normal ([H, W, 4] each, None unless want_aovs), stats and multi (PtrMultiInfo).
    `device_ids` (tests) names the devices explicitly as render_multi's does; -(id + 1) forces the staged hand-over."""
    lib = load_library()
    rgb = np.zeros((settings.height, settings.width, 3), dtype=np.float32)
    cov = np.zeros((settings.height, settings.width, 6), dtype=np.float32)
    albedo, normal = _aov_pair(settings, want_aovs)
    stats, multi = PtrRenderStats(), PtrMultiInfo()
    err = _err_buf()
    tail = (_fptr(rgb), _fptr(cov), _opt(albedo, _fptr), _opt(normal, _fptr), C.byref(stats), C.byref(multi), err, len(err))
    if device_ids is not None:
        ids = (C.c_int * len(device_ids))(*device_ids)
        _check(lib.ptr_multi_debug_cov_on(C.byref(desc), C.byref(settings), spp, ids, len(device_ids), *tail), err)
    else:
        _check(lib.ptr_render_multi_cov(C.byref(desc), C.byref(settings), spp, n_devices, int(verbose), *tail), err)
    return {"rgb": rgb, "cov": cov, "albedo": albedo, "normal": normal, "stats": stats, "multi": multi}


def render_multi_adaptive(desc: PtrSceneDesc, settings: PtrSettings, params: PtrAdaptiveParams, n_devices: int = 0, device_ids=None,
                          want_cov: bool = True, want_count: bool = True, want_aovs: bool = False, verbose: bool = False) -> dict:
    """An adaptive frame over several devices (include/ptr_multi.h ptr_render_multi_adaptive), bit for bit DeviceScene.render_adaptive's:
    a dict with rgb [H, W, 3], cov [H, W, 6] or None, count [H, W] uint32 or None, albedo / normal (None unless want_aovs), stats, info
    (PtrAdaptiveInfo) and multi (PtrMultiInfo).  `device_ids` as render_multi_cov's."""
    lib = load_library()
    h, w = settings.height, settings.width
    rgb = np.zeros((h, w, 3), dtype=np.float32)
    cov = np.zeros((h, w, 6), dtype=np.float32) if want_cov else None
    count = np.zeros((h, w), dtype=np.uint32) if want_count else None
    albedo, normal = _aov_pair(settings, want_aovs)
    stats, info, multi = PtrRenderStats(), PtrAdaptiveInfo(), PtrMultiInfo()
    err = _err_buf()
    tail = (_fptr(rgb), _opt(cov, _fptr), _opt(count, _uptr), _opt(albedo, _fptr), _opt(normal, _fptr), C.byref(stats), C.byref(info), C.byref(multi),
            err, len(err))
    if device_ids is not None:
        ids = (C.c_int * len(device_ids))(*device_ids)
        _check(lib.ptr_multi_debug_adaptive_on(C.byref(desc), C.byref(settings), C.byref(params), ids, len(device_ids), *tail), err)
    else:
        _check(lib.ptr_render_multi_adaptive(C.byref(desc), C.byref(settings), C.byref(params), n_devices, int(verbose), *tail), err)
    return {"rgb": rgb, "cov": cov, "count": count, "albedo": albedo, "normal": normal, "stats": stats, "info": info, "multi": multi}


def multi_adaptive_debug_frame(samples: np.ndarray, params: PtrAdaptiveParams, device_ids):
    """ptr_multi_debug_adaptive_frame (tests): the partition loop of render_multi_adaptive on samples [maxSpp, H, W, 3 or 4] instead of a
    scene.  Returns (rgb [H, W, 3], cov [H, W, 6], count [H, W] uint32, info)."""
    samples = np.asarray(samples, dtype=np.float32)
    if samples.ndim != 4 or samples.shape[3] not in (3, 4) or samples.shape[0] < params.maxSpp:
        raise ValueError("multi_adaptive_debug_frame: samples must be [>= maxSpp, H, W, 3 or 4]")
    if samples.shape[3] == 3:
        samples = np.concatenate([samples, np.zeros(samples.shape[:3] + (1,), np.float32)], axis=3)
    samples = np.ascontiguousarray(samples)
    h, w = samples.shape[1], samples.shape[2]
    rgb = np.zeros((h, w, 3), dtype=np.float32)
    cov = np.zeros((h, w, 6), dtype=np.float32)
    count = np.zeros((h, w), dtype=np.uint32)
    info = PtrAdaptiveInfo()
    ids = (C.c_int * len(device_ids))(*device_ids)
    err = _err_buf()
    _check(load_library().ptr_multi_debug_adaptive_frame(w, h, C.byref(params), _fptr(samples), ids, len(device_ids), _fptr(rgb), _fptr(cov),
                                                         _uptr(count), C.byref(info), err, len(err)), err)
    return rgb, cov, count, info


class MultiFrame:
    """include/ptr_multi_frame.h: a resumable frame on several devices, continued call by call; made by multi_frame() or
    debug_multi_frame().  The calls mirror Frame's; the state, the images and every info are bit for bit those of a single-device Frame
    given the same calls, and a checkpoint (export_state / import_state) passes between the two and between device counts."""

    def __init__(self, handle: C.c_void_p, keepalive=None, devices=None):
        self._h = handle
        self._keepalive = keepalive
        self._devices = devices   # the device of every partition when the frame was made on an id list

    def _handle(self):
        if not self._h:
            raise PtrError("the frame is closed")
        return self._h

    def accumulate(self, spp: int) -> PtrRenderStats:
        """Every pixel gets `spp` more samples (the frame must be uniform)."""
        stats = PtrRenderStats()
        err = _err_buf()
        _check(load_library().ptr_multi_frame_accumulate(self._handle(), spp, C.byref(stats), err, len(err)), err)
        return stats

    def refine(self, params: PtrAdaptiveParams) -> Tuple[PtrRenderStats, PtrAdaptiveInfo]:
        """The resumable adaptive loop of Frame.refine in lock step over the partitions.  Returns (stats, info) of this call."""
        stats, info = PtrRenderStats(), PtrAdaptiveInfo()
        err = _err_buf()
        _check(load_library().ptr_multi_frame_refine(self._handle(), C.byref(params), C.byref(stats), C.byref(info), err, len(err)), err)
        return stats, info

    def info(self) -> PtrFrameInfo:
        out = PtrFrameInfo()
        if load_library().ptr_multi_frame_info(self._handle(), C.byref(out), None) != 0:
            raise PtrError("ptr_multi_frame_info failed")
        return out

    def multi_info(self) -> PtrMultiInfo:
        """The partitions of the last accumulate, refine or resolve."""
        out, multi = PtrFrameInfo(), PtrMultiInfo()
        if load_library().ptr_multi_frame_info(self._handle(), C.byref(out), C.byref(multi)) != 0:
            raise PtrError("ptr_multi_frame_info failed")
        return multi

    def resolve(self, want_cov: bool = True, want_count: bool = True, want_aovs: bool = False):
        """([H, W, 3] image, [H, W, 6] covariance of the pixel means, [H, W] uint32 samples per pixel), image order; with want_aovs also
        the first-hit feature buffers ([H, W, 4] albedo, [H, W, 4] normal) of the first partition's resident scene.  The state stays."""
        i = self.info()
        rgb = np.zeros((i.height, i.width, 3), dtype=np.float32)
        cov = np.zeros((i.height, i.width, 6), dtype=np.float32) if want_cov else None
        count = np.zeros((i.height, i.width), dtype=np.uint32) if want_count else None
        albedo = np.zeros((i.height, i.width, 4), dtype=np.float32) if want_aovs else None
        normal = np.zeros((i.height, i.width, 4), dtype=np.float32) if want_aovs else None
        err = _err_buf()
        _check(load_library().ptr_multi_frame_resolve(self._handle(), _fptr(rgb), _opt(cov, _fptr), _opt(count, _uptr), _opt(albedo, _fptr),
                                                      _opt(normal, _fptr), err, len(err)), err)
        return (rgb, cov, count, albedo, normal) if want_aovs else (rgb, cov, count)

    def resolve_device(self, d_rgb: int, d_cov: int = 0, d_count: int = 0, stream: int = 0) -> None:
        """resolve() into caller-owned image-order buffers on the frame's FIRST device, on `stream` of that device."""
        err = _err_buf()
        _check(load_library().ptr_multi_frame_resolve_device(self._handle(), C.c_void_p(d_rgb), C.c_void_p(d_cov or None),
                                                             C.c_void_p(d_count or None), C.c_void_p(stream or None), err, len(err)), err)

    def export_state(self) -> dict:
        """The checkpoint of Frame.export_state, image order, each pixel from its owner: it does not depend on the device count."""
        i = self.info()
        pixels = i.width * i.height
        st = {k: np.zeros((pixels, cols) if cols else pixels, dtype=dt) for k, cols, dt in FRAME_STATE}
        err = _err_buf()
        _check(load_library().ptr_multi_frame_export(self._handle(), _fptr(st["sum"]), _fptr(st["mean"]), _fptr(st["m"]), _uptr(st["n"]),
                                                     _fptr(st["e"]), err, len(err)), err)
        return st

    def import_state(self, state: dict) -> None:
        i = self.info()
        pixels = i.width * i.height
        st = {k: np.ascontiguousarray(state[k], dtype=dt).reshape((pixels, cols) if cols else pixels) for k, cols, dt in FRAME_STATE}
        err = _err_buf()
        _check(load_library().ptr_multi_frame_import(self._handle(), _fptr(st["sum"]), _fptr(st["mean"]), _fptr(st["m"]), _uptr(st["n"]),
                                                     _fptr(st["e"]), err, len(err)), err)

    def reset(self, settings: Optional[PtrSettings] = None) -> None:
        """The state back to zero on every device; `settings` of the same size replace the stored ones."""
        err = _err_buf()
        _check(load_library().ptr_multi_frame_reset(self._handle(), C.byref(settings) if settings is not None else None, err, len(err)), err)

    # ---- include/ptr_multi_dynamic.h: a frame made with dynamic=True is updated in place on all its devices.  The calls take what
    # DeviceScene's take, without the stream, and return PtrMultiUpdateInfo.as_dict().  reset() before accumulating the new pose.
    def is_dynamic(self) -> bool:
        return bool(load_library().ptr_multi_frame_is_dynamic(self._handle()))

    def dynamic_flags(self) -> int:
        return int(load_library().ptr_multi_frame_dynamic_flags(self._handle()))

    def _update(self, name: str, items, count: int, *more) -> dict:
        info = PtrMultiUpdateInfo()
        err = _err_buf()
        _check(getattr(load_library(), name)(self._handle(), items, count, *more, C.byref(info), err, len(err)), err)
        return info.as_dict()

    def set_mesh_transforms(self, transforms: dict) -> dict:
        return self._update("ptr_multi_frame_set_mesh_transforms", _transform_items(transforms), len(transforms))

    def set_mesh_vertices(self, meshes: dict) -> dict:
        items, keep = _vertex_items(meshes)
        return self._update("ptr_multi_frame_set_mesh_vertices", items, len(meshes))

    def set_spheres(self, spheres: dict) -> dict:
        return self._update("ptr_multi_frame_set_spheres", _sphere_items(spheres), len(spheres))

    def set_rects(self, rects: dict) -> dict:
        return self._update("ptr_multi_frame_set_rects", _rect_items(rects), len(rects))

    def set_mesh_vertices_device(self, meshes: dict, stream=None) -> dict:
        """ptr_multi_frame_set_mesh_vertices_device: torch tensors as DeviceScene.set_mesh_vertices_device takes them, all on one device,
        which need not be one of the frame's; they are read on `stream` of that device (None: torch's current stream there)."""
        items, device = _vertex_device_items(meshes, None)
        if device is None:
            raise PtrError("set_mesh_vertices_device: no tensor names a device")
        if stream is None:
            import torch   # (only here: the module itself does not need torch)

            stream = torch.cuda.current_stream(device).cuda_stream
        return self._update("ptr_multi_frame_set_mesh_vertices_device", items, len(meshes), device, C.c_void_p(stream))

    # ---- include/ptr_multi_appearance.h: DeviceScene's appearance calls on every partition, on static frames too.  They take what
    # DeviceScene's take, without the stream, and return PtrMultiAppearanceInfo.as_dict().  reset() before accumulating the edited scene.
    _device = None   # (for DeviceScene._device_pixels: the tensors of a device form may live on any device)

    def _appearance(self, name: str, *args) -> dict:
        info = PtrMultiAppearanceInfo()
        err = _err_buf()
        _check(getattr(load_library(), name)(self._handle(), *args, C.byref(info), err, len(err)), err)
        return info.as_dict()

    @staticmethod
    def _source_of(name: str, tensors, stream):
        """(src_device, stream) of a device form: the one device all its tensors are on, and torch's current stream there by default."""
        devices = {t.device.index for t in tensors}
        if len(devices) != 1:
            raise PtrError("%s: the tensors are on %d devices, not on one" % (name, len(devices)))
        device = devices.pop()
        if stream is None:
            import torch   # (only here: the module itself does not need torch)

            stream = torch.cuda.current_stream(device).cuda_stream
        return device, C.c_void_p(stream)

    def set_materials(self, materials: dict) -> dict:
        indices, items = DeviceScene._material_items(materials)
        return self._appearance("ptr_multi_frame_set_materials", indices, items, len(materials))

    def set_textures(self, textures: dict) -> dict:
        items, keep = DeviceScene._texture_items("set_textures", textures, DeviceScene._host_pixels)
        return self._appearance("ptr_multi_frame_set_textures", items, len(textures))

    def set_textures_device(self, textures: dict, stream=None) -> dict:
        """ptr_multi_frame_set_textures_device: torch tensors as DeviceScene.set_textures_device takes them, all on one device, which need
        not be one of the frame's; they are read on `stream` of that device (None: torch's current stream there)."""
        items, keep = DeviceScene._texture_items("set_textures_device", textures, lambda *a: DeviceScene._device_pixels(self, *a))
        device, stream = self._source_of("set_textures_device", keep, stream)
        return self._appearance("ptr_multi_frame_set_textures_device", items, len(textures), device, stream)

    def set_environment(self, pixels) -> dict:
        a, (h, w) = DeviceScene._host_pixels("set_environment", "the map", pixels)
        return self._appearance("ptr_multi_frame_set_environment", a.ctypes.data_as(C.c_void_p), w, h)

    def set_environment_device(self, pixels, stream=None) -> dict:
        """ptr_multi_frame_set_environment_device: a torch tensor on any visible device, read on `stream` of that device."""
        t, (h, w) = DeviceScene._device_pixels(self, "set_environment_device", "the map", pixels)
        device, stream = self._source_of("set_environment_device", [t], stream)
        return self._appearance("ptr_multi_frame_set_environment_device", C.c_void_p(t.data_ptr()), w, h, device, stream)

    def tree_cost(self) -> float:
        cost = C.c_double(0.0)
        err = _err_buf()
        _check(load_library().ptr_multi_frame_tree_cost(self._handle(), C.byref(cost), err, len(err)), err)
        return float(cost.value)

    def rebuild_tree(self, keep_if_better: bool = True) -> dict:
        """ptr_multi_frame_rebuild_tree: DeviceScene.rebuild_tree on every partition, which all reach the same tree."""
        info = PtrRebuildInfo()
        err = _err_buf()
        flags = PTR_REBUILD_KEEP_IF_BETTER if keep_if_better else 0
        _check(load_library().ptr_multi_frame_rebuild_tree(self._handle(), flags, C.byref(info), err, len(err)), err)
        return info.as_dict()

    def part_scene(self, p: int) -> "DeviceScene":
        """Partition p's scene, borrowed: it keeps the frame alive, its close() does nothing, and it refuses the update and rebuild
        calls (they go through the frame).  Rendering, temporal() and the arrays() / rebuild_arrays() probes may use it."""
        h = load_library().ptr_multi_frame_part_scene(self._handle(), p)
        if not h:
            raise PtrError("part_scene: the frame has no partition %d with a scene" % p)
        return _BorrowedScene(C.c_void_p(h), self._devices[p] if self._devices else p, self)

    def temporal(self, width: int, height: int, params: Optional["PtrTemporalParams"] = None, cov=None) -> "Temporal":
        """part_scene(0).temporal(...): a Temporal handle on the frame's first device, beside resolve_device."""
        return self.part_scene(0).temporal(width, height, params, cov)

    def close(self) -> None:
        if self._h:
            load_library().ptr_multi_frame_release(self._h)
            self._h = None
        self._keepalive = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def multi_frame(desc: PtrSceneDesc, settings: PtrSettings, n_devices: int = 0, device_ids=None, dynamic: bool = False, deformable: bool = False,
                primitives: bool = False, vertex_normals: bool = False) -> MultiFrame:
    """A resumable frame on several devices of this node (include/ptr_multi_frame.h): the scene is prepared once and uploaded to every
    device once, for the frame's life.  `device_ids` (tests) names the devices explicitly as render_multi_adaptive's does.
    dynamic (include/ptr_multi_dynamic.h): every device's scene is a dynamic scene and the frame's set_* / rebuild_tree calls update
    them in place; deformable / primitives / vertex_normals as DeviceScene takes them."""
    handle = C.c_void_p()
    err = _err_buf()
    lib = load_library()
    if (deformable or primitives or vertex_normals) and not dynamic:
        raise PtrError("deformable / primitives / vertex_normals need dynamic=True")
    flags = (PTR_DYNAMIC_DEFORMABLE if deformable else 0) | (PTR_DYNAMIC_PRIMITIVES if primitives else 0) | (PTR_DYNAMIC_VERTEX_NORMALS if vertex_normals else 0)
    devices = None
    if device_ids is not None:
        ids = (C.c_int * len(device_ids))(*device_ids)
        devices = [-(i + 1) if i < 0 else i for i in device_ids]
        if dynamic:
            _check(lib.ptr_multi_frame_debug_create_dynamic_on(C.byref(desc), C.byref(settings), flags, ids, len(device_ids), C.byref(handle), err, len(err)), err)
        else:
            _check(lib.ptr_multi_frame_debug_create_on(C.byref(desc), C.byref(settings), ids, len(device_ids), C.byref(handle), err, len(err)), err)
    elif dynamic:
        _check(lib.ptr_multi_frame_create_dynamic(C.byref(desc), C.byref(settings), n_devices, flags, C.byref(handle), err, len(err)), err)
    else:
        _check(lib.ptr_multi_frame_create(C.byref(desc), C.byref(settings), n_devices, C.byref(handle), err, len(err)), err)
    return MultiFrame(handle, devices=devices)


def debug_multi_check_update(desc: PtrSceneDesc, call: str, update: dict, deformable: bool = True, primitives: bool = True,
                             vertex_normals: bool = False) -> None:
    """ptr_multi_frame_debug_check_update (tests, no GPU): the host checks of MultiFrame.<call>(update) - set_mesh_transforms,
    set_mesh_vertices, set_spheres or set_rects - against a frame made from `desc` with these flags; raises PtrError with the call's
    own message when it would be refused."""
    kinds = {"set_mesh_transforms": (0, _transform_items), "set_mesh_vertices": (1, _vertex_items), "set_spheres": (2, _sphere_items),
             "set_rects": (3, _rect_items)}
    kind, make = kinds[call]
    made = make(update)   # (_vertex_items also returns the arrays its items point into: `made` keeps them until the call has returned)
    items = made[0] if isinstance(made, tuple) else made
    flags = (PTR_DYNAMIC_DEFORMABLE if deformable else 0) | (PTR_DYNAMIC_PRIMITIVES if primitives else 0) | (PTR_DYNAMIC_VERTEX_NORMALS if vertex_normals else 0)
    err = _err_buf()
    _check(load_library().ptr_multi_frame_debug_check_update(C.byref(desc), flags, kind, C.cast(items, C.c_void_p), len(update), err, len(err)), err)


def debug_multi_check_appearance(desc: PtrSceneDesc, call: str, update, primitives: bool = False) -> None:
    """ptr_multi_frame_debug_check_appearance (tests, no GPU): the host checks of MultiFrame.<call>(update) - set_materials, set_textures
    or set_environment, the look at every pixel component included - against a frame made from `desc`, static or (primitives) dynamic with
    PTR_DYNAMIC_PRIMITIVES; raises PtrError with the call's own message when it would be refused."""
    flags = PTR_DYNAMIC_PRIMITIVES if primitives else 0
    if call == "set_materials":
        indices, items = DeviceScene._material_items(update)
        args = (0, C.cast(indices, C.c_void_p), items, len(update), 0, 0)
    elif call == "set_textures":
        items, keep = DeviceScene._texture_items(call, update, DeviceScene._host_pixels)
        args = (1, C.cast(items, C.c_void_p), None, len(update), 0, 0)
    elif call == "set_environment":
        a, (h, w) = DeviceScene._host_pixels(call, "the map", update)
        args = (2, a.ctypes.data_as(C.c_void_p), None, 0, w, h)
    else:
        raise PtrError("debug_multi_check_appearance: no such call: %s" % call)
    err = _err_buf()
    _check(load_library().ptr_multi_frame_debug_check_appearance(C.byref(desc), flags, *args, err, len(err)), err)


def debug_multi_frame(samples: np.ndarray, device_ids) -> MultiFrame:
    """ptr_multi_frame_debug_create (tests): debug_frame() on the partitions `device_ids` names; samples [S, H, W, 3 or 4]."""
    samples = np.asarray(samples, dtype=np.float32)
    count, h, w = samples.shape[:3]
    x4 = np.zeros((count, h, w, 4), dtype=np.float32)
    x4[..., :3] = samples[..., :3]
    ids = (C.c_int * len(device_ids))(*device_ids)
    handle = C.c_void_p()
    err = _err_buf()
    _check(load_library().ptr_multi_frame_debug_create(w, h, _fptr(x4), count, ids, len(device_ids), C.byref(handle), err, len(err)), err)
    return MultiFrame(handle)


def decode_image(data: bytes) -> np.ndarray:
    """PNG / baseline JPEG bytes -> [H, W, 4] uint8 through the library's own decoders (ptr_host_decode_image)."""
    lib = load_library()
    w, h = C.c_uint32(), C.c_uint32()
    err = _err_buf()
    _check(lib.ptr_host_decode_image(data, len(data), None, 0, C.byref(w), C.byref(h), err, len(err)), err)
    out = np.zeros((h.value, w.value, 4), dtype=np.uint8)
    _check(lib.ptr_host_decode_image(data, len(data), out.ctypes.data_as(C.POINTER(C.c_uint8)), out.nbytes, C.byref(w), C.byref(h), err, len(err)), err)
    return out


def write_exr_aovs(path: str, rgb: np.ndarray, albedo: np.ndarray, normal: np.ndarray) -> None:
    """Beauty + first-hit albedo / normal / depth layers in one EXR (ptr_host_write_exr_aovs)."""
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    albedo = np.ascontiguousarray(albedo, dtype=np.float32)
    normal = np.ascontiguousarray(normal, dtype=np.float32)
    h, w = rgb.shape[0], rgb.shape[1]
    err = _err_buf()
    _check(load_library().ptr_host_write_exr_aovs(os.fsencode(path), _fptr(rgb), _fptr(albedo), _fptr(normal), w, h, err, len(err)), err)


# ----------------------------------------------------------------------------- post-processing (include/ptr_post.h)


def denoise(rgb: np.ndarray, albedo: np.ndarray, normal: np.ndarray, params: Optional[PtrDenoiseParams] = None, device: int = 0,
            return_ms: bool = False, cov: Optional[np.ndarray] = None):
    """The edge-avoiding a-trous wavelet filter of include/ptr_post.h on host arrays: rgb [H, W, 3] and the first-hit feature buffers of
    DeviceScene.render_aovs ([H, W, 4] each) -> [H, W, 3] float32 (with return_ms: and the milliseconds its kernels took).
    cov ([H, W, 6], DeviceScene.render_image_cov): the filter takes its variance from it (include/ptr_stats.h ptr_denoise_cov)."""
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    albedo = np.ascontiguousarray(albedo, dtype=np.float32)
    normal = np.ascontiguousarray(normal, dtype=np.float32)
    if rgb.ndim != 3 or rgb.shape[2] != 3 or albedo.shape != rgb.shape[:2] + (4,) or normal.shape != albedo.shape:
        raise ValueError("denoise: rgb must be [H, W, 3], albedo and normal [H, W, 4]")
    lib = load_library()
    params = params if params is not None else PtrDenoiseParams.defaults()
    out = np.empty_like(rgb)
    ms = C.c_double(0.0)
    err = _err_buf()
    if cov is not None:
        cov = np.ascontiguousarray(cov, dtype=np.float32)
        if cov.shape != rgb.shape[:2] + (6,):
            raise ValueError("denoise: cov must be [H, W, 6]")
        _check(lib.ptr_denoise_cov(_fptr(rgb), _fptr(albedo), _fptr(normal), _fptr(cov), rgb.shape[1], rgb.shape[0], C.byref(params), device,
                                   _fptr(out), C.byref(ms), err, len(err)), err)
    else:
        _check(lib.ptr_denoise(_fptr(rgb), _fptr(albedo), _fptr(normal), rgb.shape[1], rgb.shape[0], C.byref(params), device, _fptr(out),
                               C.byref(ms), err, len(err)), err)
    return (out, float(ms.value)) if return_ms else out


def denoise_device(d_rgb: int, d_albedo: int, d_normal: int, width: int, height: int, params: Optional[PtrDenoiseParams] = None,
                   d_out: Optional[int] = None, stream: int = 0, d_cov: int = 0) -> None:
    """The same filter on device buffers given as raw pointers (a torch tensor's data_ptr()), asynchronous on `stream`; d_out defaults
    to d_rgb (in place).  d_cov (width * height * 6 floats): the variance comes from it (ptr_denoise_cov_device)."""
    lib = load_library()
    params = params if params is not None else PtrDenoiseParams.defaults()
    err = _err_buf()
    out = C.c_void_p(d_rgb if d_out is None else d_out)
    if d_cov:
        _check(lib.ptr_denoise_cov_device(C.c_void_p(d_rgb), C.c_void_p(d_albedo), C.c_void_p(d_normal), C.c_void_p(d_cov), width, height,
                                          C.byref(params), out, C.c_void_p(stream), err, len(err)), err)
    else:
        _check(lib.ptr_denoise_device(C.c_void_p(d_rgb), C.c_void_p(d_albedo), C.c_void_p(d_normal), width, height, C.byref(params), out,
                                      C.c_void_p(stream), err, len(err)), err)


def denoise_timed(d_rgb: int, d_albedo: int, d_normal: int, width: int, height: int, d_out: int, params: Optional[PtrDenoiseParams] = None,
                  runs: int = 20, warmup: int = 5) -> Tuple[list, list]:
    """ptr_denoise_timed: (mean ms of prepare, every a-trous pass and finish over `runs` runs, 1 where the LDS-tiled kernel ran)."""
    lib = load_library()
    params = params if params is not None else PtrDenoiseParams.defaults()
    n = params.iterations + 2
    ms, tiled = (C.c_double * n)(), (C.c_uint32 * n)()
    err = _err_buf()
    _check(lib.ptr_denoise_timed(C.c_void_p(d_rgb), C.c_void_p(d_albedo), C.c_void_p(d_normal), width, height, C.byref(params),
                                 C.c_void_p(d_out), runs, warmup, ms, tiled, err, len(err)), err)
    return [float(v) for v in ms], [int(v) for v in tiled]


def adaptive_debug_round(width: int, height: int, params: PtrAdaptiveParams, n_before: int, samples: np.ndarray, active: np.ndarray,
                         state: dict, last_sub_pass: bool = True):
    """ptr_adaptive_debug_round (tests): one round - or one sub-pass of it - of update -> select -> compact on synthetic data.  samples
    [round_spp, len(active), 4]; state = {"sum": [H*W, 3], "mean": [H*W, 3], "m": [H*W, 6], "n": [H*W] uint32, "e": [H*W]}.  Returns (new
    state, next list as handed back - its first `next_count` words are the kept entries, the rest are 0xFFFFFFFF - , next_count)."""
    samples = np.ascontiguousarray(samples, dtype=np.float32)
    active = np.ascontiguousarray(active, dtype=np.uint32).reshape(-1)
    out = {k: np.ascontiguousarray(state[k], dtype=np.uint32 if k == "n" else np.float32).copy() for k in ("sum", "mean", "m", "n", "e")}
    nxt = np.full(active.size, 0xFFFFFFFF, dtype=np.uint32)
    nxt_count = C.c_uint32(0)
    err = _err_buf()
    _check(load_library().ptr_adaptive_debug_round(width, height, C.byref(params), n_before, samples.shape[0], int(last_sub_pass), _uptr(active),
                                                   active.size, _fptr(samples), _fptr(out["sum"]), _fptr(out["mean"]), _fptr(out["m"]),
                                                   _uptr(out["n"]), _fptr(out["e"]), _uptr(nxt), C.byref(nxt_count), err, len(err)), err)
    return out, nxt, int(nxt_count.value)


def assemble_bands(parts_out, width: int, height: int) -> np.ndarray:
    """Interleave per-partition band buffers ([bands*BAND_ROWS, W, C] each - C = 3 for images, 6 for covariances - , band b of part p =
    image band p + b*P)."""
    parts = len(parts_out)
    R = BAND_ROWS
    img = np.zeros((((height + R - 1) // R) * R, width, parts_out[0].shape[2] if parts else 3), dtype=np.float32)
    for p, buf in enumerate(parts_out):
        nb = buf.shape[0] // R
        for b in range(nb):
            g = p + b * parts
            img[g * R:(g + 1) * R] = buf[b * R:(b + 1) * R]
    return img[:height]


def write_image(path: str, rgb: np.ndarray, fmt: str = "pfm", rgba_exr: bool = False, tonemap: int = 1,
                aces_variant: int = 0, exposure: float = 0.0, reinhard_white: float = 1.5) -> None:
    lib = load_library()
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    h, w = rgb.shape[0], rgb.shape[1]
    err = _err_buf()
    _check(lib.ptr_host_write_image(os.fsencode(path), fmt.encode(), _fptr(rgb), w, h, int(rgba_exr), tonemap,
                                    aces_variant, exposure, reinhard_white, err, len(err)), err)


def write_exr_multilayer(path: str, rgb: np.ndarray, sample_counts: Optional[np.ndarray] = None,
                         colorspace: str = "Linear sRGB") -> None:
    """RGBA EXR with a planar SAMPLES channel (per-pixel sample counts), or plain RGBA when sample_counts is None."""
    lib = load_library()
    rgb = np.ascontiguousarray(rgb, dtype=np.float32)
    h, w = rgb.shape[0], rgb.shape[1]
    counts = None
    if sample_counts is not None:
        counts = np.ascontiguousarray(sample_counts, dtype=np.float32).reshape(h, w)
    err = _err_buf()
    _check(lib.ptr_host_write_exr_multilayer(os.fsencode(path), _fptr(rgb), w, h, _fptr(counts) if counts is not None else None,
                                             colorspace.encode(), err, len(err)), err)


def read_pfm(path: str) -> np.ndarray:
    lib = load_library()
    w, h = C.c_uint32(), C.c_uint32()
    if lib.ptr_host_read_pfm(os.fsencode(path), None, 0, C.byref(w), C.byref(h)) != 0:
        raise PtrError(f"cannot read PFM header: {path}")
    out = np.zeros((h.value, w.value, 3), dtype=np.float32)
    if lib.ptr_host_read_pfm(os.fsencode(path), _fptr(out), out.size, C.byref(w), C.byref(h)) != 0:
        raise PtrError(f"cannot read PFM data: {path}")
    return out


# ----------------------------------------------------------------------------- device-function probes (tests)


def debug_eval_bsdf(material: PtrMaterial, settings: PtrSettings, inputs: np.ndarray) -> np.ndarray:
    return _batch(load_library().ptr_debug_eval_bsdf, (C.byref(material), C.byref(settings)), inputs, np.float32, 12, [((5,), np.float32)])


def debug_sample_bsdf(material: PtrMaterial, settings: PtrSettings, inputs: np.ndarray, front: np.ndarray,
                      states: np.ndarray):
    front = np.ascontiguousarray(front, dtype=np.uint32)
    states = np.ascontiguousarray(states, dtype=np.uint32)
    return _batch(load_library().ptr_debug_sample_bsdf, (C.byref(material), C.byref(settings)), inputs, np.float32, 9,
                  [((8,), np.float32), ((), np.uint32)], more=(_uptr(front), _uptr(states)))


def debug_sample_lobes(material: PtrMaterial, settings: PtrSettings, inputs: np.ndarray, front: np.ndarray, states: np.ndarray):
    """ptr_debug_sample_lobes on the inputs of debug_sample_bsdf: ([n, 3] {lobe, lobe roughness, isDelta}, [n, 8] sample as
    debug_sample_bsdf returns it, [n] rng states after sampling, the material's environment-lighting roughness)."""
    front = np.ascontiguousarray(front, dtype=np.uint32)
    states = np.ascontiguousarray(states, dtype=np.uint32)
    env_rough = C.c_float()
    out, sample, out_states = _batch(load_library().ptr_debug_sample_lobes, (C.byref(material), C.byref(settings)), inputs, np.float32, 9,
                                     [((3,), np.float32), ((8,), np.float32), ((), np.uint32)], more=(_uptr(front), _uptr(states)),
                                     tail=(C.byref(env_rough),))
    return out, sample, out_states, float(env_rough.value)


def debug_sss_walk_begin(material: PtrMaterial, settings: PtrSettings, inputs: np.ndarray, states: np.ndarray):
    """ptr_debug_sss_walk_begin: sssWalkBegin on inputs [n, 12] {point, entry normal, wo, incident} with random states [n]:
    ([n, 16] rows of SSS_BEGIN_FIELDS, the states afterwards)."""
    states = np.ascontiguousarray(states, dtype=np.uint32)
    return _batch(load_library().ptr_debug_sss_walk_begin, (C.byref(material), C.byref(settings)), inputs, np.float32, 12,
                  [((16,), np.float32), ((), np.uint32)], more=(_uptr(states),))


def debug_sss_walk_step(material: PtrMaterial, settings: PtrSettings, rows: np.ndarray, states: np.ndarray):
    """ptr_debug_sss_walk_step: sssWalkStep with maxSteps = settings.sssMaxSteps on rows [n, 20] (SSS_STEP_IN_FIELDS) with random states
    [n]: ([n, 24] rows of SSS_STEP_FIELDS, the states afterwards)."""
    states = np.ascontiguousarray(states, dtype=np.uint32)
    return _batch(load_library().ptr_debug_sss_walk_step, (C.byref(material), C.byref(settings)), rows, np.float32, 20,
                  [((24,), np.float32), ((), np.uint32)], more=(_uptr(states),))


def debug_env_mips(rgba: np.ndarray):
    """Host-side (no GPU): the environment mip chain PTR_METAL_ENV_LOD builds - a list of [h_l, w_l, 4] float32 levels, level 0 first."""
    rgba = np.ascontiguousarray(rgba, dtype=np.float32)
    h, w = rgba.shape[0], rgba.shape[1]
    lib = load_library()
    levels = C.c_uint32(0)
    if lib.ptr_debug_env_mips(_fptr(rgba), w, h, None, 0, C.byref(levels)) != 0:
        raise PtrError("ptr_debug_env_mips failed")
    sizes = [(max(h >> l, 1), max(w >> l, 1)) for l in range(levels.value)]
    out = np.zeros(sum(a * b for a, b in sizes) * 4, dtype=np.float32)
    if lib.ptr_debug_env_mips(_fptr(rgba), w, h, _fptr(out), out.size, C.byref(levels)) != 0:
        raise PtrError("ptr_debug_env_mips failed")
    chain, at = [], 0
    for a, b in sizes:
        chain.append(out[at:at + a * b * 4].reshape(a, b, 4))
        at += a * b * 4
    return chain


def debug_camera_rays(settings: PtrSettings, xys: np.ndarray):
    return _batch(load_library().ptr_debug_camera_rays, (C.byref(settings),), xys, np.uint32, 3, [((6,), np.float32), ((), np.uint32)])


def debug_env_distribution(rgba: np.ndarray) -> dict:
    """Host-side environment importance tables (no GPU needed)."""
    rgba = np.ascontiguousarray(rgba, dtype=np.float32)
    h, w = rgba.shape[0], rgba.shape[1]
    pdf = np.zeros((h, w), np.float32)
    ca = np.zeros((h, w), np.uint32)
    ct = np.zeros((h, w), np.float32)
    ma = np.zeros(h, np.uint32)
    mt = np.zeros(h, np.float32)
    total = C.c_float()
    rc = load_library().ptr_debug_env_distribution(_fptr(rgba), w, h, _fptr(pdf), _uptr(ca), _fptr(ct), _uptr(ma), _fptr(mt),
                                                   C.byref(total))
    if rc != 0:
        raise PtrError("environment map has no positive radiance")
    return dict(pdf=pdf, cond_alias=ca, cond_threshold=ct, marg_alias=ma, marg_threshold=mt, total=total.value)


GEOMETRY_FIELDS = ("nodes", "leaves", "triangles_referenced", "spheres_referenced", "max_depth", "max_leaf_size",
                   "unreferenced", "multiply_referenced", "box_violations", "quant_violations", "bad_refs", "triangles",
                   "spheres", "sah_cost_milli", "build_ms", "quantized_usable")


def background_cull(settings: PtrSettings, scene: Optional["DeviceScene"] = None, desc: Optional[PtrSceneDesc] = None, part: int = 0,
                    parts: int = 1, count: bool = False) -> dict:
    """ptr_background_debug_cull (host only): which pixels a plain frame keeps out of the path pool.  The bounds are those of the device
    scene `scene`, or those of `desc` prepared on the host.  rect = (x0, x1, y0, y1): pixels outside [x0, x1) x [y0, y1) are background."""
    out = (C.c_uint32 * 8)()
    bounds = (C.c_double * 7)()
    err = _err_buf()
    _check(load_library().ptr_background_debug_cull(scene._h if scene is not None else None, C.byref(desc) if desc is not None else None,
                                                    C.byref(settings), part, parts, int(count), out, bounds, err, len(err)), err)
    return {"culling": bool(out[0]), "rect": (int(out[1]), int(out[2]), int(out[3]), int(out[4])), "traced": int(out[5]),
            "background": int(out[6]), "lo": np.array(bounds[0:3]), "hi": np.array(bounds[3:6]), "bounds_valid": bool(bounds[6])}


def debug_scene_geometry(desc: PtrSceneDesc, leaf_max: int = 0) -> dict:
    """Host-side (no GPU): build the BVH / leaf-order arrays exactly as ptr_scene_upload does and validate them."""
    out = (C.c_uint64 * 16)()
    err = _err_buf()
    _check(load_library().ptr_debug_scene_geometry(C.byref(desc), leaf_max, out, err, len(err)), err)
    g = dict(zip(GEOMETRY_FIELDS, [int(v) for v in out]))
    word = g["quantized_usable"]
    g["oversize"] = (word >> 8) & 0xFF                   # triangles kept out of the tree (tested first by every ray)
    g["wide_nodes"] = (word >> 16) & 0xFFFFFFFF          # four-wide nodes of the persistent traversal kernels
    g["wide_depth"] = (word >> 48) & 0xFF               # levels of their (by-area) tree
    g["wide_problems"] = word >> 63                      # bad references / primitives not reached exactly once through them
    g["quantized_usable"] = word & 0xFF
    return g


def rect_update(index: int, corner, edgeU, edgeV, normal) -> PtrRectUpdate:
    """A PtrRectUpdate with the w words the scene loader stores (SceneResources::storeRectangleOriented): 0, 1/|U|^2, 1/|V|^2, and the
    unit normal with dot(normal, corner); float32 arithmetic in the loader's order."""
    f = np.float32
    c, u, v, n = (np.asarray(a, f).reshape(3) for a in (corner, edgeU, edgeV, normal))

    def dot(a, b):
        return f(f(f(a[0] * b[0]) + f(a[1] * b[1])) + f(a[2] * b[2]))

    out = PtrRectUpdate()
    out.rectIndex = int(index)
    with np.errstate(all="ignore"):
        unit = n / np.sqrt(dot(n, n)) if dot(n, n) > 0 else n
        out.corner[:] = [float(c[0]), float(c[1]), float(c[2]), 0.0]
        out.edgeU[:] = [float(u[0]), float(u[1]), float(u[2]), float(f(1.0) / dot(u, u))]
        out.edgeV[:] = [float(v[0]), float(v[1]), float(v[2]), float(f(1.0) / dot(v, v))]
        out.normalAndPlane[:] = [float(unit[0]), float(unit[1]), float(unit[2]), float(dot(unit, c))]
    return out


def debug_dynamic_update_rows(desc: PtrSceneDesc, update) -> list:
    """ptr_debug_dynamic_update_rows (host only): what ptr_scene_set_spheres / ptr_scene_set_rects would scatter for one PtrSphereUpdate /
    PtrRectUpdate on `desc`, as [(array name of SCATTER_ARRAYS, row, float32[4])]."""
    lib = load_library()
    err = _err_buf()
    kind = 0 if isinstance(update, PtrSphereUpdate) else 1
    n = C.c_uint64(0)
    _check(lib.ptr_debug_dynamic_update_rows(C.byref(desc), kind, C.byref(update), None, 0, C.byref(n), err, len(err)), err)
    buf = np.zeros(n.value * 5, np.uint32)
    _check(lib.ptr_debug_dynamic_update_rows(C.byref(desc), kind, C.byref(update), buf.ctypes.data_as(C.c_void_p), buf.nbytes, C.byref(n), err, len(err)), err)
    rows, dest = buf[: n.value * 4].view(np.float32).reshape(-1, 4), buf[n.value * 4:]
    return [(SCATTER_ARRAYS[int(d) >> 28], int(d) & 0x0FFFFFFF, rows[i]) for i, d in enumerate(dest)]


def debug_vertex_adjacency(desc: PtrSceneDesc, mesh: int) -> Tuple[np.ndarray, np.ndarray]:
    """ptr_debug_vertex_adjacency (host only): the vertex adjacency PTR_DYNAMIC_VERTEX_NORMALS keeps for mesh `mesh` of `desc`, as (row offsets
    [vertexCount + 1], entries [corners]): an entry is the number, within the mesh, of a description triangle that names the vertex."""
    lib = load_library()
    err = _err_buf()
    size = C.c_uint64(0)
    _check(lib.ptr_debug_vertex_adjacency(C.byref(desc), mesh, None, 0, C.byref(size), err, len(err)), err)
    buf = np.zeros(size.value // 4, np.uint32)
    _check(lib.ptr_debug_vertex_adjacency(C.byref(desc), mesh, buf.ctypes.data_as(C.c_void_p), buf.nbytes, C.byref(size), err, len(err)), err)
    n = int(desc.meshes[mesh].vertexCount) + 1
    return buf[:n], buf[n:]


def _sized_array(call, dtype, what=None) -> np.ndarray:
    """What every probe that writes into a caller's buffer is asked twice: call(None, 0, size_ref) for the size in bytes, then
    call(out, cap_bytes, size_ref) with a buffer of that size.  Returns the flat array of `dtype`.  `call` raises on a failure itself
    or, with `what`, returns the probe's code: a code other than 0 raises "<what> failed", with the code when it is the call that fills."""
    size = C.c_uint64(0)
    rc = call(None, 0, C.byref(size))
    if what and rc != 0:
        raise PtrError("%s failed" % what)
    buf = np.zeros(size.value // np.dtype(dtype).itemsize, dtype)
    rc = call(buf.ctypes.data_as(C.c_void_p), buf.nbytes, C.byref(size))
    if what and rc != 0:
        raise PtrError("%s failed (%d)" % (what, rc))
    return buf


def debug_dynamic_tables(desc: PtrSceneDesc, names=None) -> dict:
    """ptr_debug_dynamic_tables (host only): the tables ptr_scene_upload_dynamic prepares for `desc` as numpy arrays; "info" as a dict."""
    lib = load_library()
    out = {}
    for name in (names or DYNAMIC_TABLES):
        which, dtype, shape = DYNAMIC_TABLES[name]
        err = _err_buf()
        buf = _sized_array(lambda o, cap, size: _check(lib.ptr_debug_dynamic_tables(C.byref(desc), which, o, cap, size, err, len(err)), err), dtype)
        out[name] = buf.reshape(2, 3) if name == "grid" else buf.reshape((-1,) + shape)
    if "info" in out:
        out["info"] = dict(zip(DYNAMIC_TABLE_INFO, (int(v) for v in out["info"])))
    return out


def debug_rebuild_tables(nodes: np.ndarray, names=None) -> dict:
    """ptr_debug_rebuild_tables (host only): the builder's own functions on a preorder array of 64 B float nodes, as numpy arrays ("sah" a
    float, "wideDepth" and "depthCheck" ints).  Raises PtrError for what the probe refuses ("depthCheck": a tree too deep to install)."""
    lib = load_library()
    nodes = np.ascontiguousarray(nodes, np.float32).reshape(-1, 16)
    out = {}
    for name in (names or [n for n in REBUILD_TABLES if n != "depthCheck"]):
        which, dtype, shape = REBUILD_TABLES[name]
        err = _err_buf()
        buf = _sized_array(lambda o, cap, size: _check(lib.ptr_debug_rebuild_tables(_fptr(nodes), len(nodes), which, o, cap, size, err, len(err)), err), dtype)
        if name == "grid":
            out[name] = buf.reshape(2, 3)
        elif name in ("sah", "wideDepth", "depthCheck"):
            out[name] = buf[0].item()
        else:
            out[name] = buf.reshape((-1,) + shape)
    return out


def walk_stack_depths(desc: PtrSceneDesc, rays: np.ndarray) -> np.ndarray:
    """Host-side (no GPU), ptr_debug_walk_stack_depths: per ray [n, 8], the most entries the four-wide walk's traversal stack holds (entries
    past the 16 LDS levels are in the HBM spill area)."""
    return _batch(load_library().ptr_debug_walk_stack_depths, (C.byref(desc),), rays, np.float32, 8, [((), np.uint32)])
