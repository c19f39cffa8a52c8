"""CPU tests of the surface of appearance updates for frames on several devices (include/ptr_multi_appearance.h): the exported
functions and their ctypes table, PtrMultiAppearanceInfo against a compiled program, what is refused before a frame is looked at, and -
through ptr_multi_frame_debug_check_appearance, which runs step 1 of a call on records made from the description on the host - every
refusal include/ptr_appearance.h lists for the three host forms, in the single-device words behind the multi-frame name.

A frame is created on devices only, so what is refused before a frame is looked at is called with a made-up handle that must never be
looked behind.  src_device at or past the visible count, the device forms and the guards of a borrowed scene need devices:
tests/test_gpu_multi_appearance.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import appearance_scenes as aps
import light_scenes as ls
import traversal_scenes as ts

pt = ts.pt
ROOT = ts.ROOT
HEADER = os.path.join(ROOT, "include", "ptr_multi_appearance.h")

COUNTS = {"ptr_multi_frame_set_materials": 7, "ptr_multi_frame_set_textures": 6, "ptr_multi_frame_set_environment": 7,
          "ptr_multi_frame_set_textures_device": 8, "ptr_multi_frame_set_environment_device": 9, "ptr_multi_frame_debug_check_appearance": 10}
FRAME = C.c_void_p(0x1000)
METAL_TYPE = 1


def test_library_exports_every_function_of_the_header():
    text = open(HEADER).read()
    assert '#include "ptr_appearance.h"' in text and '#include "ptr_multi_frame.h"' in text and "Kernels: none of its own" in text
    text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    found = {name: (kind, args.count(",") + 1) for kind, name, args in re.findall(r"\b(int|uint32_t)\s+(ptr_[a-z_]+)\s*\(([^()]*)\)\s*;", text)}
    assert found == {name: ("int", count) for name, count in COUNTS.items()}
    assert tuple(found) == pt.MULTI_APPEARANCE_FUNCTIONS, "header order"
    lib = pt.load_library()
    for name, (_, count) in found.items():
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == count and fn.restype is C.c_int, name
    others = set()
    for table in (n for n in dir(pt) if n.endswith("_SYMBOLS")):
        others |= set(getattr(pt, table))
    assert not set(pt.MULTI_APPEARANCE_FUNCTIONS) & others
    assert len(pt.MULTI_DYNAMIC_SYMBOLS) == 13 and len(pt.APPEARANCE_SYMBOLS) == 6 and len(pt.MULTI_FRAME_SYMBOLS) == 12, "the other surfaces are what they were"


def test_python_mirrors_device_scene_and_the_borrowed_scene_refuses():
    setters = ("set_materials", "set_textures", "set_textures_device", "set_environment", "set_environment_device")
    for name in setters:
        assert callable(getattr(pt.MultiFrame, name)) and callable(getattr(pt.DeviceScene, name)), name
        assert getattr(pt.MultiFrame, name) is not getattr(pt.DeviceScene, name)
    borrowed = pt._BorrowedScene(C.c_void_p(0x1000), 0, None)   # (the refusal comes before the handle is looked at)
    for name in setters:
        with pytest.raises(pt.PtrError, match="through its MultiFrame"):
            getattr(borrowed, name)({})
    assert callable(pt.debug_multi_check_appearance)


def test_info_layout_against_a_compiled_program(tmp_path):
    fields = ["parts", "stagedParts", "hostStagedBytes", "totalSeconds", "distributeSeconds", "partSeconds", "first"]
    src = tmp_path / "sizes.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "ptr_multi_appearance.h"\nint main() { std::printf("%zu %zu'
                   + " %zu" * len(fields) + '\\n", sizeof(PtrMultiAppearanceInfo), sizeof(PtrAppearanceInfo), '
                   + ", ".join("offsetof(PtrMultiAppearanceInfo, %s)" % f for f in fields) + "); }\n")
    exe = tmp_path / "sizes"
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(s) for s in subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    info = pt.PtrMultiAppearanceInfo
    assert [n for n, _ in info._fields_] == fields
    assert got == [C.sizeof(info), C.sizeof(pt.PtrAppearanceInfo)] + [getattr(info, f).offset for f in fields]
    assert got[0] == 8 + 8 + 16 + 8 * pt.MULTI_MAX_PARTS + C.sizeof(pt.PtrAppearanceInfo)
    # the header's struct names the same members in the same order
    body = re.search(r"typedef struct PtrMultiAppearanceInfo \{(.*?)\} PtrMultiAppearanceInfo;", open(HEADER).read(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b(\w+)(?:\[\w+\])?;", body) == fields
    d = info().as_dict()
    assert {"parts", "stagedParts", "hostStagedBytes", "distributeSeconds", "partSeconds", "rowsRekeyed", "lightsAfter", "envSampling"} <= set(d)


def _refused(name, *args, words=None):
    err = C.create_string_buffer(256)
    rc = getattr(pt.load_library(), name)(*args, err, len(err))
    message = err.value.decode()
    assert rc == 1 and message.startswith(name + ": ") and (words is None or words in message), (name, rc, message)
    return message


def test_what_is_refused_before_a_frame_is_looked_at():
    idx, mat, tex, px = (C.c_uint32 * 1)(0), pt.PtrMaterial(), (pt.PtrTextureUpdate * 1)(), (C.c_float * 4)()
    info = pt.PtrMultiAppearanceInfo()
    info.parts = 77
    by = C.byref(info)
    name = "ptr_multi_frame_set_materials"
    _refused(name, None, idx, mat, 1, by, words="null argument")
    _refused(name, FRAME, None, mat, 1, by, words="null material list")
    _refused(name, FRAME, idx, None, 1, by, words="null material list")
    _refused(name, FRAME, idx, mat, 0, by, words="count is 0")
    name = "ptr_multi_frame_set_textures"
    _refused(name, None, tex, 1, by, words="null argument")
    _refused(name, FRAME, None, 1, by, words="null texture list")
    _refused(name, FRAME, tex, 0, by, words="count is 0")
    name = "ptr_multi_frame_set_textures_device"
    _refused(name, None, tex, 1, 0, None, by, words="null argument")
    _refused(name, FRAME, None, 1, 0, None, by, words="null texture list")
    _refused(name, FRAME, tex, 0, 0, None, by, words="count is 0")
    _refused(name, FRAME, tex, 1, -1, None, by, words="no such HIP device")
    name = "ptr_multi_frame_set_environment"
    _refused(name, None, px, 1, 1, by, words="null argument")
    _refused(name, FRAME, None, 1, 1, by, words="null pixels")
    name = "ptr_multi_frame_set_environment_device"
    _refused(name, None, px, 1, 1, 0, None, by, words="null argument")
    _refused(name, FRAME, None, 1, 1, 0, None, by, words="null pixels")
    _refused(name, FRAME, px, 1, 1, -1, None, by, words="no such HIP device")
    assert info.parts == 77, "a refused call leaves the info alone"
    # and no message buffer is needed
    assert pt.load_library().ptr_multi_frame_set_materials(None, idx, mat, 1, None, None, 0) == 1


def _raw(desc, flags, kind, items, materials, count, w=0, h=0):
    err = C.create_string_buffer(512)
    rc = pt.load_library().ptr_multi_frame_debug_check_appearance(C.byref(desc) if desc is not None else None, flags, kind, items, materials, count, w, h, err, len(err))
    return rc, err.value.decode()


def test_material_checks_in_the_single_device_words(tmp_path):
    """lights_scene: rectangles use materials 0, 2, 3 and 4; material 1 is the sphere's and the mesh's.  No textures."""
    host = aps.lights_scene(tmp_path)
    d = host.desc
    check = pt.debug_multi_check_appearance
    name = "^ptr_multi_frame_set_materials: "
    sphere = {1: aps.material_of(d, 1, typeEta=(float(METAL_TYPE),))}
    light = {3: aps.material_of(d, 3, emission=(0.0, 0.0, 0.0))}
    # accepted lists return 0: a material no rectangle uses on a static frame, and any with PTR_DYNAMIC_PRIMITIVES
    check(d, "set_materials", sphere)
    check(d, "set_materials", sphere, primitives=True)
    check(d, "set_materials", {**sphere, **light}, primitives=True)
    # the rectangle-material rule: refused without PTR_DYNAMIC_PRIMITIVES (a static frame, and a dynamic one without the flag), accepted with it
    words = "a rectangle uses a named material and the scene does not keep its rectangles \\(upload it with ptr_scene_upload_dynamic_ex and PTR_DYNAMIC_PRIMITIVES\\)$"
    with pytest.raises(pt.PtrError, match=name + words):
        check(d, "set_materials", light)
    idx, items = pt.DeviceScene._material_items(light)
    rc, message = _raw(d, pt.PTR_DYNAMIC_DEFORMABLE, 0, idx, items, 1)
    assert rc == 1 and re.match(name + words, message)
    check(d, "set_materials", light, primitives=True)
    refused = [({d.materialCount: aps.material_of(d, 0)}, "material index %d out of range \\(the scene has %d materials\\)" % (d.materialCount, d.materialCount)),
               ({1: aps.material_of(d, 1, emission=(float("nan"),))}, "material 1 has a non-finite entry"),
               ({1: aps.material_of(d, 1, baseColorRoughness=(0.5, float("inf")))}, "material 1 has a non-finite entry"),
               ({1: aps.material_of(d, 1, textureIndices0=(0,))}, "material 1 names texture 0 and the scene was uploaded without textures"),
               ({1: aps.material_of(d, 1, textureIndices1=(aps.NONE, 3))}, "material 1 names texture 3 and the scene was uploaded without textures")]
    for call, words in refused:
        for primitives in (False, True):
            with pytest.raises(pt.PtrError, match=name + words):
                check(d, "set_materials", call, primitives=primitives)
    lib, err = pt.load_library(), C.create_string_buffer(256)
    # an index named twice cannot be said with a dict: through the C interface; and the probe's own arguments
    twice = (C.c_uint32 * 2)(1, 1)
    two = (pt.PtrMaterial * 2)()
    for k in range(2):
        C.memmove(C.byref(two[k]), C.byref(d.materials[1]), C.sizeof(pt.PtrMaterial))
    assert _raw(d, 0, 0, twice, two, 2) == (1, "ptr_multi_frame_set_materials: material index 1 named twice")
    assert _raw(d, 0, 0, None, two, 2) == (1, "ptr_multi_frame_set_materials: null material list")
    assert _raw(d, 0, 0, twice, None, 2) == (1, "ptr_multi_frame_set_materials: null material list")
    assert _raw(d, 0, 0, twice, two, 0) == (1, "ptr_multi_frame_set_materials: count is 0")
    assert _raw(None, 0, 0, twice, two, 1) == (1, "ptr_multi_frame_debug_check_appearance: null argument")
    assert _raw(d, 0, 3, twice, two, 1) == (1, "ptr_multi_frame_debug_check_appearance: no such kind")
    rc, message = _raw(d, 8, 0, twice, two, 1)
    assert rc == 1 and message.startswith("ptr_multi_frame_debug_check_appearance: ") and "unknown flag" in message
    # ptr_multi_frame_debug_check_update is what it was
    assert lib.ptr_multi_frame_debug_check_update(C.byref(d), 3, 4, twice, 1, err, len(err)) == 1 and err.value.endswith(b": no such kind")


def test_material_texture_indices_on_a_textured_scene():
    quads = aps.Quads(aps.TEXTURE_SIZES[:-1])
    d = quads.desc
    n = d.textureCount
    check = pt.debug_multi_check_appearance
    check(d, "set_materials", {0: aps.material_of(d, 0, textureIndices0=(n - 1, aps.NONE))})
    with pytest.raises(pt.PtrError, match="^ptr_multi_frame_set_materials: material 2 names texture %d \\(the scene has %d textures\\)$" % (n, n)):
        check(d, "set_materials", {2: aps.material_of(d, 2, textureIndices1=(n,))})


def test_texture_checks_in_the_single_device_words(tmp_path):
    sizes = aps.TEXTURE_SIZES[:-1]   # (without the 65536 x 1 texture)
    quads = aps.Quads(sizes)
    d = quads.desc
    check = pt.debug_multi_check_appearance
    name = "^ptr_multi_frame_set_textures: "
    rng = np.random.default_rng(3)
    new = {i: rng.random((h, w, 4), dtype=np.float32) for i, (w, h) in enumerate(sizes)}
    check(d, "set_textures", new)
    check(d, "set_textures", {3: (new[3], 2, 1, 0)}, primitives=True)
    bad = new[3].copy()
    bad[5, 5, 2] = np.inf
    nan = new[5].copy()
    nan[15, 6, 3] = np.nan
    refused = [({len(sizes): new[3]}, "texture index %d out of range \\(the scene has %d textures\\)" % (len(sizes), len(sizes))),
               ({3: new[4]}, "texture 3 was uploaded at 8 x 8, not 16 x 2$"),
               ({2: new[2][:, :4]}, "texture 2 was uploaded at 5 x 3, not 4 x 3$"),
               ({3: bad}, "texture 3 has a non-finite component$"),
               ({0: new[0], 5: nan}, "texture 5 has a non-finite component$")]
    for call, words in refused:
        with pytest.raises(pt.PtrError, match=name + words):
            check(d, "set_textures", call)
    items = (pt.PtrTextureUpdate * 2)()
    for k in range(2):
        items[k].textureIndex, items[k].width, items[k].height, items[k].rgba = 3, 8, 8, new[3].ctypes.data
    assert _raw(d, 0, 1, items, None, 2) == (1, "ptr_multi_frame_set_textures: texture index 3 named twice")
    items[1].textureIndex, items[1].width, items[1].height, items[1].rgba = 4, 16, 2, None
    assert _raw(d, 0, 1, items, None, 2) == (1, "ptr_multi_frame_set_textures: texture 4 has null pixels")
    assert _raw(d, 0, 1, items, None, 1) == (0, "")
    assert _raw(d, 0, 1, None, None, 1) == (1, "ptr_multi_frame_set_textures: null texture list")
    assert _raw(d, 0, 1, items, None, 0) == (1, "ptr_multi_frame_set_textures: count is 0")
    # a scene without textures
    plain = aps.lights_scene(tmp_path)
    with pytest.raises(pt.PtrError, match=name + "the scene has no textures$"):
        check(plain.desc, "set_textures", {0: new[3]})


def test_environment_checks_in_the_single_device_words(tmp_path):
    w, h = 16, 8
    host, old = ls.env_scene(tmp_path, ls.env_map("noise", w, h), "env_checks")
    d = host.desc
    check = pt.debug_multi_check_appearance
    name = "^ptr_multi_frame_set_environment: "
    lit = old * np.float32(0.5)
    black = np.zeros_like(old)
    check(d, "set_environment", lit)
    check(d, "set_environment", black)   # (no positive radiance is not an error)
    check(d, "set_environment", lit, primitives=True)
    bad = lit.copy()
    bad[3, 4, 1] = np.nan
    for arg, words in ((lit[:, :8], "the map was uploaded at 16 x 8, not 8 x 8$"), (lit[:4], "the map was uploaded at 16 x 8, not 16 x 4$"),
                       (bad, "the map has a non-finite component$")):
        with pytest.raises(pt.PtrError, match=name + words):
            check(d, "set_environment", np.ascontiguousarray(arg))
    assert _raw(d, 0, 2, None, None, 0, w, h) == (1, "ptr_multi_frame_set_environment: null pixels")
    # a scene without a map
    plain = aps.lights_scene(tmp_path)
    with pytest.raises(pt.PtrError, match=name + "the scene was uploaded without an environment map$"):
        check(plain.desc, "set_environment", lit)
    # a map above PTR_APPEARANCE_ENV_MAX_DIM: the same description under a map of 4097 x 1
    wide = pt.PtrSceneDesc()
    C.memmove(C.byref(wide), C.byref(d), C.sizeof(pt.PtrSceneDesc))
    pixels = np.ones((1, pt.PTR_APPEARANCE_ENV_MAX_DIM + 1, 4), np.float32)
    wide.envRgba, wide.envWidth, wide.envHeight = pixels.ctypes.data_as(C.POINTER(C.c_float)), pixels.shape[1], 1
    with pytest.raises(pt.PtrError, match=name + "a map of 4097 x 1 is above the 4096 entries an alias table may have here$"):
        check(wide, "set_environment", pixels)
