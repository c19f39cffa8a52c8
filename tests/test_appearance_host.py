"""CPU tests of include/ptr_appearance.h: the exported surface and the ctypes mirrors, what the entry points refuse without a device, the
numpy restatements of tests/appearance_ref.py against the host probes, and the stand-alone sanitizer program.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import appearance_ref as ref
import appearance_scenes as aps
import light_scenes as ls
import traversal_scenes as ts

pt = ts.pt
ROOT = ts.ROOT

FUNCTIONS = {"ptr_scene_set_materials": 8, "ptr_scene_set_textures": 7, "ptr_scene_set_textures_device": 7, "ptr_scene_set_environment": 8,
             "ptr_scene_set_environment_device": 8, "ptr_debug_appearance_arrays": 5}


# --------------------------------------------------------------------------- the surface
def test_library_exports_every_function_of_the_appearance_header():
    text = open(os.path.join(ROOT, "include", "ptr_appearance.h")).read()
    text = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    found = {name: (kind, args.count(",") + 1) for kind, name, args in re.findall(r"\b(int|uint32_t)\s+(ptr_[a-z_]+)\s*\(([^()]*)\)\s*;", text)}
    assert found == {name: ("int", count) for name, count in FUNCTIONS.items()}
    assert tuple(found) == pt.APPEARANCE_SYMBOLS, "header order"
    lib = pt.load_library()
    for name, (_, count) in found.items():
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == count and fn.restype is C.c_int, name


def test_appearance_symbols_are_in_no_other_table_and_every_table_keeps_its_size():
    tables = {"ABI": 0, "DEBUG": 0, "POST": 4, "STATS": 5, "ADAPTIVE": 4, "MULTI": 5, "FRAME": 11, "MULTI_FRAME": None, "DYNAMIC": 5, "DEFORM": 6,
              "DEFORM_DEVICE": 3, "BACKGROUND": None, "TEMPORAL": None, "TEMPORAL_COV": 6, "REBUILD": None, "MULTI_DYNAMIC": None, "PBR_HIT": None,
              "SSS_WALK": None, "PATH_STATE": None}
    others = set()
    for name, size in tables.items():
        table = getattr(pt, name + "_SYMBOLS")
        others |= set(table)
        if size:
            assert len(table) == size, name
    assert len(pt.ABI_SYMBOLS) + len(pt.DEBUG_SYMBOLS) == 48
    assert not set(pt.APPEARANCE_SYMBOLS) & others and len(set(pt.APPEARANCE_SYMBOLS)) == len(pt.APPEARANCE_SYMBOLS) == 6
    # every *_SYMBOLS table of the module is one of those: a new one would have to be listed here
    assert {n[:-8] for n in dir(pt) if n.endswith("_SYMBOLS")} == set(tables) | {"APPEARANCE"}


def test_python_mirrors_have_the_headers_layout(tmp_path):
    info_members = ["totalSeconds", "stagingMs", "kernelMs", "rowsRekeyed", "texelsWritten", "lightsBefore", "lightsAfter", "envSampling", "pad"]
    tex_members = ["textureIndex", "width", "height", "wrapS", "wrapT", "filter", "rgba"]
    src = tmp_path / "sizes.cpp"
    src.write_text('#include <cstddef>\n#include <cstdio>\n#include "ptr_appearance.h"\nint main() { std::printf("%zu %zu", sizeof(PtrAppearanceInfo), sizeof(PtrTextureUpdate));\n'
                   + "".join('std::printf(" %%zu", offsetof(PtrAppearanceInfo, %s));\n' % m for m in info_members)
                   + "".join('std::printf(" %%zu", offsetof(PtrTextureUpdate, %s));\n' % m for m in tex_members)
                   + 'std::printf(" %d %d\\n", (int)PTR_APPEARANCE_ENV_MAX_DIM, (int)PTR_APPEARANCE_SCALARS); }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["g++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(s) for s in subprocess.run([str(exe)], check=True, stdout=subprocess.PIPE, text=True).stdout.split()]
    info, tex = pt.PtrAppearanceInfo, pt.PtrTextureUpdate
    want = [C.sizeof(info), C.sizeof(tex)] + [getattr(info, m).offset for m in info_members] + [getattr(tex, m).offset for m in tex_members]
    assert got == want + [pt.PTR_APPEARANCE_ENV_MAX_DIM, pt.APPEARANCE_ARRAYS["scalars"][0]]
    assert got[:2] == [96, 32] and pt.PTR_APPEARANCE_ENV_MAX_DIM == 4096
    assert sorted(v[0] for v in pt.APPEARANCE_ARRAYS.values()) == list(range(12)) and len(pt.APPEARANCE_SCALARS) == 6


def test_what_the_entry_points_refuse_without_a_device():
    lib = pt.load_library()
    err = C.create_string_buffer(256)
    m = pt.PtrMaterial()
    idx = (C.c_uint32 * 1)(0)
    tex = (pt.PtrTextureUpdate * 1)()
    px = (C.c_float * 4)()
    calls = {"ptr_scene_set_materials": (idx, m, 1), "ptr_scene_set_textures": (tex, 1), "ptr_scene_set_textures_device": (tex, 1),
             "ptr_scene_set_environment": (px, 1, 1), "ptr_scene_set_environment_device": (px, 1, 1)}
    for name, args in calls.items():
        err.value = b""
        assert getattr(lib, name)(None, *args, None, None, err, len(err)) == 1
        assert err.value == name.encode() + b": null argument"
        assert getattr(lib, name)(None, *args, None, None, None, 0) == 1   # and no message buffer is needed
    size = C.c_uint64(7)
    assert lib.ptr_debug_appearance_arrays(None, 0, None, 0, C.byref(size)) == 1 and size.value == 7
    # the upload knows no new flag: bit 8 stays refused by both entry points
    out = C.c_void_p()
    desc = pt.PtrSceneDesc()
    assert lib.ptr_scene_upload_dynamic_ex(C.byref(desc), 0, 8, C.byref(out), err, len(err)) == 1 and b"unknown flag" in err.value
    assert lib.ptr_scene_upload_deformable(C.byref(desc), 0, 8, C.byref(out), err, len(err)) == 1 and b"unknown flag" in err.value


# --------------------------------------------------------------------------- the restatements against the host probes
def test_light_table_reference_equals_the_preparation(tmp_path):
    hosts = [ls.light_scene(tmp_path, n) for n in (1, 2, 8, 9)] + [aps.lights_scene(tmp_path), ts.scene_a()]
    counts = []
    for host in hosts:
        d = host.desc
        index, lights = ref.light_table(d)
        rows = pt.debug_dynamic_tables(d, ["rectLights"])["rectLights"]
        assert len(rows) == len(lights)
        for row, (rect, emission, two_sided) in zip(rows, lights):
            assert row[2, 3:4].view(np.uint32)[0] == rect and np.array_equal(row[4, :3], emission) and row[1, 3] == two_sided and row[4, 3] == 0
            assert np.array_equal(row[0, :3], np.array(list(d.rects[rect].corner)[:3], np.float32))
        assert (index >= 0).sum() == len(lights) and list(index[index >= 0]) == list(range(len(lights)))
        counts.append(len(lights))
    assert counts[:5] == [1, 2, 8, 9, 2]
    # an edit changes the table the way the header says: emission 0 and a type change take a light out, emission puts one in
    host = aps.lights_scene(tmp_path)
    for edit, want in (({3: aps.material_of(host.desc, 3, emission=(0, 0, 0))}, [2]),
                       ({2: aps.material_of(host.desc, 2, typeEta=(0.0,))}, [3]),
                       ({4: aps.material_of(host.desc, 4, emission=(1, 2, 3))}, list(range(2, 11)))):
        edited = aps.Edited(host.desc, host, materials=edit)
        index, lights = ref.light_table(edited.desc)
        assert [l[0] for l in lights] == want
        rows = pt.debug_dynamic_tables(edited.desc, ["rectLights"])["rectLights"]
        assert [int(r[2, 3:4].view(np.uint32)[0]) for r in rows] == want


def test_mip_reference_equals_the_host_chain():
    rng = np.random.default_rng(2)
    for w, h in aps.TEXTURE_SIZES + ((3, 5), (16, 8), (64, 32), (2, 1)):
        level0 = rng.random((h, w, 4), dtype=np.float32)
        got, want = ref.mip_chain(level0), pt.debug_env_mips(level0)
        assert len(got) == len(want) == min(max(w, h).bit_length(), 16), (w, h)
        for a, b in zip(got, want):
            assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), (w, h)


def test_alias_reference_equals_the_host_tables():
    """Maps of one row: the cell weight is sin(pi / 2) pi 2 pi / w with a sine of exactly 1, so the conditional table's probabilities can be
    restated without the host's sine; the marginal table has one entry."""
    rng = np.random.default_rng(4)
    for w in (1, 2, 3, 7, 64, 257, 1000):
        rgb = np.exp(rng.uniform(np.log(1e-3), np.log(50.0), (1, w, 3))).astype(np.float32)
        if w > 3:
            rgb[0, w // 2] = 0.0          # thresholds of exactly 0
            rgb[0, w // 3] = 1e4          # one entry that stays on the over-full list for a long run
        rgba = np.concatenate([rgb, np.ones((1, w, 1), np.float32)], axis=2)
        tables = pt.debug_env_distribution(rgba)
        cell, weight, row, total = ref.env_tables(rgba)
        assert np.float32(tables["total"]) == total
        inv = np.float32(1) / row[0]
        thr, alias = ref.alias_table((weight[0] * inv).astype(np.float32))
        assert np.array_equal(alias, tables["cond_alias"][0]) and np.array_equal(thr.view(np.uint32), tables["cond_threshold"][0].view(np.uint32)), w
        assert tables["marg_alias"][0] == 0 and tables["marg_threshold"][0] == 1
        pdf = ((weight[0] / total) / cell[0]).astype(np.float32)
        assert np.array_equal(pdf.view(np.uint32), tables["pdf"][0].view(np.uint32)), w
    # the tails: equal probabilities are all over-full and never enter the loop
    thr, alias = ref.alias_table(np.full(8, 0.125, np.float32))
    assert np.array_equal(thr, np.ones(8, np.float32)) and list(alias) == list(range(8))


# --------------------------------------------------------------------------- the sanitizer program
def test_the_stand_alone_host_check_builds_and_runs_clean(tmp_path):
    """tools/appearance_host_check.cpp with -fsanitize=address,undefined: a stand-alone program on the CPU with its own main and the
    sanitizers' runtimes linked in."""
    csrc = os.path.join(ROOT, "metal-pathtracer-arm64_amd", "csrc")
    exe = tmp_path / "appearance_host_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-pthread",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(csrc, "host"), "-I", os.path.join(csrc, "kernels"),
                    os.path.join(ROOT, "tools", "appearance_host_check.cpp"), os.path.join(csrc, "host", "appearance_host.cpp"),
                    os.path.join(csrc, "host", "scene_geometry.cpp"), os.path.join(csrc, "host", "bvh_builder.cpp"), os.path.join(csrc, "host", "knobs.cpp"),
                    "-o", str(exe)], check=True)
    res = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert res.returncode == 0, res.stdout
    lines = res.stdout.strip().split("\n")
    assert lines[0] == "0 materials, 0 rectangles: ok" and lines[-2] == "512 materials, 128 rectangles: ok" and len(lines) == 31
    assert lines[-1] == "mip levels and cell weights: ok"
    assert "runtime error" not in res.stdout and "AddressSanitizer" not in res.stdout
