"""Appearance updates for frames on several devices (include/ptr_multi_appearance.h) on the device: a MultiFrame given the calls of
MultiFrame.set_materials / set_textures[_device] / set_environment[_device] against ONE single-device DeviceScene given the same calls,
and once per test against a fresh upload of the edited description (appearance_scenes.Edited).  Every comparison of arrays, images and
infos is exact (bit patterns).

64x40 pixels, depth 4, 4 spp: five 8-row bands, so three partitions own 2 / 2 / 1 of them.  Device lists (test_gpu_multi_dynamic.py's):
one partition, three partitions on device 0, two partitions of which the second is forced through pinned host memory, and every visible
device where there is more than one.  With one device the peer path (hipMemcpyPeerAsync) is not executed: the in-place path and the
staged path are."""
import ctypes as C
import os

import numpy as np
import pytest
import torch      # before the library is loaded: the library then binds to the HIP runtime torch brought, and the two share the device

import appearance_scenes as aps
import deform_scenes as dsc
import light_scenes as ls
import traversal_scenes as ts
from test_gpu_appearance import LAMBERT, LIGHT_TYPE, METAL_TYPE, SSS_TYPE, assert_same_scene, assert_tables_are_the_hosts, by_meta, new_map, upload, words
from test_gpu_multi_dynamic import H, LIST_IDS, LISTS, SPP, W, arrays_of, info_of, make, on, outputs, same_outputs, settings_of
from test_gpu_rebuild import same_arrays

pt = ts.pt
pytestmark = pytest.mark.gpu
GOLDEN = ts.GOLDEN
ENV_ARRAYS = ["envRgba", "envCond", "envMarg", "envPdf", "scalars"]


def staged_of(ids):
    return sum(1 for i in ids if i < 0)


def both_semantics(host):
    return [settings_of(host, 0), settings_of(host, aps.METAL)]


def same_on_every_partition(frame, ids, dev, settings, what, geometry=True, tree=True):
    """Every partition's appearance arrays, scalars, scene arrays, info and shade_kernel_set are the scene's; geometry: a dynamic scene's
    rebuild arrays too (device pointers excepted)."""
    want = arrays_of(dev) if geometry else None
    for p in range(len(ids)):
        label = "%s, partition %d of %s" % (what, p, ids)
        scene = frame.part_scene(p)
        assert_same_scene(scene, dev, settings, label, renders=False, tree=tree)
        if geometry:
            same_arrays(arrays_of(scene), want, label)


def appearance_of(frame, ids, names=None):
    return [frame.part_scene(p).appearance_arrays(names) for p in range(len(ids))]


def assert_unchanged(frame, ids, before, what, names=None):
    for p, (a, b) in enumerate(zip(before, appearance_of(frame, ids, names))):
        for k in a:
            assert (a[k] == b[k]) if k == "scalars" else np.array_equal(a[k], b[k]), (what, p, k)


def fan_out(info, ids, what):
    assert info["parts"] == len(ids) and len(info["partSeconds"]) == len(ids) and min(info["partSeconds"]) > 0, what
    assert 0 < info["distributeSeconds"] <= info["totalSeconds"] and max(info["partSeconds"]) <= info["totalSeconds"], what


# --------------------------------------------------------------------------------------------------------------------- 1. materials
@pytest.mark.parametrize("ids", LISTS, ids=LIST_IDS)
def test_every_kind_of_material_edit_on_every_partition(tmp_path, ids):
    host = aps.lights_scene(tmp_path)
    settings = both_semantics(host)
    frame, dev = make(host, ids, s=settings[0], primitives=True)
    try:
        assert dev.info()["triangles"] == 23 and host.desc.rectCount == 11
        same_on_every_partition(frame, ids, dev, settings, "uploaded")
        m = float
        steps = [("colour only", dict(m1=dict(baseColorRoughness=(0.9, 0.1, 0.2))), (0, 2, 2)),
                 ("Lambert to metal on a sphere and a mesh", dict(m1=dict(typeEta=(m(METAL_TYPE),), baseColorRoughness=(0.9, 0.8, 0.5, 0.2))), (1, 2, 2)),
                 ("Lambert to metal on two rectangles", dict(m0=dict(typeEta=(m(METAL_TYPE),), baseColorRoughness=(0.8, 0.8, 0.8, 0.4))), (4, 2, 2)),
                 ("a light's emission changes", dict(m2=dict(emission=(1.0, 2.0, 3.0))), (0, 2, 2)),
                 ("a light goes out by emission 0", dict(m3=dict(emission=(0.0, 0.0, 0.0))), (0, 2, 1)),
                 ("the last light goes out by type", dict(m2=dict(typeEta=(m(LAMBERT),))), (2, 1, 0)),
                 ("two rectangles become lights in one call", dict(m2=dict(typeEta=(m(LIGHT_TYPE),)), m3=dict(emission=(2.0, 6.0, 3.0))), (2, 0, 2)),
                 ("nine lights: the settle flag goes off", dict(m4=dict(emission=(4.0, 4.0, 4.0))), (0, 2, 9)),
                 ("back to two", dict(m4=dict(emission=(0.0, 0.0, 0.0))), (0, 9, 2)),
                 ("the random-walk flag on", dict(m1=dict(typeEta=(m(SSS_TYPE),), sssParams=(0.1, 1.0, 0.0, 0.0))), None),
                 ("the random-walk flag off", dict(m1=dict(sssParams=(0.1, 0.0, 0.0, 0.0))), None)]
        materials = {}
        for what, members, figures in steps:
            current = aps.Edited(host.desc, host, materials=materials)
            call = {int(k[1:]): aps.material_of(current.desc, int(k[1:]), **v) for k, v in members.items()}
            want, got = dev.set_materials(call), frame.set_materials(call)
            materials.update(call)
            same_on_every_partition(frame, ids, dev, settings, what)
            for field in ("rowsRekeyed", "lightsBefore", "lightsAfter"):
                assert got[field] == want[field], (what, field)
            if figures:
                assert (got["rowsRekeyed"], got["lightsBefore"], got["lightsAfter"]) == figures, what
            fan_out(got, ids, what)
            assert got["hostStagedBytes"] == 0 and got["stagedParts"] == 0, what
            scalars = frame.part_scene(len(ids) - 1).appearance_arrays(["scalars"])["scalars"]
            if what.startswith("nine lights"):
                assert scalars["settleRectLights"] == 0
            if what.startswith("back to two"):
                assert scalars["settleRectLights"] == 1
            if what.startswith("the random-walk flag"):
                assert scalars["hasRandomWalkMaterial"] == (1 if what.endswith("on") else 0)
        fresh = upload(aps.Edited(host.desc, host, materials=materials))
        for p in range(len(ids)):
            assert_same_scene(frame.part_scene(p), fresh, settings, "the fresh upload of every edit, partition %d" % p, renders=False)
        fresh.close()
    finally:
        frame.close()
        dev.close()


# --------------------------------------------------------------------------------------------------------------------- 2. static frames
def test_a_static_frame_takes_a_material_edit(tmp_path):
    ids = [0, 0, 0]
    host = aps.static_scene(tmp_path)
    settings = both_semantics(host)
    frame, dev = make(host, ids, s=settings[0], dynamic=False)
    try:
        assert not frame.is_dynamic()
        call = {0: aps.material_of(host.desc, 0, typeEta=(float(METAL_TYPE),)), 1: aps.material_of(host.desc, 1, emission=(1.0, 5.0, 2.0))}
        want, got = dev.set_materials(call), frame.set_materials(call)
        assert got["rowsRekeyed"] == want["rowsRekeyed"] == 1 and got["parts"] == 3
        same_on_every_partition(frame, ids, dev, settings, "static: the mesh turns to metal", geometry=False)
        fresh = upload(aps.Edited(host.desc, host, materials=call), dynamic=False)
        for p in range(3):
            assert_same_scene(frame.part_scene(p), fresh, settings, "static, the fresh upload, partition %d" % p, renders=False)
        # ... and renders it: the frame's image is the single-device frame's on the edited scene
        single = dev.frame(settings[0])
        frame.reset()
        for t in (single, frame):
            t.accumulate(SPP)
        same_outputs(outputs(frame), outputs(single, dev, settings[0]), "a static frame after the edit")
        single.close()
        # the calls of ptr_multi_dynamic.h stay refused
        with pytest.raises(pt.PtrError, match="^ptr_multi_frame_set_mesh_transforms: the scene is not dynamic"):
            frame.set_mesh_transforms({0: np.eye(4)})
        fresh.close()
    finally:
        frame.close()
        dev.close()


def test_a_static_frame_refuses_a_rectangles_material(tmp_path):
    ids = [0, 0, 0]
    host = aps.lights_scene(tmp_path)
    settings = both_semantics(host)
    frame, dev = make(host, ids, s=settings[0], dynamic=False)
    try:
        before = appearance_of(frame, ids)
        tris = [frame.part_scene(p).arrays(["tris"])["tris"].copy() for p in range(3)]
        with pytest.raises(pt.PtrError) as e:
            dev.set_materials({3: aps.material_of(host.desc, 3, emission=(0.0, 0.0, 0.0))})
        single_words = str(e.value).split(": ", 1)
        assert single_words[0] == "ptr_scene_set_materials" and "PTR_DYNAMIC_PRIMITIVES" in single_words[1]
        with pytest.raises(pt.PtrError) as e:
            frame.set_materials({3: aps.material_of(host.desc, 3, emission=(0.0, 0.0, 0.0))})
        assert str(e.value) == "ptr_multi_frame_set_materials: " + single_words[1]
        assert_unchanged(frame, ids, before, "after the refusal")
        for p in range(3):
            assert np.array_equal(words(tris[p]), words(frame.part_scene(p).arrays(["tris"])["tris"]))
        # a material no rectangle uses is accepted
        call = {1: aps.material_of(host.desc, 1, baseColorRoughness=(0.3, 0.3, 0.9))}
        dev.set_materials(call)
        frame.set_materials(call)
        same_on_every_partition(frame, ids, dev, settings, "a material no rectangle uses", geometry=False)
    finally:
        frame.close()
        dev.close()


# --------------------------------------------------------------------------------------------------------------------- 3. textures
SIZES = aps.TEXTURE_SIZES[:-1]   # (1,1) (1,7) (5,3) (8,8) (16,2) (7,16)


def quads_settings(quads):
    base = pt.HostScene.load(os.path.join(GOLDEN, "textured.scene"), GOLDEN)
    out = []
    for metal in (False, True):
        s = quads.settings(base.settings_for(), metal)
        s.width, s.height, s.maxDepth = W, H, 4
        out.append(s)
    return out


def new_textures(quads, seed, rewrap=3):
    rng = np.random.default_rng(seed)
    new = {}
    for i, (w, h) in enumerate(SIZES):
        old = quads.desc.textures[i]
        pixels = np.exp(rng.uniform(-4.0, 2.0, (h, w, 4))).astype(np.float32)
        new[i] = (pixels, (old.wrapS + 1) % 3, (old.wrapT + 2) % 3, 1 - old.filter) if i == rewrap else (pixels, old.wrapS, old.wrapT, old.filter)
    return new


def same_textures(frame, ids, want_scene, what):
    want = want_scene.appearance_arrays(["texels", "texInfo"])
    for p in range(len(ids)):
        got = frame.part_scene(p).appearance_arrays(["texels", "texInfo"])
        for k in want:
            assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, p, k)


@pytest.mark.parametrize("ids", LISTS, ids=LIST_IDS)
def test_texture_updates_from_host_and_device_pixels(ids):
    quads = aps.Quads(SIZES)
    settings = quads_settings(quads)
    frame = pt.multi_frame(quads.desc, settings[1], device_ids=ids)
    dev = pt.DeviceScene(quads.desc, 0, keepalive=quads)
    payload = sum(w * h * 16 for w, h in SIZES)
    try:
        # the host form: every texture, wrap and filter changed on texture 3
        new = new_textures(quads, 9)
        want, got = dev.set_textures(new), frame.set_textures(new)
        fresh = pt.DeviceScene(aps.Edited(quads.desc, quads, textures=new).desc, 0, keepalive=quads)
        same_textures(frame, ids, fresh, "host pixels")
        same_on_every_partition(frame, ids, dev, settings, "host pixels", geometry=False)
        fan_out(got, ids, "host pixels")
        assert got["hostStagedBytes"] == payload and got["stagedParts"] == 0 and got["texelsWritten"] == want["texelsWritten"]
        # the device form: tensors on device 0, other pixels, wrap and filter changed on texture 1
        other = new_textures(quads, 10, rewrap=1)
        tensors = {i: (on(v[0]),) + v[1:] for i, v in other.items()}
        want, got = dev.set_textures_device(tensors), frame.set_textures_device(tensors)
        fresh2 = pt.DeviceScene(aps.Edited(quads.desc, quads, textures=other).desc, 0, keepalive=quads)
        same_textures(frame, ids, fresh2, "device pixels")
        same_on_every_partition(frame, ids, dev, settings, "device pixels", geometry=False)
        fan_out(got, ids, "device pixels")
        assert got["hostStagedBytes"] == 0 and got["stagedParts"] == staged_of(ids) and got["texelsWritten"] == want["texelsWritten"]
        # two of the textures only: the payload is theirs
        two = {2: new[2], 5: new[5]}
        got = frame.set_textures(two)
        assert got["hostStagedBytes"] == (5 * 3 + 7 * 16) * 16
        dev.set_textures(two)
        # a NaN texel: refused with the texture's index, by the host form in step 1 and by the device form after the device check
        kept = appearance_of(frame, ids, ["texels", "texInfo"])
        bad = other[3][0].copy()
        bad[5, 5, 2] = np.nan
        with pytest.raises(pt.PtrError, match="^ptr_multi_frame_set_textures: texture 3 has a non-finite component$"):
            frame.set_textures({0: new[0], 3: bad})
        with pytest.raises(pt.PtrError, match="^ptr_multi_frame_set_textures_device: texture 3 has a non-finite component$"):
            frame.set_textures_device({0: on(new[0][0]), 3: on(bad)})
        # a host-memory pointer given to the device form: the single-device words
        items, keep = pt.DeviceScene._texture_items("set_textures", {3: new[3][0]}, pt.DeviceScene._host_pixels)
        lib, err = pt.load_library(), C.create_string_buffer(256)
        assert lib.ptr_scene_set_textures_device(dev._h, items, 1, None, None, err, len(err)) == 1
        single_words = err.value.decode().split(": ", 1)[1]
        assert single_words.startswith("the pixel array of texture 3 is ") and "host memory" in single_words
        assert lib.ptr_multi_frame_set_textures_device(frame._h, items, 1, 0, None, None, err, len(err)) == 1
        assert err.value.decode() == "ptr_multi_frame_set_textures_device: " + single_words
        assert_unchanged(frame, ids, kept, "after the refusals", ["texels", "texInfo"])
        # an accepted call afterwards equals a fresh upload
        again = new_textures(quads, 11, rewrap=5)
        frame.set_textures(again)
        fresh3 = pt.DeviceScene(aps.Edited(quads.desc, quads, textures=again).desc, 0, keepalive=quads)
        same_textures(frame, ids, fresh3, "accepted after the refusals")
        for s in (fresh, fresh2, fresh3):
            s.close()
    finally:
        frame.close()
        dev.close()


# --------------------------------------------------------------------------------------------------------------------- 4. environment
ENV_CASES = [(1, 1, "noise"), (3, 5, "noise"), (64, 32, "black_row")]


def same_environment(frame, ids, dev, rgba, what):
    want = dev.appearance_arrays(ENV_ARRAYS)
    for p in range(len(ids)):
        scene = frame.part_scene(p)
        assert_tables_are_the_hosts(scene, rgba)
        got = scene.appearance_arrays(ENV_ARRAYS)
        for k in want:
            assert (got[k] == want[k]) if k == "scalars" else np.array_equal(got[k], want[k]), (what, p, k)


@pytest.mark.parametrize("ids", LISTS, ids=LIST_IDS)
@pytest.mark.parametrize("w,h,kind", ENV_CASES, ids=["%dx%d" % c[:2] for c in ENV_CASES])
def test_environment_updates_from_host_and_device_pixels(tmp_path, w, h, kind, ids):
    host, old = ls.env_scene(tmp_path, ls.env_map("noise", w, h), "menv_%d_%d" % (w, h))
    settings = both_semantics(host)
    frame, dev = make(host, ids, s=settings[0], dynamic=False)
    try:
        rgba = new_map(w, h, kind, 21)
        want, got = dev.set_environment(rgba), frame.set_environment(rgba)
        same_environment(frame, ids, dev, rgba, "host pixels")
        fresh = pt.DeviceScene(aps.Edited(host.desc, host, env=rgba).desc, 0, keepalive=host)
        for p in range(len(ids)):
            assert_same_scene(frame.part_scene(p), fresh, settings, "host pixels, the fresh upload, partition %d" % p, renders=False)
        fresh.close()
        fan_out(got, ids, "host pixels")
        assert got["hostStagedBytes"] == w * h * 16 and got["stagedParts"] == 0
        assert got["envSampling"] == want["envSampling"] == 1 and got["texelsWritten"] == want["texelsWritten"] == w * h
        other = new_map(w, h, kind, 22)
        want, got = dev.set_environment_device(on(other)), frame.set_environment_device(on(other))
        same_environment(frame, ids, dev, other, "device pixels")
        same_on_every_partition(frame, ids, dev, settings, "device pixels", geometry=False)
        fan_out(got, ids, "device pixels")
        assert got["hostStagedBytes"] == 0 and got["stagedParts"] == staged_of(ids) and got["envSampling"] == 1
    finally:
        frame.close()
        dev.close()


@pytest.mark.parametrize("ids", LISTS, ids=LIST_IDS)
def test_a_black_map_turns_sampling_off_on_every_partition(tmp_path, ids):
    w, h = 16, 8
    host, _ = ls.env_scene(tmp_path, ls.env_map("noise", w, h), "menv_black")
    settings = both_semantics(host)
    frame, dev = make(host, ids, s=settings[0], dynamic=False)
    try:
        black, lit = new_map(w, h, "black", 1), new_map(w, h, "noise", 2)
        dev.set_environment(black)
        info = frame.set_environment(black)
        assert info["envSampling"] == 0
        same_on_every_partition(frame, ids, dev, settings, "black", geometry=False)
        for got in appearance_of(frame, ids, ["envCond", "scalars"]):
            assert got["envCond"].size == 0 and got["scalars"]["envSampling"] == 0
        dev.set_environment(lit)
        info = frame.set_environment_device(on(lit))
        assert info["envSampling"] == 1
        same_environment(frame, ids, dev, lit, "lit again")
        # refusals: another size, a NaN from either form; every partition unchanged
        before = appearance_of(frame, ids)
        bad = lit.copy()
        bad[3, 4, 1] = np.nan
        for call, arg, name, text in ((frame.set_environment, np.ascontiguousarray(lit[:, :8]), "ptr_multi_frame_set_environment", "the map was uploaded at 16 x 8, not 8 x 8"),
                                      (frame.set_environment, bad, "ptr_multi_frame_set_environment", "the map has a non-finite component"),
                                      (frame.set_environment_device, on(bad), "ptr_multi_frame_set_environment_device", "the map has a non-finite component")):
            with pytest.raises(pt.PtrError) as e:
                call(arg)
            assert str(e.value) == name + ": " + text
        assert_unchanged(frame, ids, before, "after the refusals")
        again = new_map(w, h, "noise", 3)
        assert frame.set_environment(again)["envSampling"] == 1
        fresh = pt.DeviceScene(aps.Edited(host.desc, host, env=again).desc, 0, keepalive=host)
        for p in range(len(ids)):
            assert_tables_are_the_hosts(frame.part_scene(p), again)
            assert_same_scene(frame.part_scene(p), fresh, settings, "accepted after the refusals, partition %d" % p, renders=False)
        fresh.close()
    finally:
        frame.close()
        dev.close()


def test_the_mip_chain_is_rebuilt_on_every_partition_that_has_one():
    ids = [0, 0, 0]
    host = pt.HostScene.load(os.path.join(GOLDEN, "env_materials.scene"), ts.SCENES)
    d = host.desc
    w, h = d.envWidth, d.envHeight
    own = np.ctypeslib.as_array(d.envRgba, shape=(h, w, 4)).copy()
    rgba = np.ascontiguousarray(own[::-1, ::-1] * np.float32(0.5) + np.float32(0.01))
    rgba[..., 3] = 1.0
    lod = settings_of(host, aps.METAL | pt.PTR_METAL_ENV_LOD)
    frame = pt.multi_frame(d, lod, device_ids=ids)
    try:
        frame.accumulate(1)   # every partition builds the chain of the old map
        for got in appearance_of(frame, ids, ["scalars"]):
            assert got["scalars"]["envMipLevels"] == 7
        info = frame.set_environment(rgba)
        chain = pt.debug_env_mips(rgba)
        assert info["texelsWritten"] == sum(l.shape[0] * l.shape[1] for l in chain)
        want = np.concatenate([l.reshape(-1, 4) for l in chain[1:]]).view(np.uint32)
        for p in range(3):
            scene = frame.part_scene(p)
            assert_tables_are_the_hosts(scene, rgba)
            assert np.array_equal(scene.appearance_arrays(["envMips"])["envMips"][5:], want), p
        # a frame made afterwards has no chain yet on its partitions, and the call builds none
        late = pt.multi_frame(d, lod, device_ids=[0, 0])
        late.set_environment(rgba)
        for got in appearance_of(late, [0, 0], ["scalars", "envMips"]):
            assert got["scalars"]["envMipLevels"] == 0 and got["envMips"].size == 0
        # both frames render the same image under the new map
        frame.reset()
        frame.accumulate(SPP)
        late.accumulate(SPP)
        same_outputs(outputs(late), outputs(frame), "the chain built before and after the call")
        late.close()
    finally:
        frame.close()


# --------------------------------------------------------------------------------------------------------------------- 5. frames
@pytest.mark.parametrize("metal", [0, aps.METAL], ids=["default", "metal"])
@pytest.mark.parametrize("ids", LISTS, ids=LIST_IDS)
def test_frames_after_a_reset_are_the_single_device_frames(tmp_path, ids, metal):
    host = aps.lights_scene(tmp_path)
    s = settings_of(host, metal)
    mats = {2: aps.material_of(host.desc, 2, emission=(0.5, 0.4, 0.3)), 1: aps.material_of(host.desc, 1, typeEta=(float(METAL_TYPE),))}
    frame, dev = make(host, ids, s=s, primitives=True)
    fresh = upload(aps.Edited(host.desc, host, materials=mats))
    single, other = dev.frame(s), fresh.frame(s)
    try:
        for t in (single, frame):
            t.accumulate(SPP)
        before = outputs(frame)
        dev.set_materials(mats)
        frame.set_materials(mats)
        same_outputs(outputs(frame), before, "an update leaves the sample state alone")
        for t in (single, frame):
            t.reset()
        for t in (single, frame, other):
            t.accumulate(SPP)
        want = outputs(single, dev, s)
        assert (want[2] == SPP).all() and want[0].max() > 0 and not np.array_equal(want[0], before[0])
        same_outputs(outputs(frame), want, "the edited scene on %s" % ids)
        same_outputs(outputs(other, fresh, s), want, "the fresh upload's frame")
        e = single.export_state()["e"]
        params = pt.PtrAdaptiveParams(SPP, 12, 4, float(np.median(e[e > 0])))
        _, want_info = single.refine(params)
        _, got_info = frame.refine(params)
        _, fresh_info = other.refine(params)
        assert 0 < want_info.activeAfter[0] < W * H, "the threshold leaves some pixels active and settles others"
        assert info_of(got_info) == info_of(want_info) == info_of(fresh_info)
        want = outputs(single, dev, s)
        same_outputs(outputs(frame), want, "after the refine on %s" % ids)
        same_outputs(outputs(other, fresh, s), want, "the fresh upload's frame after the refine")
    finally:
        for t in (single, other, frame, dev, fresh):
            t.close()


# --------------------------------------------------------------------------------------------------------------------- 6. with geometry
@pytest.mark.parametrize("ids", LISTS, ids=LIST_IDS)
def test_material_calls_between_geometry_calls(tmp_path, ids):
    host = aps.lights_scene(tmp_path)
    settings = both_semantics(host)
    moved = dsc.rect_of(host, 3)
    moved["corner"] = moved["corner"] + np.array([0.3, -0.2, 0.4], np.float32)
    mats = {3: aps.material_of(host.desc, 3, emission=(0.7, 0.1, 0.1)), 4: aps.material_of(host.desc, 4, emission=(0.5, 0.5, 0.5))}
    changed = dsc.Changed(host, rects={3: pt.rect_update(3, **moved)})
    fresh = upload(aps.Edited(changed.desc, changed, materials=mats))
    want = fresh.arrays()
    made = []
    try:
        for order in ("rectangles first", "materials first"):
            frame, dev = make(host, ids, s=settings[0], primitives=True)
            made += [frame, dev]
            for target in (dev, frame):
                if order == "rectangles first":
                    target.set_rects({3: moved})
                    target.set_materials(mats)
                else:
                    target.set_materials(mats)
                    target.set_rects({3: moved})
            same_on_every_partition(frame, ids, dev, settings, order)
            # the fresh upload of the moved rectangle builds another tree: as test_set_rects_and_set_materials_in_either_order compares it
            for p in range(len(ids)):
                scene = frame.part_scene(p)
                assert_same_scene(scene, fresh, settings, order, arrays=False, renders=False, tree=False)
                got = scene.arrays()
                a, b = by_meta(got), by_meta(want)
                for name in ("tris", "triNormals", "triBounds"):
                    assert np.array_equal(words(got[name][a]), words(want[name][b])), (order, p, name)
                for name in ("rects", "rectLights", "spheres"):
                    assert np.array_equal(words(got[name]), words(want[name])), (order, p, name)
        # a rebuild, then a type change: the rekey runs on the rebuilt tree
        frame, dev = made[-2:]
        rekey = {0: aps.material_of(host.desc, 0, typeEta=(float(METAL_TYPE),)), 3: aps.material_of(host.desc, 3, emission=(0.0, 0.0, 0.0))}
        infos = []
        for target in (dev, frame):
            assert target.rebuild_tree(keep_if_better=False)["installed"] == 1
            infos.append(target.set_materials(rekey))
        assert infos[0]["rowsRekeyed"] == infos[1]["rowsRekeyed"] == 4 and infos[1]["lightsAfter"] == infos[0]["lightsAfter"] == 8
        same_on_every_partition(frame, ids, dev, settings, "a type change on the rebuilt tree")
    finally:
        for t in made:
            t.close()
        fresh.close()


# --------------------------------------------------------------------------------------------------------------------- 7. guards
def test_a_partitions_scene_is_edited_through_the_frame_alone(tmp_path):
    ids = [0, -1]
    quads = aps.Quads(SIZES)
    frame = pt.multi_frame(quads.desc, quads_settings(quads)[1], device_ids=ids)
    host, _ = ls.env_scene(tmp_path, ls.env_map("noise", 16, 8), "menv_guard")
    lit = pt.multi_frame(host.desc, settings_of(host), device_ids=ids)
    try:
        before, env_before = appearance_of(frame, ids), appearance_of(lit, ids)
        pixels = new_textures(quads, 4)
        for call in (lambda: frame.part_scene(1).set_materials({0: aps.material_of(quads.desc, 0, baseColorRoughness=(0.1, 0.2, 0.3))}),
                     lambda: frame.part_scene(1).set_textures({3: pixels[3]}), lambda: frame.part_scene(0).set_textures_device({3: on(pixels[3][0])}),
                     lambda: lit.part_scene(1).set_environment(new_map(16, 8, "noise", 5)), lambda: lit.part_scene(0).set_environment_device(on(new_map(16, 8, "noise", 5)))):
            with pytest.raises(pt.PtrError, match="through its MultiFrame"):
                call()
        assert_unchanged(frame, ids, before, "after the borrowed scene's refusals")
        assert_unchanged(lit, ids, env_before, "after the borrowed scene's refusals")
        # src_device at the device count: through the C interface
        lib, err = pt.load_library(), C.create_string_buffer(256)
        items, keep = pt.DeviceScene._texture_items("set_textures_device", {3: on(pixels[3][0])}, lambda *a: pt.DeviceScene._device_pixels(frame, *a))
        assert lib.ptr_multi_frame_set_textures_device(frame._h, items, 1, pt.device_count(), None, None, err, len(err)) == 1
        assert err.value == b"ptr_multi_frame_set_textures_device: no such HIP device"
        t = on(new_map(16, 8, "noise", 6))
        assert lib.ptr_multi_frame_set_environment_device(lit._h, C.c_void_p(t.data_ptr()), 16, 8, pt.device_count(), None, None, err, len(err)) == 1
        assert err.value == b"ptr_multi_frame_set_environment_device: no such HIP device"
        assert_unchanged(frame, ids, before, "after the refused source device")
        assert_unchanged(lit, ids, env_before, "after the refused source device")
        # tensors that are not on one device, or on none
        with pytest.raises(pt.PtrError, match="not on a HIP device"):
            frame.set_textures_device({3: torch.from_numpy(pixels[3][0])})
    finally:
        frame.close()
        lit.close()


def test_a_temporal_sequence_through_the_frame_across_a_dimmed_light(tmp_path):
    """test_gpu_appearance.py's sequence - six frames of 4 spp with covariance at a fixed camera, the light's emission dropping before
    frame 3 - with the frames accumulated by a MultiFrame and filtered by part_scene(0).temporal, against a single-device scene, Frame and
    Temporal given the same calls."""
    host = aps.lights_scene(tmp_path)
    settings = settings_of(host)
    frame, dev = make(host, [0, 0, 0], s=settings, primitives=True)
    single = dev.frame(settings)
    handles = [frame.part_scene(0).temporal(W, H, cov=True), dev.temporal(W, H, cov=True)]
    dim = {2: aps.material_of(host.desc, 2, emission=(0.45, 0.4, 0.35)), 3: aps.material_of(host.desc, 3, emission=(0.1, 0.3, 0.15))}
    try:
        for k in range(6):
            s = settings.copy()
            s.seed = 100 + k
            outs = []
            for target, accumulator, temporal in ((frame, frame, handles[0]), (dev, single, handles[1])):
                if k == 3:
                    target.set_materials(dim)
                accumulator.reset(s)
                accumulator.accumulate(SPP)
                rgb, cov, _ = accumulator.resolve()[:3]
                outs.append(temporal.step(s, rgb, cov))
            got, want = outs
            assert want["info"]["frameIndex"] == got["info"]["frameIndex"] == k and np.isfinite(want["rgb"]).all()
            for name in ("rgb", "cov", "length"):
                assert np.array_equal(words(got[name]), words(want[name])), (k, name)
    finally:
        for t in handles + [single, frame, dev]:
            t.close()
