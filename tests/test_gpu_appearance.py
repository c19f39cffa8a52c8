"""include/ptr_appearance.h on the device: ptr_scene_set_materials, ptr_scene_set_textures and ptr_scene_set_environment (with their
device-pointer forms) against what a fresh upload of the edited description produces.  The reference is always that fresh upload, and for
the environment the host probes debug_env_distribution / debug_env_mips as well; every comparison is exact (raw words)."""
import os

import numpy as np
import pytest

import appearance_scenes as aps
import deform_scenes as dsc
import light_scenes as ls
import traversal_scenes as ts

pt = ts.pt
pytestmark = pytest.mark.gpu
GOLDEN = ts.GOLDEN
LAMBERT, METAL_TYPE, LIGHT_TYPE, SSS_TYPE = 0, 1, 3, 5


def upload(holder, dynamic=True):
    return pt.DeviceScene(holder.desc, 0, keepalive=holder, dynamic=dynamic, primitives=dynamic)


def views(host):
    """32 x 24 settings of the scene under the default and under the Metal semantics."""
    out = []
    for metal in (0, aps.METAL):
        s = host.settings_for(width=32, height=24)
        s.metalSemantics = metal
        out.append(s)
    return out


def words(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def assert_same_scene(got, want, settings, what, arrays=True, renders=True, tree=True):
    a, b = got.appearance_arrays(), want.appearance_arrays()
    assert a["scalars"] == b["scalars"], what
    for name in a:
        if name != "scalars":
            assert a[name].shape == b[name].shape and np.array_equal(a[name], b[name]), (what, name)
    if arrays:
        x, y = got.arrays(), want.arrays()
        for name in x:
            assert x[name].shape == y[name].shape and np.array_equal(words(x[name]), words(y[name])), (what, name)
    drop = () if tree else ("nodes", "leaves", "max_depth", "max_leaf", "sah_cost_x1000")   # (what another tree changes)
    assert {k: v for k, v in got.info().items() if k not in drop} == {k: v for k, v in want.info().items() if k not in drop}, what
    for s in settings:
        assert got.shade_kernel_set(s) == want.shade_kernel_set(s), what
        if renders:
            assert np.array_equal(words(got.render_image(s, 4)[0]), words(want.render_image(s, 4)[0])), (what, s.metalSemantics)


class Session:
    """A device scene that is edited call by call beside the description a fresh upload is given."""

    def __init__(self, host, dynamic=True):
        self.host, self.dynamic = host, dynamic
        self.materials = {}
        self.dev = upload(host, dynamic)
        self.settings = views(host)

    def edit(self, what, twice=False, **members_by_index):
        """edit("...", m3=dict(emission=(0, 0, 0))): one call that names every given material, on top of the edits so far."""
        current = aps.Edited(self.host.desc, self.host, materials=self.materials)
        call = {int(k[1:]): aps.material_of(current.desc, int(k[1:]), **v) for k, v in members_by_index.items()}
        info = self.dev.set_materials(call)
        if twice:
            again = self.dev.set_materials(call)
            assert again["rowsRekeyed"] == 0 and again["lightsBefore"] == again["lightsAfter"] == info["lightsAfter"], what
        self.materials.update(call)
        edited = aps.Edited(self.host.desc, self.host, materials=self.materials)
        fresh = upload(edited, self.dynamic)
        assert_same_scene(self.dev, fresh, self.settings, what)
        assert info["lightsAfter"] == fresh.info()["rect_lights"], what
        fresh.close()
        return info


# --------------------------------------------------------------------------- materials
def test_every_kind_of_material_edit_equals_a_fresh_upload(tmp_path):
    host = aps.lights_scene(tmp_path)
    s = Session(host)
    tris = s.dev.info()["triangles"]
    assert tris == 23 and s.dev.info()["rect_lights"] == 2
    info = s.edit("colour only", m1=dict(baseColorRoughness=(0.9, 0.1, 0.2)))
    assert info["rowsRekeyed"] == 0 and (info["lightsBefore"], info["lightsAfter"]) == (2, 2)
    info = s.edit("Lambert to metal on a sphere and a mesh", m1=dict(typeEta=(float(METAL_TYPE),), baseColorRoughness=(0.9, 0.8, 0.5, 0.2)))
    assert info["rowsRekeyed"] == 1, "the mesh's one triangle"
    info = s.edit("Lambert to metal on two rectangles", m0=dict(typeEta=(float(METAL_TYPE),), baseColorRoughness=(0.8, 0.8, 0.8, 0.4)))
    assert info["rowsRekeyed"] == 4
    info = s.edit("a light's emission changes", m2=dict(emission=(1.0, 2.0, 3.0)))
    assert info["rowsRekeyed"] == 0 and (info["lightsBefore"], info["lightsAfter"]) == (2, 2)
    info = s.edit("a light goes out by emission 0", m3=dict(emission=(0.0, 0.0, 0.0)))
    assert (info["lightsBefore"], info["lightsAfter"]) == (2, 1)
    info = s.edit("the last light goes out by type", m2=dict(typeEta=(float(LAMBERT),)))
    assert (info["lightsBefore"], info["lightsAfter"]) == (1, 0) and info["rowsRekeyed"] == 2
    info = s.edit("two materials in one call: two rectangles become lights", m2=dict(typeEta=(float(LIGHT_TYPE),)), m3=dict(emission=(2.0, 6.0, 3.0)))
    assert (info["lightsBefore"], info["lightsAfter"]) == (0, 2) and info["rowsRekeyed"] == 2
    assert s.dev.appearance_arrays(["scalars"])["scalars"]["settleRectLights"] == 1
    info = s.edit("nine lights: past the most a scene settles connections for", m4=dict(emission=(4.0, 4.0, 4.0)))
    assert (info["lightsBefore"], info["lightsAfter"]) == (2, 9)
    assert s.dev.appearance_arrays(["scalars"])["scalars"]["settleRectLights"] == 0
    info = s.edit("back to two, and the same call twice", twice=True, m4=dict(emission=(0.0, 0.0, 0.0)))
    assert (info["lightsBefore"], info["lightsAfter"]) == (9, 2)
    s.edit("the random-walk flag on", m1=dict(typeEta=(float(SSS_TYPE),), sssParams=(0.1, 1.0, 0.0, 0.0)))
    assert s.dev.appearance_arrays(["scalars"])["scalars"]["hasRandomWalkMaterial"] == 1
    s.edit("the random-walk flag off", m1=dict(sssParams=(0.1, 0.0, 0.0, 0.0)))
    assert s.dev.appearance_arrays(["scalars"])["scalars"]["hasRandomWalkMaterial"] == 0


def stock_scenes(tmp):
    yield "materials", pt.HostScene.load(os.path.join(GOLDEN, "materials.scene"), ts.SCENES)
    yield "cornell_small_mesh", ts.scene_a()
    for n in (1, 2, 8, 9):
        yield "lights_%d" % n, ls.light_scene(tmp, n)


def test_edits_of_the_stock_scenes_equal_a_fresh_upload(tmp_path):
    for key, host in stock_scenes(tmp_path):
        d = host.desc
        types = [int(d.materials[i].typeEta[0]) for i in range(d.materialCount)]
        lights = [i for i, t in enumerate(types) if t == LIGHT_TYPE]
        lambert = types.index(LAMBERT)
        s = Session(host)
        before = s.dev.info()["rect_lights"]
        s.edit(key + ": colour only", **{"m%d" % lambert: dict(baseColorRoughness=(0.1, 0.7, 0.3))})
        info = s.edit(key + ": Lambert to metal", **{"m%d" % lambert: dict(typeEta=(float(METAL_TYPE),), baseColorRoughness=(0.9, 0.9, 0.9, 0.1))})
        if lights:
            info = s.edit(key + ": a light goes out", **{"m%d" % lights[0]: dict(emission=(0.0, 0.0, 0.0))})
            assert info["lightsBefore"] == before and info["lightsAfter"] <= before
            info = s.edit(key + ": and comes back dimmer", **{"m%d" % lights[0]: dict(emission=(0.5, 0.25, 2.0))})
            assert info["lightsAfter"] == before


def test_a_static_scene_without_rectangles_accepts_the_call(tmp_path):
    host = aps.static_scene(tmp_path)
    s = Session(host, dynamic=False)
    assert not s.dev.is_dynamic
    info = s.edit("static: the mesh turns to metal, the sphere's light changes colour", m0=dict(typeEta=(float(METAL_TYPE),)), m1=dict(emission=(1.0, 5.0, 2.0)))
    assert info["rowsRekeyed"] == 1
    s.edit("static: and back", twice=True, m0=dict(typeEta=(float(LAMBERT),)))


def test_rectangles_without_their_records_refuse_and_leave_the_scene_unchanged():
    host = ts.scene_a()
    d = host.desc
    used = {min(d.rects[i].materialTwoSided[0], d.materialCount - 1) for i in range(d.rectCount)}
    free = [i for i in range(d.materialCount) if i not in used]
    for dynamic, primitives in ((False, False), (True, False)):
        dev = pt.DeviceScene(d, 0, keepalive=host, dynamic=dynamic, primitives=primitives)
        before, tris = dev.appearance_arrays(), dev.arrays(["tris"])["tris"].copy()
        with pytest.raises(pt.PtrError) as e:
            dev.set_materials({min(used): aps.material_of(d, min(used), typeEta=(float(METAL_TYPE),))})
        assert str(e.value).startswith("ptr_scene_set_materials: a rectangle uses a named material") and "PTR_DYNAMIC_PRIMITIVES" in str(e.value)
        after = dev.appearance_arrays()
        assert before["scalars"] == after["scalars"] and all(np.array_equal(before[k], after[k]) for k in before if k != "scalars")
        assert np.array_equal(words(tris), words(dev.arrays(["tris"])["tris"]))
        # what the list itself says wrong is refused by name as well, and a material no rectangle uses is accepted
        for call, text in (({d.materialCount: aps.material_of(d, 0)}, "out of range"),
                           ({0: aps.material_of(d, 0, emission=(float("nan"),))}, "non-finite"),
                           ({0: aps.material_of(d, 0, textureIndices0=(0,))}, "uploaded without textures")):
            with pytest.raises(pt.PtrError) as e:
                dev.set_materials(call)
            assert str(e.value).startswith("ptr_scene_set_materials: ") and text in str(e.value)
        if free:
            dev.set_materials({free[0]: aps.material_of(d, free[0], baseColorRoughness=(0.3, 0.3, 0.9))})
            fresh = pt.DeviceScene(aps.Edited(d, host, materials={free[0]: aps.material_of(d, free[0], baseColorRoughness=(0.3, 0.3, 0.9))}).desc, 0, keepalive=host,
                                   dynamic=dynamic, primitives=primitives)
            assert_same_scene(dev, fresh, views(host), "a material no rectangle uses")
    assert free, "scene A's mesh has a material of its own"


def test_set_rects_and_set_materials_in_either_order(tmp_path):
    host = aps.lights_scene(tmp_path)
    moved = dsc.rect_of(host, 3)
    moved["corner"] = moved["corner"] + np.array([0.3, -0.2, 0.4], np.float32)
    update = pt.rect_update(3, **moved)
    mats = {3: aps.material_of(host.desc, 3, emission=(7.0, 1.0, 1.0)), 4: aps.material_of(host.desc, 4, emission=(0.5, 0.5, 0.5))}
    changed = dsc.Changed(host, rects={3: update})
    fresh = upload(aps.Edited(changed.desc, changed, materials=mats))
    want = fresh.arrays()
    devs = []
    for order in ("materials first", "rectangles first"):
        dev = upload(host)
        if order == "materials first":
            dev.set_materials(mats)
            dev.set_rects({3: moved})
        else:
            dev.set_rects({3: moved})
            dev.set_materials(mats)
        # the fresh upload of a moved rectangle builds another tree, so its triangles are in another leaf order: they are compared in the
        # order of their meta words, as tests/test_gpu_dynamic_deform.py compares them; what does not depend on the tree is compared as it is
        assert_same_scene(dev, fresh, views(host), order, arrays=False, renders=False, tree=False)
        got = dev.arrays()
        a, b = by_meta(got), by_meta(want)
        for name in ("tris", "triNormals", "triBounds"):
            assert np.array_equal(words(got[name][a]), words(want[name][b])), (order, name)
        for name in ("rects", "rectLights", "spheres"):
            assert np.array_equal(words(got[name]), words(want[name])), (order, name)
        devs.append(dev)
    # and the two orders leave one and the same scene, tree included
    assert_same_scene(devs[0], devs[1], views(host), "either order")


def by_meta(a):
    """Order of the triangles by their meta words without the shade key (kind | geometry, primitive index)."""
    w = a["tris"].view(np.uint32)
    key = ((w[:, 1, 3] & np.uint32(0xC3FFFFFF)).astype(np.uint64) << np.uint64(32)) | w[:, 2, 3].astype(np.uint64)
    assert len(np.unique(key)) == len(key)
    return np.argsort(key)


def test_a_rebuilt_tree_stays_rebuilt(tmp_path):
    host = aps.lights_scene(tmp_path)
    dev = upload(host)
    dev.rebuild_tree(keep_if_better=False)
    tree = dev.rebuild_arrays()
    nodes = {k: v.copy() for k, v in dev.arrays(["boxes", "qnodes", "wnodes"]).items()}
    mats = {0: aps.material_of(host.desc, 0, typeEta=(float(METAL_TYPE),)), 3: aps.material_of(host.desc, 3, emission=(0.0, 0.0, 0.0))}
    dev.set_materials(mats)
    after = dev.rebuild_arrays()
    assert tree["info"] == after["info"] and all(np.array_equal(tree[k], after[k]) for k in tree if k != "info")
    assert all(np.array_equal(v, dev.arrays([k])[k]) for k, v in nodes.items())
    fresh = upload(aps.Edited(host.desc, host, materials=mats))
    a, b = dev.appearance_arrays(), fresh.appearance_arrays()
    assert a["scalars"] == b["scalars"] and all(np.array_equal(a[k], b[k]) for k in a if k != "scalars")
    for name in ("tris", "triNormals", "rects", "rectLights"):
        assert np.array_equal(words(dev.arrays([name])[name]), words(fresh.arrays([name])[name])), name


# --------------------------------------------------------------------------- textures
def sample_points(n, seed):
    rng = np.random.default_rng(seed)
    uv = rng.uniform(-1.5, 2.5, (n, 2))
    return np.concatenate([uv, rng.uniform(-1.0, 17.0, (n, 1))], axis=1).astype(np.float32)


def test_texture_updates_equal_a_fresh_upload():
    import torch

    quads = aps.Quads()
    base = pt.HostScene.load(os.path.join(GOLDEN, "textured.scene"), GOLDEN)
    settings = [quads.settings(base.settings_for(), metal) for metal in (False, True)]
    rng = np.random.default_rng(9)
    new = {}
    for i, (w, h) in enumerate(aps.TEXTURE_SIZES):
        old = quads.desc.textures[i]
        new[i] = (np.exp(rng.uniform(-4.0, 2.0, (h, w, 4))).astype(np.float32), (old.wrapS + 1) % 3, old.wrapT, 1 - old.filter)
    fresh = pt.DeviceScene(aps.Edited(quads.desc, quads, textures=new).desc, 0, keepalive=quads)
    levels = [int(r[2]) for r in fresh.appearance_arrays(["texInfo"])["texInfo"]]
    assert levels == [1, 3, 3, 4, 5, 5, 16]
    uv = sample_points(257, 1)
    for path in ("host", "device"):
        dev = pt.DeviceScene(quads.desc, 0, keepalive=quads)
        before = dev.appearance_arrays(["texInfo"])["texInfo"]
        if path == "host":
            info = dev.set_textures(new)
        else:
            tensors = {i: (torch.from_numpy(v[0]).cuda(), v[1], v[2], v[3]) for i, v in new.items()}
            info = dev.set_textures_device(tensors)
        after = dev.appearance_arrays(["texInfo"])["texInfo"]
        assert (before[:, 3] != after[:, 3]).all() and np.array_equal(np.delete(before, 3, axis=1), np.delete(after, 3, axis=1)), "only wrap / filter change"
        assert info["texelsWritten"] == len(fresh.appearance_arrays(["texels"])["texels"])
        assert_same_scene(dev, fresh, settings, "quads from " + path)
        for t in range(len(aps.TEXTURE_SIZES)):
            assert np.array_equal(words(dev.texture_sample(t, uv)), words(fresh.texture_sample(t, uv))), (path, t)
    # one texture of several: the others keep their texels; and what the call refuses
    dev = pt.DeviceScene(quads.desc, 0, keepalive=quads)
    dev.set_textures({2: new[2]})
    assert_same_scene(dev, pt.DeviceScene(aps.Edited(quads.desc, quads, textures={2: new[2]}).desc, 0, keepalive=quads), settings, "one texture of seven")
    kept = dev.appearance_arrays(["texels", "texInfo"])
    bad = new[3][0].copy()
    bad[5, 5, 2] = np.inf
    for name, call, arg, text in (("ptr_scene_set_textures", dev.set_textures, {3: bad}, "non-finite"),
                                  ("ptr_scene_set_textures_device", dev.set_textures_device, {3: torch.from_numpy(bad).cuda()}, "non-finite"),
                                  ("ptr_scene_set_textures", dev.set_textures, {3: new[4][0]}, "was uploaded at 8 x 8"),
                                  ("ptr_scene_set_textures", dev.set_textures, {7: new[3][0]}, "out of range")):
        with pytest.raises(pt.PtrError) as e:
            call(arg)
        assert str(e.value).startswith(name + ": ") and text in str(e.value)
        now = dev.appearance_arrays(["texels", "texInfo"])
        assert all(np.array_equal(kept[k], now[k]) for k in kept), text
    # a check that refused left nothing behind: an accepted call with the pixels texture 3 has, another wrap and filter, is a fresh upload's
    old = quads.desc.textures[3]
    rewrapped = (quads.pixels[3], (old.wrapS + 1) % 3, (old.wrapT + 2) % 3, 1 - old.filter)
    dev.set_textures({3: rewrapped})
    now = dev.appearance_arrays(["texels", "texInfo"])
    assert np.array_equal(kept["texels"], now["texels"]) and (kept["texInfo"] != now["texInfo"]).sum() == 1, "only the wrap / filter word of texture 3"
    fresh = pt.DeviceScene(aps.Edited(quads.desc, quads, textures={2: new[2], 3: rewrapped}).desc, 0, keepalive=quads)
    assert_same_scene(dev, fresh, settings, "wrap and filter of one texture after the refusals")
    plain = ts.scene_a()   # (held: the device scene reads the description while it uploads)
    with pytest.raises(pt.PtrError) as e:
        pt.DeviceScene(plain.desc, 0, keepalive=plain).set_textures({0: new[3][0]})
    assert str(e.value) == "ptr_scene_set_textures: the scene has no textures"


def test_textures_of_the_gltf_scene():
    import torch

    host = pt.HostScene.load(os.path.join(GOLDEN, "textured.scene"), GOLDEN)
    d = host.desc
    rng = np.random.default_rng(12)
    new = {i: (rng.random((d.textures[i].height, d.textures[i].width, 4), dtype=np.float32), d.textures[i].wrapS, d.textures[i].wrapT, d.textures[i].filter)
           for i in (0, 4)}
    settings = views(host)
    fresh = pt.DeviceScene(aps.Edited(d, host, textures=new).desc, 0, keepalive=host)
    a = pt.DeviceScene(d, 0, keepalive=host)
    a.set_textures(new)
    b = pt.DeviceScene(d, 0, keepalive=host)
    b.set_textures_device({i: (torch.from_numpy(v[0]).cuda(),) + v[1:] for i, v in new.items()})
    assert_same_scene(a, fresh, settings, "textured.scene from host pixels")
    assert_same_scene(b, fresh, settings, "textured.scene from device pixels")


# --------------------------------------------------------------------------- environment
def new_map(w, h, kind, seed):
    rng = np.random.default_rng(seed)
    rgba = np.ones((h, w, 4), np.float32)
    rgba[..., :3] = np.exp(rng.uniform(np.log(0.02), np.log(8.0), (h, w, 3))).astype(np.float32)
    if kind == "black_row":
        rgba[h // 3, :, :3] = 0.0
    elif kind == "spot":
        rgba[h // 2, w // 3, :3] = 1e5
    elif kind == "black":
        rgba[..., :3] = 0.0
    return rgba


def assert_tables_are_the_hosts(dev, rgba):
    got = dev.appearance_arrays(["envRgba", "envCond", "envMarg", "envPdf", "scalars"])
    want = pt.debug_env_distribution(rgba)
    h, w = rgba.shape[:2]
    assert got["scalars"]["envSampling"] == 1
    assert np.array_equal(got["envRgba"].reshape(h, w, 4), rgba.view(np.uint32))
    cond = got["envCond"].reshape(h, w, 2)
    assert np.array_equal(cond[..., 0], want["cond_threshold"].view(np.uint32)) and np.array_equal(cond[..., 1], want["cond_alias"])
    assert np.array_equal(got["envMarg"][:, 0], want["marg_threshold"].view(np.uint32)) and np.array_equal(got["envMarg"][:, 1], want["marg_alias"])
    assert np.array_equal(got["envPdf"].reshape(h, w), want["pdf"].view(np.uint32))


ENV_CASES = [(1, 1, "noise"), (2, 1, "noise"), (3, 5, "noise"), (16, 8, "noise"), (64, 32, "black_row"), (512, 256, "spot")]


@pytest.mark.parametrize("w,h,kind", ENV_CASES, ids=["%dx%d" % c[:2] for c in ENV_CASES])
def test_environment_updates_equal_a_fresh_upload(tmp_path, w, h, kind):
    import torch

    host, old = ls.env_scene(tmp_path, ls.env_map("noise", w, h), "env_%d_%d" % (w, h))
    assert old.shape == (h, w, 4)
    rgba = new_map(w, h, kind, 21)
    settings = views(host)
    fresh = pt.DeviceScene(aps.Edited(host.desc, host, env=rgba).desc, 0, keepalive=host)
    u = ls.env_u(pt.debug_env_distribution(rgba), 200, 5)
    dirs = ls.env_directions(w, h, settings[0].environmentRotation, 200, 6)
    for path in ("host", "device"):
        dev = pt.DeviceScene(host.desc, 0, keepalive=host)
        info = dev.set_environment(rgba) if path == "host" else dev.set_environment_device(torch.from_numpy(rgba).cuda())
        assert info["envSampling"] == 1 and info["texelsWritten"] == w * h
        assert_tables_are_the_hosts(dev, rgba)
        assert_same_scene(dev, fresh, settings, "%s path" % path)
        for s in settings:
            assert np.array_equal(words(dev.env_sample(s, u)), words(fresh.env_sample(s, u))), path
            assert np.array_equal(words(dev.env_eval(s, dirs)), words(fresh.env_eval(s, dirs))), path


def test_a_black_map_turns_sampling_off_and_a_lit_one_turns_it_on_again(tmp_path):
    w, h = 16, 8
    host, _ = ls.env_scene(tmp_path, ls.env_map("noise", w, h), "env_black")
    settings = views(host)
    black, lit = new_map(w, h, "black", 1), new_map(w, h, "noise", 2)
    dev = pt.DeviceScene(host.desc, 0, keepalive=host)
    info = dev.set_environment(black)
    assert info["envSampling"] == 0
    assert_same_scene(dev, pt.DeviceScene(aps.Edited(host.desc, host, env=black).desc, 0, keepalive=host), settings, "black")
    assert dev.appearance_arrays(["envCond"])["envCond"].size == 0
    info = dev.set_environment(lit)
    assert info["envSampling"] == 1
    assert_tables_are_the_hosts(dev, lit)
    assert_same_scene(dev, pt.DeviceScene(aps.Edited(host.desc, host, env=lit).desc, 0, keepalive=host), settings, "lit again")
    # a scene that was uploaded black has no tables yet: the call makes them
    dark = pt.DeviceScene(aps.Edited(host.desc, host, env=black).desc, 0, keepalive=host)
    assert dark.appearance_arrays(["scalars"])["scalars"]["envSampling"] == 0
    dark.set_environment(lit)
    assert_same_scene(dark, dev, settings, "lit after a black upload")
    # refusals: another size, a non-finite component, a scene without a map
    before = dev.appearance_arrays()
    bad = lit.copy()
    bad[3, 4, 1] = np.nan
    for arg, text in ((lit[:, :8], "was uploaded at 16 x 8, not 8 x 8"), (bad, "non-finite")):
        with pytest.raises(pt.PtrError) as e:
            dev.set_environment(np.ascontiguousarray(arg))
        assert str(e.value).startswith("ptr_scene_set_environment: ") and text in str(e.value)
    after = dev.appearance_arrays()
    assert all(np.array_equal(before[k], after[k]) for k in before if k != "scalars") and before["scalars"] == after["scalars"]
    # a check that refused left nothing behind: an accepted call after the refusals is a fresh upload of its map
    again = new_map(w, h, "noise", 3)
    assert dev.set_environment(again)["envSampling"] == 1
    assert_tables_are_the_hosts(dev, again)
    assert_same_scene(dev, pt.DeviceScene(aps.Edited(host.desc, host, env=again).desc, 0, keepalive=host), settings, "accepted after the refusals")
    plain = ts.scene_a()   # (held: the device scene reads the description while it uploads)
    with pytest.raises(pt.PtrError) as e:
        pt.DeviceScene(plain.desc, 0, keepalive=plain).set_environment(lit)
    assert str(e.value) == "ptr_scene_set_environment: the scene was uploaded without an environment map"


def test_the_environment_of_the_material_scene_and_its_mip_chain():
    host = pt.HostScene.load(os.path.join(GOLDEN, "env_materials.scene"), ts.SCENES)
    d = host.desc
    w, h = d.envWidth, d.envHeight
    own = np.ctypeslib.as_array(d.envRgba, shape=(h, w, 4)).copy()
    rgba = np.ascontiguousarray(own[::-1, ::-1] * np.float32(0.5) + np.float32(0.01))
    rgba[..., 3] = 1.0
    lod = host.settings_for(width=32, height=24)
    lod.metalSemantics = aps.METAL | pt.PTR_METAL_ENV_LOD
    settings = views(host) + [lod]
    # (the scene has two rectangles; the environment calls need nothing of them, so a static upload does)
    dev = pt.DeviceScene(d, 0, keepalive=host)
    dev.render_image(lod, 1)   # builds the chain of the old map
    assert dev.appearance_arrays(["scalars"])["scalars"]["envMipLevels"] == 7
    info = dev.set_environment(rgba)
    assert_tables_are_the_hosts(dev, rgba)
    chain = pt.debug_env_mips(rgba)
    assert info["texelsWritten"] == sum(l.shape[0] * l.shape[1] for l in chain)
    mips = dev.appearance_arrays(["envMips"])["envMips"]
    assert np.array_equal(mips[5:], np.concatenate([l.reshape(-1, 4) for l in chain[1:]]).view(np.uint32))
    fresh = pt.DeviceScene(aps.Edited(d, host, env=rgba).desc, 0, keepalive=host)
    fresh.render_image(lod, 1)
    assert_same_scene(dev, fresh, settings, "env_materials.scene")
    # its own map again, from the other entry point
    import torch

    dev.set_environment_device(torch.from_numpy(own).cuda())
    again = pt.DeviceScene(d, 0, keepalive=host)
    again.render_image(lod, 1)
    assert_same_scene(dev, again, settings, "its own map again")


# --------------------------------------------------------------------------- handles
def test_a_frame_that_is_reset_after_an_update_equals_the_fresh_scenes_frame(tmp_path):
    host = aps.lights_scene(tmp_path)
    settings = views(host)[0]
    mats = {2: aps.material_of(host.desc, 2, emission=(0.5, 0.4, 0.3)), 1: aps.material_of(host.desc, 1, typeEta=(float(METAL_TYPE),))}
    dev = upload(host)
    frame = dev.frame(settings)
    frame.accumulate(4)
    dev.set_materials(mats)
    frame.reset()
    frame.accumulate(4)
    fresh = upload(aps.Edited(host.desc, host, materials=mats))
    other = fresh.frame(settings)
    other.accumulate(4)
    for a, b in zip(frame.resolve(), other.resolve()):
        assert np.array_equal(words(a), words(b))


def test_a_temporal_sequence_runs_across_a_dimmed_light(tmp_path):
    """Six frames of 4 spp with covariance at a fixed camera; the light's emission drops to a twentieth before frame 4.  The history length
    the filter reports says where it started over: the count of pixels whose length is 1 after frame 4 is printed beside the count after
    frame 3, the last frame before the change.  Neither is held to a threshold."""
    host = aps.lights_scene(tmp_path)
    settings = views(host)[0]
    dev = upload(host)
    temporal = dev.temporal(settings.width, settings.height, cov=True)
    restarted = []
    for k in range(6):
        if k == 3:
            dev.set_materials({2: aps.material_of(host.desc, 2, emission=(0.45, 0.4, 0.35)), 3: aps.material_of(host.desc, 3, emission=(0.1, 0.3, 0.15))})
        s = settings.copy()
        s.seed = 100 + k
        rgb, cov, _ = dev.render_image_cov(s, 4)
        out = temporal.step(s, rgb, cov)
        assert out["info"]["frameIndex"] == k and np.isfinite(out["rgb"]).all() and np.isfinite(out["cov"]).all()
        restarted.append(int((out["length"] == 1.0).sum()))   # (0: the pixel misses the scene)
    print("pixels whose history restarted, per frame: %s (the light dims before frame 3; %d pixels)" % (restarted, settings.width * settings.height))
    assert restarted[0] > 0, "the first step starts every pixel that sees the scene"
