"""Descriptions of the appearance tests (test_appearance_host.py on the CPU, test_gpu_appearance.py on the device): a copy of a
description with other materials, texture pixels and environment pixels - what a fresh upload is given where the device scene was
updated - material edits, and the small scenes those tests build."""
import ctypes as C

import numpy as np

import traversal_scenes as ts

pt = ts.pt
NONE = 0xFFFFFFFF
METAL = pt.PTR_METAL_MEDIA | pt.PTR_METAL_THIN | pt.PTR_METAL_FACE_NORMAL | pt.PTR_METAL_SPECULAR | pt.PTR_METAL_SSS | pt.PTR_METAL_PBR | pt.PTR_METAL_CLAMPS


def material_of(desc, index, **changes):
    """A copy of material `index` of the description with the named members replaced (a sequence fills the member's first entries)."""
    m = pt.PtrMaterial()
    C.memmove(C.byref(m), C.byref(desc.materials[index]), C.sizeof(pt.PtrMaterial))
    for name, value in changes.items():
        member = getattr(m, name)
        if hasattr(member, "__len__"):
            for k, v in enumerate(value):
                member[k] = v
        else:
            setattr(m, name, value)
    return m


class Edited:
    """A copy of a description with other materials ({index: PtrMaterial}), texture pixels ({index: pixels [h, w, 4] or (pixels, wrapS,
    wrapT, filter)}) and environment pixels ([h, w, 4]); everything else is the original's, which `keep` keeps alive."""

    def __init__(self, desc, keep=None, materials=None, textures=None, env=None):
        self._keep = [keep]
        self.desc = pt.PtrSceneDesc()
        C.memmove(C.byref(self.desc), C.byref(desc), C.sizeof(pt.PtrSceneDesc))
        self._materials = (pt.PtrMaterial * max(desc.materialCount, 1))()
        for i in range(desc.materialCount):
            C.memmove(C.byref(self._materials[i]), C.byref(desc.materials[i]), C.sizeof(pt.PtrMaterial))
        for i, m in (materials or {}).items():
            C.memmove(C.byref(self._materials[i]), C.byref(m), C.sizeof(pt.PtrMaterial))
        self.desc.materials = C.cast(self._materials, C.POINTER(pt.PtrMaterial))
        fp = C.POINTER(C.c_float)
        if textures:
            self._textures = (pt.PtrTexture * desc.textureCount)()
            for i in range(desc.textureCount):
                C.memmove(C.byref(self._textures[i]), C.byref(desc.textures[i]), C.sizeof(pt.PtrTexture))
            for i, value in textures.items():
                pixels, wrap_s, wrap_t, filt = value if isinstance(value, tuple) else (value, 0, 0, 1)
                a = np.ascontiguousarray(pixels, np.float32)
                assert a.shape == (desc.textures[i].height, desc.textures[i].width, 4)
                self._keep.append(a)
                self._textures[i].rgba = a.ctypes.data_as(fp)
                self._textures[i].wrapS, self._textures[i].wrapT, self._textures[i].filter = wrap_s, wrap_t, filt
            self.desc.textures = C.cast(self._textures, C.POINTER(pt.PtrTexture))
        if env is not None:
            a = np.ascontiguousarray(env, np.float32)
            assert a.shape == (desc.envHeight, desc.envWidth, 4)
            self._keep.append(a)
            self.desc.envRgba = a.ctypes.data_as(fp)


def lights_scene(tmp):
    """Nine small rectangles under a ceiling, over a floor, a sphere and a one-triangle mesh: rectangle 2 uses material 2, rectangle 3
    material 3, rectangles 4..10 material 4; materials 2 and 3 are emitters and material 4 is a light of emission 0, so the scene starts
    with two lights and the three materials switch 1, 1 and 7 of them.  Rectangles 0 and 1 (floor and ceiling) share material 0."""
    ts._write_obj(tmp / "tri.obj", [(-0.5, 0.2, 0.3), (0.6, 0.2, 0.2), (0.0, 1.0, 0.4)], [(0, 1, 2)])
    text = ("camera target=0,1,0 distance=7 yaw=0.5 pitch=0.25 vfov=40\nrenderer maxDepth=4 seed=11\nbackground solid=0.02,0.02,0.03\n"
            "material type=lambert albedo=0.7,0.7,0.6\nmaterial type=lambert albedo=0.2,0.5,0.8\n"
            "material type=diffuse_light emit=9,8,7\nmaterial type=diffuse_light emit=2,6,3\nmaterial type=diffuse_light emit=0,0,0\n"
            "rectangle x=-4,4 y=0 z=-4,4 normal=1 material=0\nrectangle x=-4,4 y=3 z=-4,4 normal=-1 material=0\n"
            "rectangle x=-0.5,0.5 y=2.9 z=-0.5,0.5 normal=-1 material=2\nrectangle x=1.5,2.2 y=2.9 z=-0.5,0.5 normal=-1 material=3\n")
    for k in range(7):
        text += "rectangle x=%g,%g y=2.8 z=%g,%g normal=-1 material=4\n" % (-3.5 + k, -3.0 + k, 1.5, 2.0)
    text += "sphere center=-1.2,0.5,0 radius=0.5 material=1\nmesh path=tri.obj material=1\n"
    p = tmp / "appearance_lights.scene"
    p.write_text(text)
    host = ts.load(p, str(tmp))
    assert host.desc.rectCount == 11 and host.desc.materialCount == 5
    return host


def static_scene(tmp):
    """A sphere and a one-triangle mesh, no rectangle: a static upload accepts every material of it."""
    ts._write_obj(tmp / "tri2.obj", [(-0.5, -0.4, 0.3), (0.6, -0.3, 0.2), (0.0, 0.7, 0.4)], [(0, 1, 2)])
    p = tmp / "appearance_static.scene"
    p.write_text(ts.HEAD + "material type=metal albedo=0.9,0.6,0.3 roughness=0.2\nsphere center=1.2,0,0 radius=0.5 material=1\nmesh path=tri2.obj material=0\n")
    return ts.load(p, str(tmp))


TEXTURE_SIZES = ((1, 1), (1, 7), (5, 3), (8, 8), (16, 2), (7, 16), (65536, 1))   # (width, height); the last one hits the 16-level cap


class Quads:
    """A description built in memory: one unit quad per texture, side by side in the plane z = 0, each under its own metallic-roughness
    material whose base colour is that texture; lit by the gradient background."""

    def __init__(self, sizes=TEXTURE_SIZES, seed=5):
        rng = np.random.default_rng(seed)
        n = len(sizes)
        fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
        self.pixels = [rng.random((h, w, 4), dtype=np.float32) for w, h in sizes]
        self._textures = (pt.PtrTexture * n)()
        self._materials = (pt.PtrMaterial * n)()
        self._meshes = (pt.PtrMeshDesc * n)()
        self._keep = []
        for i in range(n):
            t = self._textures[i]
            t.rgba, t.width, t.height = self.pixels[i].ctypes.data_as(fp), sizes[i][0], sizes[i][1]
            t.wrapS, t.wrapT, t.filter = i % 3, (i + 1) % 3, i % 2
            m = self._materials[i]
            m.typeEta[0], m.typeEta[1] = float(pt_type_pbr()), 1.5
            for k, v in enumerate((1.0, 1.0, 1.0, 0.6)):
                m.baseColorRoughness[k] = v
            for k in range(4):
                m.textureIndices0[k] = m.textureIndices1[k] = NONE
            m.textureIndices0[0] = i
            for k, v in enumerate((0.0, 0.6, 1.0, 1.0)):
                m.pbrParams[k] = v
            m.pbrExtras[0] = 1.0
            for r, row in enumerate(((1, 0, 0, 0), (0, 1, 0, 0)) * 6):
                for k, v in enumerate(row):
                    m.textureTransform[r][k] = float(v)
            x = 1.2 * (i - (n - 1) / 2)
            pos = np.array([(x - 0.5, -0.5, 0), (x + 0.5, -0.5, 0), (x + 0.5, 0.5, 0), (x - 0.5, 0.5, 0)], np.float32)
            nrm = np.tile(np.array([(0, 0, 1)], np.float32), (4, 1))
            uv = np.array([(0, 1), (1, 1), (1, 0), (0, 0)], np.float32) * np.float32(1.5)
            idx = np.array([0, 1, 2, 0, 2, 3], np.uint32)
            self._keep.append((pos, nrm, uv, idx))
            d = self._meshes[i]
            d.positions, d.normals, d.indices = pos.ctypes.data_as(fp), nrm.ctypes.data_as(fp), idx.ctypes.data_as(up)
            d.vertexCount, d.indexCount, d.materialIndex = 4, 6, i
            d.localToWorld[:] = np.eye(4, dtype=np.float32).reshape(-1).tolist()
            d.uv0 = uv.ctypes.data_as(fp)
        self.desc = pt.PtrSceneDesc()
        self.desc.materials, self.desc.materialCount = C.cast(self._materials, C.POINTER(pt.PtrMaterial)), n
        self.desc.meshes, self.desc.meshCount = C.cast(self._meshes, C.POINTER(pt.PtrMeshDesc)), n
        self.desc.textures, self.desc.textureCount = C.cast(self._textures, C.POINTER(pt.PtrTexture)), n

    def settings(self, base, metal=True):
        """`base` (the settings of any loaded scene) looking at the quads from +z, 32 x 24."""
        s = base.copy()
        s.width, s.height, s.maxDepth = 32, 24, 3
        s.cameraTarget[:] = [0.0, 0.0, 0.0]
        s.cameraDistance, s.cameraYaw, s.cameraPitch, s.cameraVerticalFov = 9.0, float(np.pi / 2), 0.0, 50.0
        s.metalSemantics = METAL if metal else 0
        return s


def pt_type_pbr():
    return 7   # PTR_MAT_PBR of include/ptr_abi.h
