// Material textures of the metallic-roughness model (PTR_METAL_PBR): storage, filtering, and the per-hit material the
// reference's Metal kernel builds from them (shaders/pathtrace.metal:5919-6400, helpers 108-198, 583-940, 2923-3216).
//
// The reference samples through the GPU's texture units (trilinear / anisotropic, `gradient2d` at the first hit from Igehy ray
// differentials, ray cones afterwards).  A software path has to fix its own filtering rule, and this is it - the same rule the
// oracle restates:
//   * storage: linear RGBA32F (sRGB decoded at load), every texture with its full mip chain (2x2 box filter, odd sizes clamp the
//     second tap), all levels of all textures in ONE float4 array in HBM;
//   * level of detail: ray cones only (ray_cone_lod_from_footprint, :162-176): log2(footprint x uvPerWorld x max(W, H));
//   * filtering: bilinear inside a level (texel centres at (i + 0.5) / W, wrap per the glTF sampler), linear between the two
//     nearest levels; NEAREST samplers read one texel of the rounded level.
// What the reference derives from ray differentials at the first hit (anisotropic sampling, the normal-variance term of the
// roughness widening) runs under PTR_METAL_RAY_DIFF only, at the first mesh hit of a camera ray (wavefront.hip firstHitUvGrads):
//   * level of detail from the uv gradients (material_texture_lod_from_gradients, :3143-3177), the ray cone where they give none;
//   * `gradient2d` sampling, which the hardware defines, is fixed as the reference formula of EXT_texture_filter_anisotropic:
//     Px = |(dudx W, dvdx H)|, Py = |(dudy W, dvdy H)|, Pmax / Pmin their max / min, Nt = min(ceil(Pmax / max(Pmin, 1e-6)), A),
//     lambda = clamp(log2(Pmax / Nt), 0, maxMip); the mean, summed in tap order, of Nt taps of the filter above at lambda, tap i at
//     uv + ((i + 0.5) / Nt - 0.5) g, g the uv gradient of the longer axis (x on a tie).  A = 8 (the reference's maxAnisotropy) for
//     LINEAR textures with more than one level, else 1; a NEAREST texture reads one texel of the rounded lambda.
#pragma once

#include "device_types.h"
#include "vec.h"

namespace ptrk {

constexpr uint32_t kNoTexture = 0xFFFFFFFFu;

// per-texture record in HBM: 5 uint4
//   [0] = (width, height, mipCount, wrapS | wrapT << 2 | filter << 4)   [1..4] = texel offset of levels 0..15 in the texel array
constexpr uint32_t kTexInfoVec4 = 5u;

struct TexLevel {
    uint32_t offset, width, height;
};

// level `level` of the texture whose record starts at `record` (record[0] = head)
__device__ __forceinline__ TexLevel texLevelOf(const uint4* record, uint32_t level, uint4 head) {
    const uint4 offs = record[1u + (level >> 2)];
    const uint32_t l = level & 3u;
    TexLevel r;
    r.offset = l == 0u ? offs.x : (l == 1u ? offs.y : (l == 2u ? offs.z : offs.w));
    r.width = max(head.x >> level, 1u);
    r.height = max(head.y >> level, 1u);
    return r;
}
__device__ __forceinline__ TexLevel texLevel(const SceneView& sc, uint32_t tex, uint32_t level, uint4 head) {
    return texLevelOf(sc.texInfo + tex * kTexInfoVec4, level, head);
}

__device__ __forceinline__ int texWrap(int i, int n, uint32_t mode) {
    if (mode == 1u) return min(max(i, 0), n - 1);
    if (mode == 2u) {
        const int period = 2 * n;
        int j = i % period;
        if (j < 0) j += period;
        return j < n ? j : period - 1 - j;
    }
    int j = i % n;
    return j < 0 ? j + n : j;
}

// `texels`: the array the level's offset counts from
__device__ __forceinline__ float4 texBilinear(const float4* texels, const TexLevel& L, float u, float v, uint32_t flags) {
    const uint32_t wrapS = flags & 3u, wrapT = (flags >> 2) & 3u;
    const int W = static_cast<int>(L.width), H = static_cast<int>(L.height);
    if (((flags >> 4) & 1u) == 0u) {   // NEAREST
        const int x = texWrap(static_cast<int>(floorf(u * static_cast<float>(W))), W, wrapS);
        const int y = texWrap(static_cast<int>(floorf(v * static_cast<float>(H))), H, wrapT);
        return texels[L.offset + static_cast<uint32_t>(y) * L.width + static_cast<uint32_t>(x)];
    }
    const float fx = u * static_cast<float>(W) - 0.5f, fy = v * static_cast<float>(H) - 0.5f;
    const float x0f = floorf(fx), y0f = floorf(fy);
    const float tx = fx - x0f, ty = fy - y0f;
    const int x0 = texWrap(static_cast<int>(x0f), W, wrapS), x1 = texWrap(static_cast<int>(x0f) + 1, W, wrapS);
    const int y0 = texWrap(static_cast<int>(y0f), H, wrapT), y1 = texWrap(static_cast<int>(y0f) + 1, H, wrapT);
    const float4* base = texels + L.offset;
    const float4 c00 = base[static_cast<uint32_t>(y0) * L.width + static_cast<uint32_t>(x0)];
    const float4 c10 = base[static_cast<uint32_t>(y0) * L.width + static_cast<uint32_t>(x1)];
    const float4 c01 = base[static_cast<uint32_t>(y1) * L.width + static_cast<uint32_t>(x0)];
    const float4 c11 = base[static_cast<uint32_t>(y1) * L.width + static_cast<uint32_t>(x1)];
    const float ix = 1.0f - tx, iy = 1.0f - ty;
    return make_float4((c00.x * ix + c10.x * tx) * iy + (c01.x * ix + c11.x * tx) * ty, (c00.y * ix + c10.y * tx) * iy + (c01.y * ix + c11.y * tx) * ty,
                       (c00.z * ix + c10.z * tx) * iy + (c01.z * ix + c11.z * tx) * ty, (c00.w * ix + c10.w * tx) * iy + (c01.w * ix + c11.w * tx) * ty);
}

// Linear between the two nearest levels of a chain of `levels` (lod clamped to [0, levels - 1]); bilinear(l) filters level l.
template <typename Bilinear>
__device__ __forceinline__ float4 texTrilinear(uint32_t levels, float lod, Bilinear bilinear) {
    const float maxMip = static_cast<float>(levels - 1u);
    const float l = fminf(fmaxf(lod, 0.0f), maxMip);
    const float l0f = floorf(l);
    const uint32_t l0 = static_cast<uint32_t>(l0f), l1 = min(l0 + 1u, levels - 1u);
    const float f = l - l0f;
    const float4 a = bilinear(l0);
    if (!(f > 0.0f) || l1 == l0) return a;
    const float4 b = bilinear(l1);
    return make_float4(a.x + (b.x - a.x) * f, a.y + (b.y - a.y) * f, a.z + (b.z - a.z) * f, a.w + (b.w - a.w) * f);
}

// sample_material_texture_level with the filtering rule above; `fallback` when the slot has no texture
__device__ __forceinline__ float4 texSample(const SceneView& sc, uint32_t tex, float u, float v, float lod, float4 fallback) {
    if (tex == kNoTexture || tex >= sc.textureCount) return fallback;
    const uint4 head = sc.texInfo[tex * kTexInfoVec4];
    const float maxMip = static_cast<float>(head.z - 1u);
    if (((head.w >> 4) & 1u) == 0u) {
        const float l = fminf(fmaxf(lod, 0.0f), maxMip);
        return texBilinear(sc.texels, texLevel(sc, tex, static_cast<uint32_t>(floorf(l + 0.5f)), head), u, v, head.w);
    }
    return texTrilinear(head.z, lod, [&](uint32_t level) { return texBilinear(sc.texels, texLevel(sc, tex, level, head), u, v, head.w); });
}

// ray_cone_lod_from_footprint (:162-176)
__device__ __forceinline__ float texLod(const SceneView& sc, uint32_t tex, float uvPerWorld, float footprintWorld) {
    if (tex == kNoTexture || tex >= sc.textureCount) return 0.0f;
    const uint4 head = sc.texInfo[tex * kTexInfoVec4];
    if (head.x == 0u || head.y == 0u) return 0.0f;
    if (head.z <= 1u || uvPerWorld <= 0.0f || footprintWorld <= 0.0f) return 0.0f;
    const float maxRes = fmaxf(static_cast<float>(head.x), static_cast<float>(head.y));
    const float texelFootprint = footprintWorld * uvPerWorld * maxRes;
    const float lod = log2f(fmaxf(texelFootprint, 1.0e-7f));
    return fminf(fmaxf(lod, 0.0f), static_cast<float>(head.z - 1u));
}

// decode_normal_map (:108-127), flipGreen = false
__device__ __forceinline__ f3 decodeNormalMap(f3 s, float normalScale, float& outLength) {
    f3 n = s * 2.0f - mk3(1.0f);
    n.x *= normalScale;
    n.y *= normalScale;
    outLength = length(n);
    const float xyLen2 = n.x * n.x + n.y * n.y;
    n.z = sqrtf(smax(1.0f - xyLen2, 0.0f));
    const float len2 = dot(n, n);
    if (len2 > 1.0e-12f) {
        n = n * (1.0f / sqrtf(len2));
    } else {
        n = mk3(0.0f, 0.0f, 1.0f);
    }
    return n;
}

// PTR_METAL_RAY_DIFF: the first-hit uv gradients of the two uv sets, set[k] = (dudx, dvdx, dudy, dvdy); bit k of `valid`: set k has them
struct UvGrads {
    float4 set[2];
    uint32_t valid;
};

// One texture slot's sampling context (make_pbr_texture_sampling_context, :3018-3056): transformed coordinates of the slot's uv set,
// its uv-per-world scale and, with PTR_METAL_RAY_DIFF at the first hit, its uv gradients through the transform's linear part.
struct TexSlot {
    float u, v, uvPerWorld;
    float dudx, dvdx, dudy, dvdy;
    bool grad;
};

__device__ __forceinline__ TexSlot texSlot(const float4* mraw, uint32_t slot, uint32_t uvSet, float2 uv0, float2 uv1, float perWorld0, float perWorld1,
                                           const UvGrads& grads) {
    // rows of KHR_texture_transform live behind the compact material record: raw[2*slot], raw[2*slot + 1] (xyz)
    f3 row0 = mk3(mraw[2u * slot]), row1 = mk3(mraw[2u * slot + 1u]);
    const float linearSum = (fabsf(row0.x) + fabsf(row0.y)) + (fabsf(row1.x) + fabsf(row1.y));
    if (!finite3(row0) || !finite3(row1) || !(linearSum > 1.0e-8f)) {   // pbr_texture_transform_rows (:2942-2983)
        row0 = mk3(1.0f, 0.0f, 0.0f);
        row1 = mk3(0.0f, 1.0f, 0.0f);
    }
    const float2 uv = uvSet == 0u ? uv0 : uv1;
    const float perWorld = uvSet == 0u ? perWorld0 : perWorld1;
    TexSlot t;
    t.u = (row0.x * uv.x + row0.y * uv.y) + row0.z;
    t.v = (row1.x * uv.x + row1.y * uv.y) + row1.z;
    const float sx = sqrtf(row0.x * row0.x + row1.x * row1.x), sy = sqrtf(row0.y * row0.y + row1.y * row1.y);
    t.uvPerWorld = perWorld * smax(smax(sx, sy), 1.0e-6f);   // pbr_transform_uv_per_world (:3002-3009)
    // pbr_transform_uv_gradient (:2991-2996); gradients that stop being finite are dropped
    const float4 g = uvSet == 0u ? grads.set[0] : grads.set[1];
    t.dudx = row0.x * g.x + row0.y * g.y;
    t.dvdx = row1.x * g.x + row1.y * g.y;
    t.dudy = row0.x * g.z + row0.y * g.w;
    t.dvdy = row1.x * g.z + row1.y * g.w;
    t.grad = ((grads.valid >> uvSet) & 1u) != 0u && isfinite(t.dudx) && isfinite(t.dvdx) && isfinite(t.dudy) && isfinite(t.dvdy);
    if (!t.grad) t.dudx = t.dvdx = t.dudy = t.dvdy = 0.0f;
    return t;
}

// max(|dudx|, |dvdx|, |dudy|, |dvdy|) of a slot with gradients (:3110-3112)
__device__ __forceinline__ float texGradMag(const TexSlot& t) { return fmaxf(fmaxf(fabsf(t.dudx), fabsf(t.dvdx)), fmaxf(fabsf(t.dudy), fabsf(t.dvdy))); }

// material_texture_lod_from_gradients (:3143-3177): false when the slot has no gradients, the texture one level, or rho is not positive
// and finite - the caller then takes the cone's LOD (material_texture_lod_with_fallback, :3179-3216).  head: the texture's record head
__device__ __forceinline__ bool texGradLod(uint4 head, const TexSlot& t, float& lod) {
    if (!t.grad || head.x == 0u || head.y == 0u || head.z <= 1u) return false;
    const float W = static_cast<float>(head.x), H = static_cast<float>(head.y);
    const float rho = fmaxf(fmaxf(fabsf(t.dudx) * W, fabsf(t.dvdx) * H), fmaxf(fabsf(t.dudy) * W, fabsf(t.dvdy) * H));
    if (!isfinite(rho) || !(rho > 0.0f)) return false;
    const float l = log2f(fmaxf(rho, 1.0e-8f));
    if (!isfinite(l)) return false;
    lod = fminf(fmaxf(l, 0.0f), static_cast<float>(head.z - 1u));
    return true;
}

// The taps of the gradient sample (`gradient2d`) by the rule of the header comment: level `lod`, `nt` taps along (gu, gv)
constexpr uint32_t kTexMaxAniso = 8u;
__device__ __forceinline__ void texAniso(uint4 head, float dudx, float dvdx, float dudy, float dvdy, float& lod, float& nt, float& gu, float& gv) {
    const float W = static_cast<float>(head.x), H = static_cast<float>(head.y);
    const float xw = dudx * W, xh = dvdx * H, yw = dudy * W, yh = dvdy * H;
    const float px = sqrtf(xw * xw + xh * xh), py = sqrtf(yw * yw + yh * yh);
    const bool xMajor = px >= py;
    const float pMax = xMajor ? px : py, pMin = xMajor ? py : px;
    const float maxAniso = (((head.w >> 4) & 1u) != 0u && head.z > 1u) ? static_cast<float>(kTexMaxAniso) : 1.0f;
    nt = fmaxf(fminf(ceilf(pMax / fmaxf(pMin, 1.0e-6f)), maxAniso), 1.0f);
    lod = fminf(fmaxf(log2f(pMax / nt), 0.0f), static_cast<float>(head.z - 1u));
    gu = xMajor ? dudx : dudy;
    gv = xMajor ? dvdx : dvdy;
}

// The mean, summed in tap order, of `nt` (1..kTexMaxAniso) taps of the filter at level `lod`, tap i at uv + ((i + 0.5) / nt - 0.5) g; a
// NEAREST texture reads one texel of the rounded level at uv.  nt = 1 is texSample's level sample, to the bit.
__device__ __forceinline__ float4 texTaps(const SceneView& sc, uint32_t tex, uint4 head, float u, float v, float lod, float nt, float gu, float gv) {
    if (((head.w >> 4) & 1u) == 0u) {
        const float l = fminf(fmaxf(lod, 0.0f), static_cast<float>(head.z - 1u));
        return texBilinear(sc.texels, texLevel(sc, tex, static_cast<uint32_t>(floorf(l + 0.5f)), head), u, v, head.w);
    }
    const uint32_t taps = static_cast<uint32_t>(nt);
    float4 sum = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll 1
    for (uint32_t i = 0u; i < taps; ++i) {
        const float o = (static_cast<float>(i) + 0.5f) / nt - 0.5f;
        const float tu = u + o * gu, tv = v + o * gv;
        const float4 c = texTrilinear(head.z, lod, [&](uint32_t level) { return texBilinear(sc.texels, texLevel(sc, tex, level, head), tu, tv, head.w); });
        sum.x += c.x;
        sum.y += c.y;
        sum.z += c.z;
        sum.w += c.w;
    }
    return make_float4(sum.x / nt, sum.y / nt, sum.z / nt, sum.w / nt);
}

// The gradient sample; `fallback` when the slot has no texture
__device__ __forceinline__ float4 texSampleGrad(const SceneView& sc, uint32_t tex, float u, float v, float dudx, float dvdx, float dudy, float dvdy,
                                                float4 fallback) {
    if (tex == kNoTexture || tex >= sc.textureCount) return fallback;
    const uint4 head = sc.texInfo[tex * kTexInfoVec4];
    float lod, nt, gu, gv;
    texAniso(head, dudx, dvdx, dudy, dvdy, lod, nt, gu, gv);
    return texTaps(sc, tex, head, u, v, lod, nt, gu, gv);
}

// One lookup of a slot: with `aniso` the gradient sample (sample_material_texture_filtered with non-zero gradients, :3091-3127), else the
// level sample (sample_material_texture_level) at the gradients' LOD or, where they give none, the LOD of the cone's surface footprint.
// Without gradients this is texSample at texLod, to the bit.
__device__ __forceinline__ float4 texLookup(const SceneView& sc, uint32_t tex, const TexSlot& t, bool aniso, float footprint, float4 fallback) {
    if (tex == kNoTexture || tex >= sc.textureCount) return fallback;
    const uint4 head = sc.texInfo[tex * kTexInfoVec4];
    float lod, nt = 1.0f, gu = 0.0f, gv = 0.0f;
    if (aniso) {
        texAniso(head, t.dudx, t.dvdx, t.dudy, t.dvdy, lod, nt, gu, gv);
    } else if (!texGradLod(head, t, lod)) {
        lod = texLod(sc, tex, t.uvPerWorld, footprint);
    }
    return texTaps(sc, tex, head, t.u, t.v, lod, nt, gu, gv);
}

}  // namespace ptrk
