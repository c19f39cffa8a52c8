/*
 * ptr_appearance.h — change how a resident scene looks: whole materials (and with them emission and the rectangle-light table), the
 * pixels of material textures, and the pixels of the environment map.  The geometry calls (ptr_dynamic.h, ptr_deform.h,
 * ptr_deform_device.h, ptr_rebuild.h) move what a scene holds; these change its appearance, under the same rule: after a call every
 * device array is bit for bit what a fresh upload of the edited description produces.
 *
 * Shared by every call here:
 *   - `stream`, synchronisation and the optional info struct behave as in ptr_scene_set_mesh_transforms: the device work is enqueued on
 *     `stream` (a hipStream_t; NULL: the default stream) and the call returns after a stream synchronisation, so the caller's arrays are
 *     free again and the next render sees the new scene.  `info` may be NULL.
 *   - A refusal happens before any device work that writes what the renderer reads, leaves the scene unchanged, returns 1, and its
 *     message starts with the function's name.
 *   - Nothing tells a Frame or a Temporal about the change: the caller resets them, as after a geometry update.
 *
 * ptr_scene_set_materials replaces the whole PtrMaterial of each named index (the material count does not change) and re-derives what
 * the upload derives from materials: the compact rows, the per-material texture rows of a textured scene, the material-type mask (so the
 * k_shade instantiation a render launches follows), the random-walk flag, the shade key in the meta word of every triangle row whose
 * material changed type (k_app_rekey: one triangle per lane over all rows, a per-material key table of at most 65,536 bytes, a store only
 * where the key differs; launched only when a named material changed type; a dynamic scene's object-space corner rows, whose w words
 * the bake copies into the triangle rows, are rekeyed by the same kernel), and the rectangle-light table: a rectangle can become a
 * light, stop being one (by type or by emission 0), or change emission; the table's size and order, lightIndexByRect, the light count
 * ptr_scene_info reports and whether connections to lights are settled are recomputed as the upload computes them.
 * It works on any scene, static ones included, with one exception: when a rectangle uses a named material the scene must have been
 * uploaded with PTR_DYNAMIC_PRIMITIVES (ptr_deform.h), which is what keeps the rectangles' records and the places of their triangles on
 * the host.  There is no new upload flag.
 * Refused: a null list or a count of 0; an index out of range or named twice; a non-finite float in a material; a texture index (base
 * colour, metallic-roughness, normal, occlusion, emissive, transmission) that is neither 0xFFFFFFFF nor below the scene's texture count;
 * any such index other than 0xFFFFFFFF on a scene uploaded without textures; a rectangle that uses a named material on a scene without
 * PTR_DYNAMIC_PRIMITIVES.
 *
 * ptr_scene_set_textures / ptr_scene_set_textures_device give new level-0 pixels (linear RGBA float, as PtrTexture) for the named
 * textures.  Width and height must be the upload's; wrap and filter may change.  The host call stages the pixels (and looks at every
 * component on the way); the device call reads the caller's float32 array where it is, after the pointer checks of
 * ptr_scene_set_mesh_vertices_device (4 B alignment, plain device memory of the scene's device, the allocation's size: host, managed and
 * another device's memory are refused by name) and a finiteness kernel that runs before anything the renderer reads is written.  Then
 * k_app_mip_level writes the chain level by level, one texel per lane and one launch per level, with the upload's arithmetic to the bit:
 * ((a + b) + (c + d)) * 0.25f, the second tap clamped on odd sizes, each size halved down to at least 1, at most 16 levels.  The
 * offsets of the texture records stay as they are.
 * Refused: a scene without textures; a null list or a count of 0; an index out of range or named twice; null pixels; another size; a
 * non-finite component; for the device call a pointer that fails the checks above.
 *
 * ptr_scene_set_environment / ptr_scene_set_environment_device give new pixels for the environment map at the upload's size.  Both run
 * the same device steps: (a) the pixels; (b) luminance times cell weight per texel and the row sums, one row per lane, summed left to
 * right; (c) the total, one running float sum over all texels in scan order (one lane adds while its workgroup stages rows through
 * LDS: the order decides the bits of the pdfs); (d) the marginal and the per-row conditional alias tables by Vose's method exactly as
 * the upload builds them (work lists consumed from the back, threshold 1 - 1e-7, the same tails), one workgroup per row with the row's
 * scaled values and both work lists in LDS and one lane running the loop; (e) the per-texel pdf; (f) when a render with
 * PTR_METAL_ENV_LOD has built the map's mip chain, its levels 1 and up, by the kernel of the textures.  The per-row cell weights depend on
 * the size alone and are computed on the host, as at upload.
 * A map with no positive radiance is not an error: a fresh upload renders it without environment sampling, so the call turns sampling
 * off, and a later call with radiance turns it on again.
 * Refused: a scene uploaded without an environment map; a size other than the upload's; null pixels; a non-finite component; a width or
 * a height above PTR_APPEARANCE_ENV_MAX_DIM (a row's scaled values and its two work lists take 12 B per entry of LDS: 48 KB at the cap);
 * for the device call a pointer that fails the checks above.
 *
 * Out of scope: adding or removing materials, textures or primitives; changing a texture's or the environment's size; the one-shot
 * ptr_render_multi* (a frame on several devices takes these calls through ptr_multi_appearance.h); the command-line program; the
 * geometry cache.
 */
#ifndef PTR_APPEARANCE_H
#define PTR_APPEARANCE_H

#include "ptr_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { PTR_APPEARANCE_ENV_MAX_DIM = 4096 }; /* most columns, and most rows, of an environment map the environment calls accept */

typedef struct PtrAppearanceInfo {
    double totalSeconds;   /* wall clock of the call */
    double stagingMs;      /* host: validation, derivation of the rows, staging copies */
    double kernelMs[6];    /* materials: [0] copies of the rows, [1] the rekey.  textures: [0] copies and the finiteness check, [1] the mip
                              chains.  environment: [0] pixels and check, [1] weights and row sums, [2] the sequential total, [3] alias
                              tables, [4] pdf, [5] mip chain */
    uint64_t rowsRekeyed;  /* triangle rows whose meta word was rewritten */
    uint64_t texelsWritten; /* texels of every level written (textures, environment pixels and its mip chain) */
    uint32_t lightsBefore, lightsAfter; /* rectangle lights */
    uint32_t envSampling;  /* 1: the scene samples its environment map after the call */
    uint32_t pad;
} PtrAppearanceInfo;

typedef struct PtrTextureUpdate {
    uint32_t textureIndex, width, height; /* width, height: as at upload */
    uint32_t wrapS, wrapT, filter;        /* as PtrTexture */
    const float* rgba;                    /* width * height * 4; HOST for ptr_scene_set_textures, DEVICE for ptr_scene_set_textures_device */
} PtrTextureUpdate;

int ptr_scene_set_materials(PtrDeviceScene* scene, const uint32_t* indices, const PtrMaterial* materials, uint32_t count, void* stream,
                            PtrAppearanceInfo* info, char* err, size_t err_cap);

int ptr_scene_set_textures(PtrDeviceScene* scene, const PtrTextureUpdate* textures, uint32_t count, void* stream, PtrAppearanceInfo* info, char* err,
                           size_t err_cap);
int ptr_scene_set_textures_device(PtrDeviceScene* scene, const PtrTextureUpdate* textures, uint32_t count, void* stream, PtrAppearanceInfo* info,
                                  char* err, size_t err_cap);

int ptr_scene_set_environment(PtrDeviceScene* scene, const float* rgba, uint32_t width, uint32_t height, void* stream, PtrAppearanceInfo* info,
                              char* err, size_t err_cap);
int ptr_scene_set_environment_device(PtrDeviceScene* scene, const float* rgba, uint32_t width, uint32_t height, void* stream, PtrAppearanceInfo* info,
                                     char* err, size_t err_cap);

/* ---- test-only probe ----
 * The arrays the calls above write, as the scene holds them now.  *size_out in bytes; out may be NULL (size only).  1 for a null
 * argument or an unknown selector, 2 for a buffer that is too small, 3 for a failed copy.  PTR_APPEARANCE_SCALARS: six uint32_t
 * {materialTypes, rectLightCount, settleRectLights, hasRandomWalkMaterial, envSampling, envMipLevels}.  The environment tables are empty
 * while the scene does not sample its map; PTR_APPEARANCE_ENV_MIPS is the chain's record and its levels 1 and up (empty: not built). */
enum PtrAppearanceArray {
    PTR_APPEARANCE_MATERIALS = 0,
    PTR_APPEARANCE_MATERIAL_TEX = 1,
    PTR_APPEARANCE_RECT_LIGHTS = 2,
    PTR_APPEARANCE_LIGHT_INDEX_BY_RECT = 3,
    PTR_APPEARANCE_TEXELS = 4,
    PTR_APPEARANCE_TEX_INFO = 5,
    PTR_APPEARANCE_ENV_RGBA = 6,
    PTR_APPEARANCE_ENV_COND = 7,
    PTR_APPEARANCE_ENV_MARG = 8,
    PTR_APPEARANCE_ENV_PDF = 9,
    PTR_APPEARANCE_ENV_MIPS = 10,
    PTR_APPEARANCE_SCALARS = 11
};
int ptr_debug_appearance_arrays(PtrDeviceScene* scene, uint32_t which, void* out, uint64_t cap_bytes, uint64_t* size_out);

#ifdef __cplusplus
}
#endif
#endif /* PTR_APPEARANCE_H */
