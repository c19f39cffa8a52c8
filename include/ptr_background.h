/*
 * ptr_background.h — the primary-ray bounds cull of a plain frame (ptr_render, ptr_render_bands[_device], the partitions of
 * ptr_render_multi): pixels whose camera rays cannot reach anything in the scene are resolved by a kernel of their own and never
 * enter the path pool (csrc/host/background_cull.h).  The image does not depend on it, bit for bit;
 * PTR_BACKGROUND_CULL=0 turns it off.  Covariance, adaptive and resumable frames and counting renders trace every pixel.
 */
#ifndef PTR_BACKGROUND_H
#define PTR_BACKGROUND_H

#include "ptr_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Test-only, host-side (no GPU work): what a plain frame with `settings` does with the pixels of partition `part` of `parts`.  The
 * bounds are the ones `scene` holds (after a dynamic update: the refitted ones), or with scene NULL those of `desc`, whose geometry is
 * then prepared on the host as ptr_scene_upload prepares it.  count: the counting build (never culls).
 * out = {culling (1/0), x0, x1, y0, y1 (pixels outside [x0, x1) x [y0, y1) are background; zeros without culling), traced pixels of the
 * partition, background pixels of the partition, 0}; bounds (may be NULL) = {lo xyz, hi xyz, valid (1/0)} of the world box used. */
int ptr_background_debug_cull(const PtrDeviceScene* scene, const PtrSceneDesc* desc, const PtrSettings* settings, uint32_t part, uint32_t parts,
                              int count, uint32_t out[8], double bounds[7], char* err, size_t err_cap);

#ifdef __cplusplus
}
#endif
#endif /* PTR_BACKGROUND_H */
