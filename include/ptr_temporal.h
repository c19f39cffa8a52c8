/* Temporal accumulation for sequences: each frame's colour is blended with the history of the surface point it shows, found by
 * reprojecting that point along the motion of the surface and of the camera.
 *
 * A sequence of low-sample frames flickers because each frame's residual noise is independent of the last frame's; ptr_denoise is
 * spatial only.  A PtrTemporal handle carries, per pixel, an accumulated colour and the number of frames in it from step to step.  One
 * step is: k_surface (csrc/kernels/wavefront.hip) traces the frame's first hits and writes three records per pixel, one of them the
 * position the hit point had in the pose of the previous step; k_temporal_accumulate (csrc/kernels/temporal.hip) blends.  Host:
 * csrc/host/temporal.cpp.  Restatement in numpy (the tests' reference): tests/temporal_ref.py.  Kernels and restatement are written from
 * the text below.
 *
 * ---- The records (k_surface) -----------------------------------------------------------------------------------------------------------
 *
 * One surface per pixel: the one ptr_render_aovs(sample_index 0) reports under `settings` (ptr_abi.h: the rule at ptr_render_aovs) - the
 * closest hit of the camera ray of sample 0, or with PTR_METAL_PBR on a textured scene the first surface along it the alpha test keeps.
 * "The ray", origin, direction, (u, v) and P below are those of the segment that ends on that surface; t is the rule's distance, the sum
 * of the segments' hit distances.  Per pixel three float4 records:
 *   R0 = (X.xyz, bits(id))          R1 = (n.xyz, t)          R2 = (Xprev.xyz, bits(hit word))
 *   hit word  the traversal's word for the primitive: 0xFFFFFFFF on a miss, else the leaf-order index (bit 31 set for a sphere)
 *   id        primType << 30 | index: the mesh index (primType 0), the sphere index (1) or the rectangle index (2), as at upload; 0 on a miss
 *   n, t      the unit normal ptr_render_aovs encodes (before n * 0.5 + 0.5) and its distance (normal.w); n = 0 and t = 0 on a miss
 *   X         the hit point interpolated from the rows the renderer traces, NOT origin + t * direction:
 *               triangle (of a mesh or of a rectangle) with leaf-order rows a0 = v0, a1 = v0 - v1, a2 = v2 - v0 and the traversal's own
 *               barycentrics (u, v):   X = (a0 - u a1) + v a2
 *               sphere with row (c, r0) and P = origin + t * direction:   X = c + (P - c) * (r / r0)   with (c, r) = (c, r0), this row
 *             X = 0 on a miss
 *   Xprev     the same expression, with the same (u, v) or the same P, c and r0, on the rows the handle's pose snapshot holds:
 *               (p0 - u p1) + v p2     and     c' + (P - c) * (r' / r0)
 *             Without a snapshot (the first step, after a reset, and always for a scene that is not dynamic) the snapshot rows ARE the
 *             current rows.  When nothing moved, X and Xprev come from identical operations on identical values and are bitwise equal.
 * The two AOV buffers, when asked for, are written exactly as ptr_render_aovs(sample_index 0) writes them: same surface, same bits.
 *
 * ---- The filter (k_temporal_accumulate) ------------------------------------------------------------------------------------------------
 *
 * Image space only: one pixel per lane.  Inputs: the frame's colour c (W*H*3 floats); this step's R0, R1, R2; the previous step's R0 and
 * R1; the history, one float4 (rgb, length) per pixel; the cameras of this step and of the previous one as (o, ll, h, w) = origin,
 * lower-left corner, horizontal, vertical of the renderer's camera; the parameters.  Pixel (x, y), y = 0 the top row.
 *   dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z          cross(a, b) = (a.y b.z - a.z b.y,  a.z b.x - a.x b.z,  a.x b.y - a.y b.x)
 *   |a| = sqrt(dot(a, a))                              finite(v): v - v == 0
 *
 * 1. MISS pixel: hit word 0xFFFFFFFF, or a colour channel that is not finite.  out = c, length = 0, stored history (c, 0).  Done.
 * 2. NO HISTORY (the first step, or the first after a reset): out = c, length = 1, stored history (c, 1).  Done.
 * 3. Projection of a point Y through a camera (o, ll, h, w):
 *      d = Y - o;  cN = cross(h, w);  L = ll - o
 *      den = dot(d, cN);  num = dot(L, cN);  s = num / den          valid when s > 0 and s is finite
 *      r = d * s - L
 *      U = dot(r, h) / dot(h, h);  V = dot(r, w) / dot(w, w)
 *      f = (U * W, (1 - V) * H)                                     W, H as floats
 *    fc = X through this step's camera, fp = Xprev through the previous step's.  Either invalid: RESET (6).
 * 4. Sample position: sx = x + (fp.x - fc.x), sy = y + (fp.y - fc.y) (x, y as floats), which takes the sample's jitter out: zero motion
 *    gives sx = x exactly.  sx or sy not finite: RESET.
 *      x0 = floor(sx), ax = sx - x0;  y0 = floor(sy), ay = sy - y0
 *      taps k = 0..3 at (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1)
 *      weights b = (1 - ax) * (1 - ay),  ax * (1 - ay),  (1 - ax) * ay,  ax * ay
 * 5. A tap COUNTS when all of: b > 0; it is inside the image; its history length >= 1; its three history colours are finite; the id
 *    of the previous step's R0 there equals this pixel's id; dot(n_tap, n) >= normalCos with n_tap the previous R1 there and n this
 *    pixel's R1; |dot(Xprev - X_tap, n_tap)| <= planeTolerance * |Xprev - o_prev| with X_tap the previous R0 there.
 * 6. B = sum of b over the counting taps, Sc = sum of b * rgb_tap (per channel), Sn = sum of b * length_tap: each summed in tap order
 *    starting from 0.  If B > 0:
 *      hist = Sc / B;  N = Sn / B;  N' = min(N + 1, maxHistory);  a = 1 / N'
 *      out = hist + (c - hist) * a;  length = N'
 *    otherwise RESET: out = c, length = 1.
 * 7. Stored history: (out, length).
 *
 * All arithmetic is float32, unfused, in the order written, with correctly rounded division and square root.
 *
 * After a step its R0 and R1 become "previous", its camera the previous camera, and - for a dynamic scene - the renderer's triangle and
 * sphere rows are copied device to device into the handle's snapshot (48 B per triangle, 16 B per sphere).
 */
#ifndef PTR_TEMPORAL_H
#define PTR_TEMPORAL_H

#include "ptr_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct PtrTemporal PtrTemporal;

typedef struct PtrTemporalParams {
    uint32_t maxHistory;  /* 1..65535, default 32: the blend never weighs the new frame less than 1 / maxHistory */
    float normalCos;      /* -1..1, default 0.9: smallest cosine between a tap's normal and the pixel's */
    float planeTolerance; /* > 0, default 0.01: distance of Xprev from the tap's plane, as a fraction of its distance from the camera */
    uint32_t flags;       /* 0 */
} PtrTemporalParams;

typedef struct PtrTemporalInfo {
    uint32_t frameIndex;                        /* steps since create / reset, this one not counted */
    uint32_t hadHistory;                        /* 0: this was a first step */
    double surfaceMs, accumulateMs, snapshotMs; /* device events around k_surface, k_temporal_accumulate, the snapshot copy */
} PtrTemporalInfo;

void ptr_temporal_default_params(PtrTemporalParams* params);
/* Host only.  0, or 1 with a message for a value outside the ranges above (NaN included) or a null argument. */
int ptr_temporal_check_params(const PtrTemporalParams* params, char* err, size_t err_cap);

/* A handle for width x height frames of `scene`, static or dynamic, which must outlive it.  params NULL: the defaults.  The handle holds
 * 128 B per pixel, and for a dynamic scene 48 B per triangle and 16 B per sphere.  1 for a bad argument, 2 without a HIP device. */
int ptr_temporal_create(PtrDeviceScene* scene, uint32_t width, uint32_t height, const PtrTemporalParams* params, PtrTemporal** out, char* err,
                        size_t err_cap);
void ptr_temporal_release(PtrTemporal* temporal);
/* Drops the history and the pose snapshot: the next step is a first step. */
int ptr_temporal_reset(PtrTemporal* temporal);

/* One step on device buffers of the scene's device, asynchronous on `stream` (a hipStream_t; NULL = the default stream) unless info is
 * given, in which case the call waits for the step and reports its times.  settings: those of the frame in d_rgb (camera, width, height,
 * seed); the scene must be in the pose that frame was rendered in.  d_rgb and d_out_rgb hold W*H*3 floats and may be the same buffer
 * (the same address: two buffers that overlap otherwise are refused).
 * d_out_length (W*H floats), d_out_albedo and d_out_normal (W*H*4 floats each, 16 B aligned) may be NULL.  The step uses the scene's
 * traversal scratch like every call on a scene: calls on one scene do not overlap.  It never writes to the scene.
 * Refused (1) before any device work and with the history as it was: a null argument, settings of another width or height than the
 * handle's, a buffer that is not device memory of the scene's device, and d_rgb overlapping d_out_rgb at an offset. */
int ptr_temporal_step_device(PtrTemporal* temporal, const PtrSettings* settings, const void* d_rgb, void* d_out_rgb, void* d_out_length,
                             void* d_out_albedo, void* d_out_normal, void* stream, PtrTemporalInfo* info, char* err, size_t err_cap);
/* The same step on host buffers (out_rgb may alias rgb; out_length, out_albedo, out_normal, info may be NULL).  Synchronous. */
int ptr_temporal_step(PtrTemporal* temporal, const PtrSettings* settings, const float* rgb, float* out_rgb, float* out_length, float* out_albedo,
                      float* out_normal, PtrTemporalInfo* info, char* err, size_t err_cap);

/* ---- test-only probes ----
 * k_temporal_accumulate alone on host-given buffers, on `device`: rgb W*H*3; cur_records 3 * W*H*4 (R0, R1, R2 back to back);
 * prev_records 2 * W*H*4 (R0, R1); history W*H*4; cam_cur and cam_prev 12 floats each (o, ll, h, w); has_history 0 / 1.
 * Out: out_rgb W*H*3, out_length W*H, out_history W*H*4. */
int ptr_debug_temporal_accumulate(uint32_t width, uint32_t height, const PtrTemporalParams* params, int has_history, const float* rgb,
                                  const float* cur_records, const float* prev_records, const float* history, const float* cam_cur,
                                  const float* cam_prev, int device, float* out_rgb, float* out_length, float* out_history, char* err,
                                  size_t err_cap);
/* The three records of the last step, W*H*4 floats each (any may be NULL).  Non-zero before the first step. */
int ptr_debug_temporal_records(PtrTemporal* temporal, float* out_r0, float* out_r1, float* out_r2, char* err, size_t err_cap);
/* Host only: origin, lowerLeft, horizontal, vertical of the camera the renderer builds from `settings`. */
int ptr_debug_temporal_camera(const PtrSettings* settings, float* out);

#ifdef __cplusplus
}
#endif
#endif /* PTR_TEMPORAL_H */
