// The primary-ray bounds cull of a plain frame (renderPass in hip_backend.cpp): the pixel rectangle outside which no camera ray of any
// sample can reach anything in the scene.  Pixels outside it are resolved by k_background and never enter the path pool.
// Plain C++ (no HIP): the CPU test suite checks the rule against a float64 projection and against rays (tests/test_background_cull_host.py).
#pragma once

#include <cstdint>

namespace ptr {

// The fields of CameraParams (kernels/device_types.h) the rule reads, as buildCamera fills them.
struct CullCamera {
    const float *origin, *lowerLeft, *horizontal, *vertical, *u, *v;
    float lensRadius;
};

// World box of everything a ray can hit: the triangles in the tree, the oversize triangles kept out of it, the spheres with their radii.
struct WorldBounds {
    double lo[3] = {0.0, 0.0, 0.0}, hi[3] = {0.0, 0.0, 0.0};
    bool valid = false;   // false: unknown (an empty scene, something not finite): nothing is culled
    void add(const double p[3], double pad = 0.0);
};

// triData: 12 floats per triangle (v0 | ., v0 - v1 | ., v2 - v0 | .), sphereData: 4 floats per sphere (centre, radius) - the leaf-order
// arrays of SceneGeometry, which hold every primitive whether or not the tree does.  The box is padded by a few float roundings.
WorldBounds boundsOfPrimitives(const float* triData, uint64_t triCount, const float* sphereData, uint64_t sphereCount);

struct CullRect {
    bool cull = false;                         // false: every pixel is traced
    uint32_t x0 = 0, x1 = 0, y0 = 0, y1 = 0;   // (with cull) pixels outside [x0, x1) x [y0, y1) cannot see the scene
    bool inside(uint32_t x, uint32_t y) const { return x >= x0 && x < x1 && y >= y0 && y < y1; }
    bool operator==(const CullRect& o) const { return cull == o.cull && x0 == o.x0 && x1 == o.x1 && y0 == o.y0 && y1 == o.y1; }
};

// The rectangle for cameraRay's rays (wavefront.hip: d = lowerLeft + u horizontal + (1 - v') vertical - origin, thin lens included) of
// a width x height image.  Conservative, never tight: the bounding rectangle of the eight projected corners plus one whole pixel on
// every side; with a thin lens the box is first grown by the lens radius and the rectangle widened by lensRadius / |horizontal| in u
// and lensRadius / |vertical| in v (a lens ray from origin + offset through focal-plane point P is the pinhole ray through P - offset,
// translated by offset, and the offsets lie in the focal plane's directions).  No culling when a corner of the grown box is not in
// front of the camera by more than the lens radius, the camera is inside the grown box, anything is not finite, or the rectangle
// covers the whole image.
CullRect backgroundCullRect(const CullCamera& cam, uint32_t width, uint32_t height, const WorldBounds& bounds);

}  // namespace ptr
