#include "background_cull.h"

#include <algorithm>
#include <cmath>

namespace ptr {

namespace {

struct D3 {
    double x, y, z;
};
D3 operator+(D3 a, D3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
D3 operator-(D3 a, D3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
D3 operator*(double s, D3 a) { return {s * a.x, s * a.y, s * a.z}; }
double dot(D3 a, D3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
D3 cross(D3 a, D3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
D3 ld(const float* p) { return {p[0], p[1], p[2]}; }
bool finite(D3 a) { return std::isfinite(a.x) && std::isfinite(a.y) && std::isfinite(a.z); }

}  // namespace

void WorldBounds::add(const double p[3], double pad) {
    for (int a = 0; a < 3; ++a) {
        lo[a] = valid ? std::min(lo[a], p[a] - pad) : p[a] - pad;
        hi[a] = valid ? std::max(hi[a], p[a] + pad) : p[a] + pad;
    }
    valid = true;
}

WorldBounds boundsOfPrimitives(const float* triData, uint64_t triCount, const float* sphereData, uint64_t sphereCount) {
    WorldBounds b;
    for (uint64_t i = 0; i < triCount; ++i) {
        const float* t = triData + i * 12u;
        const double v0[3] = {t[0], t[1], t[2]};
        const double v1[3] = {v0[0] - t[4], v0[1] - t[5], v0[2] - t[6]};
        const double v2[3] = {v0[0] + t[8], v0[1] + t[9], v0[2] + t[10]};
        b.add(v0);
        b.add(v1);
        b.add(v2);
    }
    for (uint64_t i = 0; i < sphereCount; ++i) {
        const float* s = sphereData + i * 4u;
        const double c[3] = {s[0], s[1], s[2]};
        b.add(c, std::fabs(static_cast<double>(s[3])));
    }
    if (!b.valid) return b;
    // the kernels intersect in float: a hit may lie a few roundings outside the exact primitive
    double scale = 0.0;
    for (int a = 0; a < 3; ++a) scale = std::max(scale, std::max(std::fabs(b.lo[a]), std::fabs(b.hi[a])));
    const double pad = scale * 1.0e-5 + 1.0e-30;
    for (int a = 0; a < 3; ++a) {
        b.lo[a] -= pad;
        b.hi[a] += pad;
        if (!std::isfinite(b.lo[a]) || !std::isfinite(b.hi[a])) b.valid = false;
    }
    return b;
}

CullRect backgroundCullRect(const CullCamera& cam, uint32_t width, uint32_t height, const WorldBounds& bounds) {
    const CullRect none;
    if (!bounds.valid || width == 0u || height == 0u) return none;
    const D3 origin = ld(cam.origin), lowerLeft = ld(cam.lowerLeft), horizontal = ld(cam.horizontal), vertical = ld(cam.vertical);
    const double lens = cam.lensRadius > 0.0f ? static_cast<double>(cam.lensRadius) : 0.0;   // (cameraRay: a lens only when > 0)
    if (!finite(origin) || !finite(lowerLeft) || !finite(horizontal) || !finite(vertical) || !std::isfinite(cam.lensRadius)) return none;
    const double hh = dot(horizontal, horizontal), vv = dot(vertical, vertical);
    D3 axis = cross(horizontal, vertical);   // normal of the focal plane
    const double axisLength = std::sqrt(dot(axis, axis));
    if (!(hh > 0.0) || !(vv > 0.0) || !(axisLength > 0.0) || !std::isfinite(axisLength)) return none;
    axis = (1.0 / axisLength) * axis;
    // the (u, v) of a focal-plane point are read off along horizontal and vertical: they have to be perpendicular, as buildCamera makes them
    if (std::fabs(dot(horizontal, vertical)) > 1.0e-5 * std::sqrt(hh * vv)) return none;
    const D3 centre = (lowerLeft + 0.5 * horizontal) + 0.5 * vertical;
    double planeDepth = dot(axis, centre - origin);   // distance of the focal plane along the view axis
    if (planeDepth < 0.0) {
        axis = -1.0 * axis;
        planeDepth = -planeDepth;
    }
    if (!(planeDepth > 0.0) || !std::isfinite(planeDepth)) return none;
    if (lens > 0.0) {
        // the lens offsets (cam.u, cam.v) must lie in the focal plane for the margin below to hold
        const D3 lu = ld(cam.u), lv = ld(cam.v);
        if (!finite(lu) || !finite(lv)) return none;
        if (std::fabs(dot(axis, lu)) > 1.0e-5 * std::sqrt(dot(lu, lu)) || std::fabs(dot(axis, lv)) > 1.0e-5 * std::sqrt(dot(lv, lv))) return none;
    }

    double lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
        lo[a] = bounds.lo[a] - lens;
        hi[a] = bounds.hi[a] + lens;
        if (!std::isfinite(lo[a]) || !std::isfinite(hi[a]) || lo[a] > hi[a]) return none;
    }
    const double o[3] = {origin.x, origin.y, origin.z};
    if (o[0] >= lo[0] && o[0] <= hi[0] && o[1] >= lo[1] && o[1] <= hi[1] && o[2] >= lo[2] && o[2] <= hi[2]) return none;   // camera inside

    double uMin = INFINITY, uMax = -INFINITY, vMin = INFINITY, vMax = -INFINITY;
    for (int k = 0; k < 8; ++k) {
        const D3 corner{(k & 1) ? hi[0] : lo[0], (k & 2) ? hi[1] : lo[1], (k & 4) ? hi[2] : lo[2]};
        const D3 q = corner - origin;
        const double depth = dot(axis, q);
        if (!(depth > lens) || !(depth > 0.0)) return none;   // not strictly in front of the whole lens
        const D3 onPlane = origin + (planeDepth / depth) * q;   // where the pinhole ray to the corner crosses the focal plane
        const D3 rel = onPlane - lowerLeft;
        const double u = dot(rel, horizontal) / hh, v = dot(rel, vertical) / vv;
        if (!std::isfinite(u) || !std::isfinite(v)) return none;
        uMin = std::min(uMin, u), uMax = std::max(uMax, u);
        vMin = std::min(vMin, v), vMax = std::max(vMax, v);
    }
    const double uPad = lens / std::sqrt(hh), vPad = lens / std::sqrt(vv);
    // pixel coordinates: x = u width; y = (1 - v) height (cameraRay flips v)
    const double xLo = (uMin - uPad) * width, xHi = (uMax + uPad) * width;
    const double yLo = (1.0 - (vMax + vPad)) * height, yHi = (1.0 - (vMin - vPad)) * height;
    if (!std::isfinite(xLo) || !std::isfinite(xHi) || !std::isfinite(yLo) || !std::isfinite(yHi)) return none;
    // first and last pixel whose square touches the interval, then one whole pixel more on every side
    auto firstPixel = [](double at, uint32_t n) { return static_cast<uint32_t>(std::min(std::max(std::floor(at) - 1.0, 0.0), static_cast<double>(n))); };
    auto endPixel = [](double at, uint32_t n) { return static_cast<uint32_t>(std::min(std::max(std::floor(at) + 2.0, 0.0), static_cast<double>(n))); };
    CullRect r;
    r.x0 = firstPixel(xLo, width), r.x1 = endPixel(xHi, width);
    r.y0 = firstPixel(yLo, height), r.y1 = endPixel(yHi, height);
    if (r.x0 >= r.x1 || r.y0 >= r.y1) r.x0 = r.x1 = r.y0 = r.y1 = 0u;   // the scene lies off the image: every pixel is background
    if (r.x0 == 0u && r.y0 == 0u && r.x1 == width && r.y1 == height) return none;
    r.cull = true;
    return r;
}

}  // namespace ptr
