// What the hipcc-compiled host files share (hip_backend.cpp: scene upload and the render loop; debug_probes.cpp: the test-only entry
// points of include/ptr_debug.h; the update calls of dynamic_host.h): HIP error handling, device and pinned buffers, the device scene
// with the host-side records its upload fills, and the few backend functions the probes call.  Internal: not part of the C-ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <exception>
#include <functional>
#include <memory>
#include <string>
#include <vector>

#include "../kernels/device_types.h"
#include "../kernels/dynamic.h"
#include "../kernels/launch.h"
#include "appearance_host.h"
#include "background_cull.h"
#include "env_importance_sampler.h"
#include "geometry_cache.h"
#include "ptr_abi.h"

namespace ptrhost {

struct HipError {
    std::string message;
};

#define HIP_CHECK(expr)                                                                                     \
    do {                                                                                                    \
        hipError_t _e = (expr);                                                                             \
        if (_e != hipSuccess) {                                                                             \
            throw ptrhost::HipError{std::string(#expr) + ": " + hipGetErrorString(_e)};                     \
        }                                                                                                   \
    } while (0)

inline void setErr(char* err, size_t cap, const std::string& msg) {
    if (err && cap > 0) std::snprintf(err, cap, "%s", msg.c_str());
}

// Nothing may unwind across the C boundary: the BVH build allocates multi-GB vectors and starts threads
// (std::bad_alloc, std::system_error), and the callers are ctypes / a C++ program built with another runtime.
#define PTR_CATCH_ALL(err, cap)                                                                             \
    catch (const ptrhost::HipError& e) {                                                                    \
        ptrhost::setErr(err, cap, e.message);                                                               \
        return 1;                                                                                           \
    }                                                                                                       \
    catch (const std::exception& e) {                                                                       \
        ptrhost::setErr(err, cap, std::string("exception: ") + e.what());                                   \
        return 1;                                                                                           \
    }                                                                                                       \
    catch (...) {                                                                                           \
        ptrhost::setErr(err, cap, "unknown exception");                                                     \
        return 1;                                                                                           \
    }

template <typename T>
struct DeviceBuffer {
    T* ptr = nullptr;
    size_t count = 0;
    DeviceBuffer() = default;
    DeviceBuffer(const DeviceBuffer&) = delete;
    DeviceBuffer& operator=(const DeviceBuffer&) = delete;
    ~DeviceBuffer() { release(); }
    void release() {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        count = 0;
    }
    void ensure(size_t n) {
        if (n <= count && ptr) return;
        release();
        if (n == 0) n = 1;
        HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&ptr), n * sizeof(T)));
        count = n;
    }
    void upload(const T* src, size_t n) {
        ensure(n);
        if (n) HIP_CHECK(hipMemcpy(ptr, src, n * sizeof(T), hipMemcpyHostToDevice));
    }
    void download(T* dst, size_t n) const {   // blocking, like upload
        if (n) HIP_CHECK(hipMemcpy(dst, ptr, n * sizeof(T), hipMemcpyDeviceToHost));
    }
};

// A pinned host buffer, grown on demand and kept until its owner goes: what the update calls stage through.  flags: hipHostMalloc's.
struct PinnedBuffer {
    void* ptr = nullptr;
    size_t bytes = 0;
    unsigned flags = hipHostMallocDefault;
    explicit PinnedBuffer(unsigned f = hipHostMallocDefault) : flags(f) {}
    PinnedBuffer(const PinnedBuffer&) = delete;
    PinnedBuffer& operator=(const PinnedBuffer&) = delete;
    ~PinnedBuffer() {
        if (ptr) (void)hipHostFree(ptr);
    }
    void* pinnedFor(size_t n) {
        if (n > bytes) {
            if (ptr) (void)hipHostFree(ptr);
            ptr = nullptr, bytes = 0;
            HIP_CHECK(hipHostMalloc(&ptr, n, flags));
            bytes = n;
        }
        return ptr;
    }
};

inline float bitsToFloat(uint32_t u) {
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

}  // namespace ptrhost

#include "adaptive_state.h"   // AdaptiveStore, which needs DeviceBuffer and which PtrDeviceScene holds

using ptrhost::DeviceBuffer;

namespace ptrhost {

// Host side of PTR_DYNAMIC_PRIMITIVES (include/ptr_deform.h): where the rows of every rectangle and sphere live on the device, what does
// not change about them, and the records they currently hold.  Filled from a description and its preparation (dynamic.cpp).
struct PrimitiveRecords {
    std::vector<uint32_t> rectTriLeaf;   // 2 per rectangle: leaf-order indices of its triangles (0xFFFFFFFF: not in the geometry)
    std::vector<uint32_t> sphereLeaf;    // original sphere index -> leaf slot
    std::vector<uint32_t> rectShadeKey;  // per rectangle: the shade key in the meta word of its triangles
    std::vector<int32_t> lightIndexByRect;
    std::vector<float> rectEmission;     // 3 per rectangle (zeros for one that is no light)
    std::vector<PtrRect> rects;
    std::vector<PtrSphere> spheres;
    uint32_t triCount = 0;               // rows of the arrays, for the destinations' bounds
};

// What ptr_scene_rebuild_tree (include/ptr_rebuild.h) keeps, allocated at its first call: the second set of node arrays a rebuild
// builds into (swapped with the scene's on install) and the scratch of its steps.
struct RebuildState {
    DeviceBuffer<float4> boxes;
    DeviceBuffer<uint4> qnodes, wnodes;
    DeviceBuffer<uint32_t> schedule, wideSource;
    std::vector<uint32_t> levelOffsets;
    DeviceBuffer<uint32_t> leaves;                 // the leaf table on the device
    DeviceBuffer<uint64_t> keys, sortedKeys;
    DeviceBuffer<uint8_t> sortScratch;             // rocprim's, sized for the largest of the two sorts and the scan
    DeviceBuffer<uint32_t> first, parent, pre, iota, marks, wideIndex, small;   // small: level offsets (64 words), then reached (64 words)
    DeviceBuffer<uint2> kids;
    DeviceBuffer<uint8_t> heights, sortedHeights, depth;
    DeviceBuffer<double> partials;                 // k_tree_cost: the block sums of two trees
    hipEvent_t events[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    ~RebuildState() {
        for (hipEvent_t e : events) {
            if (e) (void)hipEventDestroy(e);
        }
    }
};

// What a dynamic scene (include/ptr_dynamic.h) keeps beside the arrays the kernels render from: ptr::DynamicTables on the device, the
// float child boxes of every node, and the figures ptr_scene_set_mesh_transforms reports.  A static scene has none of it.
struct DynamicScene {
    DeviceBuffer<float4> objPos, objNrm, objTan;   // object-space corners, 3 float4 per triangle, leaf order
    DeviceBuffer<float4> triBounds, sphereBounds;  // 2 float4 per primitive, leaf order
    DeviceBuffer<float4> boxes;                    // quantised scenes: the 64 B float nodes (a float scene refits ds.nodes itself)
    DeviceBuffer<uint32_t> meshTris, schedule, wideSource;
    DeviceBuffer<float4> meshTable;                // kDynMeshVec4 float4 per named mesh of a call
    std::vector<uint32_t> meshTriOffsets, levelOffsets;
    std::vector<uint8_t> meshHasTangents;
    uint32_t nodeCount = 0, wideCount = 0, triCount = 0, sphereCount = 0;
    bool textured = false;
    float meanPrimExtent = 0.0f;
    hipEvent_t events[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    float4* rootBox = nullptr;   // pinned: node 0 after a refit
    // the matrix every mesh currently has, as the bake reads it: from the description at upload, then from ptr_scene_set_mesh_transforms
    std::vector<ptrk::DynMeshRow> meshRows;
    // include/ptr_deform.h.  flags: what the upload kept (PTR_DYNAMIC_*).
    uint32_t flags = 0;
    // PTR_DYNAMIC_DEFORMABLE: the corner table (3 vertex indices per entry of meshTris) and what validates a call
    DeviceBuffer<uint32_t> meshCorners;
    std::vector<uint32_t> meshVertexCount;
    std::vector<uint8_t> meshTangentsGiven;
    // PTR_DYNAMIC_VERTEX_NORMALS (include/ptr_deform_device.h): the vertex adjacency of every mesh (ptr::DynamicTables::adjOffsets /
    // adjEntries / adjBase), uploaded once; the normals k_dyn_vertex_normals computes in a call; the flag words of k_dyn_check_finite
    DeviceBuffer<uint32_t> adjOffsets, adjEntries;
    std::vector<uint64_t> adjBase;
    DeviceBuffer<float> computedNormals;
    DeviceBuffer<uint32_t> checkFlags;
    // PTR_DYNAMIC_PRIMITIVES: where the rows of a rectangle and of a sphere live, and the records they currently hold
    PrimitiveRecords prims;
    // include/ptr_rebuild.h: the leaf table of the upload's tree (host; it goes to the device at the first rebuild) and what the first
    // ptr_scene_tree_cost / ptr_scene_rebuild_tree allocates
    std::vector<uint32_t> leafTable;
    std::unique_ptr<RebuildState> rebuild;
    // staging of the update calls, grown on demand and kept: a pinned host buffer and its device twin
    DeviceBuffer<float4> staging;
    PinnedBuffer pinned;
    ~DynamicScene() {
        for (hipEvent_t e : events) {
            if (e) (void)hipEventDestroy(e);
        }
        if (rootBox) (void)hipHostFree(rootBox);
    }
};

// The host-side records of a scene's appearance, the ones the check halves of include/ptr_appearance.h read: filled by uploadScene from
// the preparation and the description (fillAppearanceRecords, no device call), changed by an accepted call; empty without an upload.
struct AppearanceRecords {
    std::vector<float> materialRows;       // the compact rows of ds.materials
    std::vector<uint32_t> rectMaterial;    // per rectangle: its material index as the description gave it
    std::vector<uint32_t> texInfo;         // the records of ds.texInfo
};

// The scratch of the appearance calls' kernels (appearance.cpp), made at the first of them.
struct AppearanceState {
    DeviceBuffer<uint8_t> keys;            // k_app_rekey's table
    DeviceBuffer<uint32_t> words;          // [0] rows rekeyed, [1..] flag words of the finiteness check
    DeviceBuffer<float4> checkRows;
    DeviceBuffer<float> envWeight, envRowWeight, envCell, envTotal;
    hipEvent_t events[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    PinnedBuffer pinned, staged;           // the rows and landing places a run lays out (small); the host pixels of a textures or environment call
    ~AppearanceState() {
        for (hipEvent_t e : events) {
            if (e) (void)hipEventDestroy(e);
        }
    }
};

}  // namespace ptrhost

struct PtrDeviceScene {
    int device = 0;
    DeviceBuffer<uint4> qnodes;
    DeviceBuffer<uint4> wnodes;   // PTR_WIDE_NODES=1: four-wide nodes (SceneView::wnodes)
    DeviceBuffer<float4> nodes, tris, triNormals, spheres, materials, rects, rectLights, envRgba;
    DeviceBuffer<uint2> sphereInfo;
    DeviceBuffer<int32_t> lightIndexByRect;
    DeviceBuffer<float2> envCond, envMarg, cone;
    DeviceBuffer<float4> triUv, triTangent, texels, materialTex;
    DeviceBuffer<uint4> texInfo;
    DeviceBuffer<float> envPdf;
    // PTR_METAL_ENV_LOD: the environment map's mip chain (EnvLodView::mips), built on the first render that sets the bit
    DeviceBuffer<float4> envMips;
    uint32_t envMipLevels = 0;   // 0: not built
    ptrk::SceneView view{};
    std::unique_ptr<ptrhost::DynamicScene> dynamic;   // ptr_scene_upload_dynamic only
    ptrhost::AppearanceRecords appearanceRecords;           // include/ptr_appearance.h: what the scene holds, from its upload
    std::unique_ptr<ptrhost::AppearanceState> appearance;   // ... and the kernels' scratch, made by the first call
    uint64_t info[8] = {0};
    double uploadSeconds = 0.0;
    double timings[4] = {0.0, 0.0, 0.0, 0.0};   // geometry preparation (or cache read), shading tables, copies to the device, 1 = geometry came from a cache
    uint64_t deviceTotalBytes = 0;        // hipDeviceProp_t::totalGlobalMem
    bool hasRandomWalkMaterial = false;   // a type-5 material with sssParams.y >= 0.5 (Metal random-walk subsurface)

    // render-time resources, grown on demand and kept across calls
    DeviceBuffer<float4> state, recBuf, itemAccum;   // state: the four 16 B words of every slot (PathPool::ray0 / ray1 / thr / accum)
    DeviceBuffer<float2> hit;
    DeviceBuffer<uint32_t> flushItem, signature, tailList, tailWords;
    DeviceBuffer<uint32_t> connectList, connectCounts;   // PathPool::connectList: per group a list and two sets of sub-list counters
    DeviceBuffer<uint32_t> busyLists, busyCounts;        // PathPool::busyIn / busyOut: per group two lists and three sets of counters
    // end of the frame: once the item queue is dry and at most this many slots are still alive, the remaining paths are finished by
    // k_tail_run (one lane per path, no launches between bounces) instead of further extend / shade / connect rounds; 0 = never
    uint64_t tailBelow = 512ull << 10;
    uint64_t poolSlots = 32ull << 20;        // resident path slots at most (PTR_POOL_SLOTS)
    // The pool is split into this many independent groups.  Two by default, each on a main stream (k_extend, k_shade) and a side stream
    // on which the k_connect of an iteration runs beside the k_extend of the next (they share nothing: one reads the rays k_shade wrote,
    // the other its connection records): four streams in flight, which is what the runtime's four hardware queues carry without
    // serialising.  (Rounds 1-3 ran four groups of one stream each; profiles/r3_ab_connect_overlap.txt.)
    // Frames of a few milliseconds (a pool of at most 8 Mi slots: config 1) keep four groups of one stream each: -6 % with two.
    uint32_t poolGroups = 0;      // PTR_POOL_GROUPS (0: two groups, four for small pools)
    bool connectOverlap = true;   // PTR_CONNECT_OVERLAP=0: k_connect on the group's own stream
    uint32_t maxPoolGroups() const { return poolGroups ? poolGroups : 4u; }
    uint32_t feederChunk = 256;   // slots per work-head claim while the pool is full (it grows as the pool drains)
    std::vector<hipStream_t> groupStreams;   // streams of groups 1.. (group 0 runs on the caller's stream)
    std::vector<hipEvent_t> groupEvents;
    std::vector<hipStream_t> sideStreams;    // per group: the stream of its k_connect launches (see poolGroups)
    std::vector<hipEvent_t> sideEvents;      // per group: k_shade of the iteration done / k_connect of the iteration done
    int refillBelow = 40;
    uint32_t spillLevels = 0;   // stack levels beyond the LDS part that the scene's tree can need (sizes the spill area)
    uint32_t wideDepth = 0;     // levels of the four-wide tree (0: the scene has no four-wide nodes)
    DeviceBuffer<uint4> medium;
    DeviceBuffer<float> envLod;   // PTR_METAL_ENV_LOD: EnvLodView::slotLod
    DeviceBuffer<uint32_t> scalars, pixelOfLocal, spill;
    DeviceBuffer<uint2> itemReserve;
    DeviceBuffer<uint32_t> itemHeads, zeros;
    DeviceBuffer<uint64_t> counters;
    DeviceBuffer<float> outBands;
    DeviceBuffer<float> covBands;    // ptr_render_bands_cov: the covariance beside outBands (include/ptr_stats.h)
    DeviceBuffer<float4> covMean;    // k_resolve_cov: per local pixel, the running mean between the passes of a frame
    ptrhost::AdaptiveStore adaptive;   // adaptive frames (include/ptr_adaptive.h): the per-pixel state, the two active lists, the scratch
    DeviceBuffer<float> adaptiveOut;   // ptr_render_adaptive: rgb, cov and count of the frame before they go to the host
    DeviceBuffer<float4> rayBatch;
    DeviceBuffer<PtrHit> hitBatch;
    uint32_t* pinnedAlive = nullptr;
    uint32_t traceGrid = 0;       // persistent blocks of the traversal kernels: fills every wave slot (also sizes the spill area)
    uint32_t traceGridHalf = 0;   // ... of k_extend / k_connect when several pool groups run large launches side by side
    // cached partition: pixelOfLocal holds the pixels renderPass traces, backgroundPixels the ones cachedCull keeps out of the pool
    uint32_t cachedW = 0, cachedH = 0, cachedPart = 0, cachedParts = 0, cachedLocalPixels = 0, cachedBackgroundPixels = 0;
    ptr::CullRect cachedCull;
    DeviceBuffer<uint32_t> backgroundPixels;
    // world box of everything a ray can hit (csrc/host/background_cull.h): from the primitives at upload, from the refitted root box
    // after an update call of ptr_dynamic.h / ptr_deform.h (invalid there when the scene keeps triangles out of the tree: nothing is culled then)
    ptr::WorldBounds worldBounds;

    ~PtrDeviceScene() {
        if (pinnedAlive) (void)hipHostFree(pinnedAlive);
        for (hipStream_t st : groupStreams) (void)hipStreamDestroy(st);
        for (hipEvent_t e : groupEvents) (void)hipEventDestroy(e);
        for (hipStream_t st : sideStreams) (void)hipStreamDestroy(st);
        for (hipEvent_t e : sideEvents) (void)hipEventDestroy(e);
    }
};

namespace ptrhost {

// Defined in hip_backend.cpp.
void compactMaterial(const PtrMaterial& m, std::vector<float>& out);
void materialTexRow(const PtrMaterial& m, float* out);   // kMaterialTexVec4 float4
void appendTextureWithMips(const PtrTexture& t, std::vector<float>& texels, std::vector<uint32_t>& info);
double ensureEnvMips(PtrDeviceScene& ds);
void fillRenderParams(const PtrSettings& s, uint32_t spp, ptrk::RenderParams& rp);
ptrk::LaunchConfig coldLaunchConfig(const PtrDeviceScene& ds);
// What renderPass does with a plain frame's pixels (csrc/host/background_cull.h): the rectangle of the pixels it traces, or no culling
// (the knob, a covariance frame, the counting build or mode bit 2, maxDepth 0, unknown bounds) for a scene of world box `world`.  Host only.
ptr::CullRect passCullRect(const ptr::WorldBounds& world, const PtrSettings& settings, bool covariance, int mode);
// dCov (nullable): the covariance of the pixel mean beside the image (include/ptr_stats.h), six floats per pixel in dOut's band layout
// mode: bit 0 the counting build, bit 1 the pool as one group (solo), bit 2 every pixel through the pool (no background cull)
void renderBands(PtrDeviceScene& ds, const PtrSettings& settings, uint32_t spp, uint32_t part, uint32_t parts, float* dOut, hipStream_t stream,
                 int mode, PtrRenderStats* stats, float* dCov = nullptr);
// passes renderBands splits a frame of `spp` samples per pixel into (the per-sample accumulators of a pass have to fit in memory)
uint32_t framePasses(const PtrDeviceScene& ds, const PtrSettings& settings, uint32_t spp);

// most per-sample accumulators one pass may hold (the scene's memory budget, or the 32-bit cap without a scene; PTR_MAX_ITEMS)
uint64_t maxPassItems(const PtrDeviceScene* ds);
// The tracing part of a pass, for a caller that brings its own local-pixel table (include/ptr_adaptive.h): samples sampleBase ..
// sampleBase + spp - 1 of the `localPixels` (> 0) pixels dPixelOfLocal names, non-counting kernels.  `consume` is handed the pass's
// accumulators - sample c of local pixel lp at [c * localPixels + lp] - and launches what reads them on `stream`; the stream is joined
// before the call returns.  Uses ds.outBands as scratch; leaves the scene's cached partition table alone.
// `mode` as renderBands takes it (0 in every render); `hook` (null in every render): what the stepping probe (include/ptr_debug_path.h)
// runs after the launches of each iteration, with the iteration's index and the whole pool; it joins the device itself.
using IterationHook = std::function<void(uint64_t, const ptrk::PathPool&)>;
void traceItems(PtrDeviceScene& ds, const PtrSettings& settings, uint32_t spp, uint32_t sampleBase, const uint32_t* dPixelOfLocal,
                uint32_t localPixels, hipStream_t stream, PtrRenderStats* stats, const std::function<void(const float4*)>& consume,
                int mode = 0, const IterationHook* hook = nullptr);
// The first-hit feature buffers of sample `sample` of the whole image, through the two device buffers (grown on demand) into the host
// arrays that are not null.  The scene's device is current; blocking.
void downloadFirstHit(PtrDeviceScene& ds, const PtrSettings& settings, uint32_t sample, DeviceBuffer<float4>& albedo, DeviceBuffer<float4>& normal,
                      float* outAlbedo, float* outNormal);
// the local-pixel order of a one-partition frame (8-row bands, 8x8 blocks)
void imagePixelOrder(uint32_t width, uint32_t height, std::vector<uint32_t>& out);
// adds the times, launches and samples of pass `one` to `sum`
void addPassStats(const PtrRenderStats& one, PtrRenderStats& sum);
// adds the per-launch figures of `b` to `a` (kernel times, k_extend launches, samples), as a frame on several devices sums its partitions
void addLaunchStats(PtrRenderStats& a, const PtrRenderStats& b);

// What the frames on several devices (multi.cpp) share with the single-device ones here.
// the local-pixel order of partition `part` of `parts`: its bands top to bottom, each in 8x8 blocks
void partitionPixels(uint32_t width, uint32_t height, uint32_t part, uint32_t parts, std::vector<uint32_t>& out);
// Device-independent half of a scene upload: geometry bake + BVH, compact materials, light list, environment tables.  Built once
// and uploaded to every device a frame is rendered on.
struct PreparedScene {
    ptr::PreparedGeometry pg;   // BVH, leaf-order arrays, four-wide nodes, node format: what a geometry cache file holds
    std::vector<float> mats;
    ptr::RectLightTable rectLights;    // (lightsHaveTriangles: every light found its two triangles in the geometry - always, unless degenerate)
    bool hasRandomWalkMaterial = false;
    ptr::EnvImportanceDistribution envDist;
    bool hasEnvDist = false;
    // material textures (kernels/texture.h): every level of every texture in one array, the per-texture records, and the
    // per-material texture records; empty when the scene has no textures
    std::vector<float> texels;
    std::vector<uint32_t> texInfo;
    std::vector<float> materialTex;
    double geometrySeconds = 0.0;   // bake + BVH + leaf order + wide nodes, or reading them from a geometry cache
    double shadingSeconds = 0.0;    // materials, lights, environment tables, texture mips
    bool geometryFromCache = false;
    double seconds = 0.0;           // both
    bool dynamic = false;           // ptr_scene_upload_dynamic: `dyn` is filled and uploadScene makes the scene dynamic
    ptr::DynamicTables dyn;
};
// The geometry half of the preparation: bake, BVH, node format (the PTR_QUANTIZED_NODES / PTR_WIDE_NODES knobs), four-wide nodes.
// dyn (nullable): the tables of a dynamic scene as well.
void prepareGeometry(const PtrSceneDesc& desc, ptr::PreparedGeometry& pg, ptr::DynamicTables* dyn = nullptr);
// cachePath (may be null): read the geometry from that file instead of building it; dynamic: prepare a dynamic scene (no cache)
// dynamicFlags: PTR_DYNAMIC_* of include/ptr_deform.h, what a dynamic scene keeps beyond ptr_scene_upload_dynamic
void prepareScene(const PtrSceneDesc& desc, PreparedScene& ps, const char* cachePath = nullptr, bool dynamic = false, uint32_t dynamicFlags = 0);
// ds.device names the device
void uploadScene(const PtrSceneDesc& desc, const PreparedScene& ps, PtrDeviceScene& ds);
// the dynamic half of uploadScene (dynamic.cpp): ps.dyn and the float nodes to the device, ds.dynamic made
void uploadDynamicTables(const PtrSceneDesc& desc, const PreparedScene& ps, PtrDeviceScene& ds);
// the root box of the tree from node 0 (dynamic.cpp): the union of its children that exist
bool rootBoxOf(const float4 row[4], float lo[3], float hi[3]);
// the rectangle-light table of `desc` over the geometry `geo`, for a caller without the compact material rows (prepareScene has them):
// ptr::DeriveRectLights on rows made here
ptr::RectLightTable rectLightsOf(const PtrSceneDesc& desc, const ptr::SceneGeometry& geo);

// What an entry point refuses before any device call: returns the C-ABI's code with the message in `err`.
inline int refuse(char* err, size_t cap, const std::string& message) {
    setErr(err, cap, message);
    return 1;
}
inline int nullArgument(const char* who, char* err, size_t cap) { return refuse(err, cap, std::string(who) + ": null argument"); }
inline int noDevice(const char* who, char* err, size_t cap) {
    setErr(err, cap, std::string(who) + ": no HIP device (the HIP path has no CPU fallback)");
    return 2;
}
// The tail of the array probes (ptr_debug_scene_arrays, ptr_debug_rebuild_arrays, ptr_debug_appearance_arrays) once the selector has named
// `bytes` at `src`, on the host or in `device`'s memory: the size written, the capacity tested, the copy.  0, 2 (too small), 3 (failed copy).
inline int probeArrayTail(int device, const void* src, bool host, uint64_t bytes, void* out, uint64_t cap_bytes, uint64_t* size_out) {
    *size_out = bytes;
    if (!out || bytes == 0u) return 0;
    if (cap_bytes < bytes) return 2;
    if (host) {
        std::memcpy(out, src, bytes);
        return 0;
    }
    if (hipSetDevice(device) != hipSuccess || hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost) != hipSuccess) return 3;
    return 0;
}
// Pixels, list entries and per-sample accumulators are 32-bit indices with room for a block of threads past the last one.
constexpr uint64_t kIndexLimit = 0xFFFF0000ull;
inline bool pastIndexLimit(uint64_t count) { return count > kIndexLimit; }

// The frame of a C-ABI entry point that works on a device: "<who>: null argument" unless argsOk (a call that needs `scene` says so
// there), the device selected (the scene's; device 0 for a call without a scene, which fails when there is none), the body, the error
// a launch in it may have left, and nothing unwinding to the caller.
template <typename Body>
int deviceCall(const char* who, const PtrDeviceScene* scene, bool argsOk, char* err, size_t cap, Body&& body) {
    if (!argsOk) return nullArgument(who, err, cap);
    try {
        if (!scene && ptr_device_count() < 1) throw HipError{"no HIP device (the HIP path has no CPU fallback)"};
        HIP_CHECK(hipSetDevice(scene ? scene->device : 0));
        body();
        HIP_CHECK(hipGetLastError());
        return 0;
    }
    PTR_CATCH_ALL(err, cap)
}

}  // namespace ptrhost
