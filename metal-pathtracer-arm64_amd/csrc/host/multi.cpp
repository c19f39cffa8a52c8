// Every frame on several devices: ptr_render_multi (include/ptr_abi.h) with its test-only variant of include/ptr_debug.h, and the frames of
// include/ptr_multi.h that carry a covariance or are sampled adaptively.  The argument checks, the scene prepared once, one host thread
// per partition (each with its own device scene and stream), the lock-step rounds of an adaptive frame with the exchange of the band-edge
// rows of e between them, the hand-over of the band-layout buffers to the first device, which interleaves them into the image.  The
// sample source of a pass is a parameter of the partition loop: the traced one for the renderer, the gathered one for the test-only probe,
// which therefore runs everything else the renderer runs.  The state's buffers, the sources and the sample step are the ones adaptive.cpp
// and the resumable frames use (adaptive_host.h); the halo goes out from the step's hook.  The device list of a call, the exchange's
// pinned memory with its publish and collect halves, the hand-over to the first device and the gather there are stated once, below, for
// this driver and for the resumable frame of multi_frame.cpp (multi_host.h, which also holds the thread-per-partition driver of both).
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../kernels/multi.h"
#include "adaptive_host.h"
#include "device_scene.h"
#include "knobs.h"
#include "multi_host.h"
#include "ptr_debug.h"
#include "ptr_multi.h"

using namespace ptrhost;
using namespace ptrk;

// ---- what multi_host.h declares for both drivers ----
namespace ptrhost {

std::string badDeviceRequest(const std::string& w, bool listed, int n) {
    if (listed && (n < 1 || n > PTR_MULTI_MAX_PARTS)) return w + ": the id list must name 1 .. " + std::to_string(PTR_MULTI_MAX_PARTS) + " devices";
    if (!listed && n > PTR_MULTI_MAX_PARTS) return w + ": at most " + std::to_string(PTR_MULTI_MAX_PARTS) + " devices";
    return std::string();
}

int pickDevices(const char* who, const int* ids, int n, bool listed, uint32_t height, std::vector<int>& devices, std::vector<char>& forceStaged,
                char* err, size_t cap) {
    const std::string w(who);
    const int available = ptr_device_count();
    if (available < 1) return noDevice(who, err, cap);
    if (listed) {   // (an id given as -(id + 1) sends that partition's bands through pinned host memory: the tests' hook)
        for (int i = 0; i < n; ++i) {
            const int id = ids[i] < 0 ? -(ids[i] + 1) : ids[i];
            if (id < 0 || id >= available) return refuse(err, cap, w + ": no such HIP device");
            devices.push_back(id);
            forceStaged.push_back(ids[i] < 0 ? 1 : 0);
        }
        return 0;
    }
    int count = n <= 0 ? available : n;
    if (count > available) {
        setErr(err, cap, w + ": " + std::to_string(count) + " devices requested, " + std::to_string(available) + " visible");
        return 2;
    }
    count = std::min(count, PTR_MULTI_MAX_PARTS);
    // never more partitions than bands
    count = static_cast<int>(std::min<uint32_t>(static_cast<uint32_t>(count), std::max(1u, (height + PTR_BAND_ROWS - 1u) / PTR_BAND_ROWS)));
    for (int i = 0; i < count; ++i) devices.push_back(i);
    forceStaged.assign(static_cast<size_t>(count), 0);
    return 0;
}

void HaloExchange::allocate(const std::vector<uint32_t>& partBands, uint32_t width) {
    const uint32_t parts = static_cast<uint32_t>(partBands.size());
    offset.assign(parts + 1u, 0u);
    for (uint32_t p = 0; p < parts; ++p) offset[p + 1u] = offset[p] + static_cast<size_t>(partBands[p]) * 2u * width;
    const size_t bytes = offset.back() * 2u * sizeof(float);
    HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&host), std::max<size_t>(bytes, sizeof(float)), hipHostMallocPortable));
    std::memset(host, 0, bytes);
}

void HaloExchange::publishZeros() {
    if (host) std::memset(host, 0, offset.back() * sizeof(float));
}

void haloPublish(const MultiPart& mp, const float* dE, float* dEdge, const HaloExchange& ex, hipStream_t stream, hipEvent_t before, hipEvent_t after) {
    if (before) HIP_CHECK(hipEventRecord(before, stream));
    launchMultiHaloPack(mp, dE, dEdge, stream);
    HIP_CHECK(hipMemcpyAsync(ex.outbox(mp.part), dEdge, ex.haloBytes(mp.part), hipMemcpyDeviceToHost, stream));
    if (after) HIP_CHECK(hipEventRecord(after, stream));
}

void haloCollect(const MultiPart& mp, float* dEdge, float* dE, const HaloExchange& ex, hipStream_t stream, hipEvent_t before, hipEvent_t after) {
    multiCollectNeighbourRows(mp, ex.host, ex.offset.data(), ex.inbox(mp.part));
    if (before) HIP_CHECK(hipEventRecord(before, stream));
    HIP_CHECK(hipMemcpyAsync(dEdge, ex.inbox(mp.part), ex.haloBytes(mp.part), hipMemcpyHostToDevice, stream));
    launchMultiHaloUnpack(mp, dEdge, dE, stream);
    if (after) HIP_CHECK(hipEventRecord(after, stream));
}

// A partition's band buffer travels to the first device of the frame (multi_host.h).
bool sendBandsToRoot(void* dRootDst, int rootDevice, const void* dSrc, int device, size_t bytes, bool forceStaged, hipStream_t stream) {
    if (device == rootDevice && !forceStaged) {
        HIP_CHECK(hipMemcpyAsync(dRootDst, dSrc, bytes, hipMemcpyDeviceToDevice, stream));
        return false;
    }
    int direct = 0;
    if (device != rootDevice) HIP_CHECK(hipDeviceCanAccessPeer(&direct, device, rootDevice));
    if (forceStaged) direct = 0;
    if (direct) {
        const hipError_t enabled = hipDeviceEnablePeerAccess(rootDevice, 0);   // (this thread's current device is `device`)
        if (enabled != hipSuccess && enabled != hipErrorPeerAccessAlreadyEnabled) direct = 0;
        (void)hipGetLastError();
    }
    if (direct) {
        HIP_CHECK(hipMemcpyPeerAsync(dRootDst, rootDevice, dSrc, device, bytes, stream));
        return false;
    }
    std::fprintf(stderr, "[ptr] device %d does not address device %d directly: its bands go through pinned host memory\n", device, rootDevice);
    void* staging = nullptr;
    HIP_CHECK(hipHostMalloc(&staging, bytes, hipHostMallocDefault));
    hipError_t copied = hipMemcpyAsync(staging, dSrc, bytes, hipMemcpyDeviceToHost, stream);
    if (copied == hipSuccess) copied = hipStreamSynchronize(stream);
    if (copied == hipSuccess) copied = hipSetDevice(rootDevice);
    if (copied == hipSuccess) copied = hipMemcpy(dRootDst, staging, bytes, hipMemcpyHostToDevice);
    (void)hipSetDevice(device);
    (void)hipHostFree(staging);
    HIP_CHECK(copied);
    return true;
}

void BandGather::allocate(const std::vector<uint32_t>& partBands, uint32_t imageWidth, uint32_t imageHeight, uint32_t covAt, uint32_t countAt, uint32_t words) {
    parts = static_cast<uint32_t>(partBands.size()), width = imageWidth, height = imageHeight, pixelWords = words;
    partPixel.assign(parts + 1u, 0u);
    wordOffset.assign(static_cast<size_t>(parts) * 3u, 0u);
    for (uint32_t p = 0; p < parts; ++p) {
        const uint64_t start = partPixel[p] * pixelWords, mine = static_cast<uint64_t>(partBands[p]) * PTR_BAND_ROWS * width;
        partPixel[p + 1u] = partPixel[p] + mine;
        wordOffset[p] = start;
        wordOffset[parts + p] = start + mine * covAt;
        wordOffset[2u * parts + p] = start + mine * countAt;
    }
    gathered.ensure(static_cast<size_t>(partPixel[parts]) * pixelWords);
    dWordOffset.upload(wordOffset.data(), wordOffset.size());
}

void BandGather::interleave(float* dRgb, float* dCov, void* dCount, hipStream_t stream) const {
    launchMultiInterleave(gathered.ptr, dWordOffset.ptr, parts, width, height, 3u, dRgb, stream);
    if (dCov) launchMultiInterleave(gathered.ptr, dWordOffset.ptr + parts, parts, width, height, 6u, dCov, stream);
    if (dCount) launchMultiInterleave(gathered.ptr, dWordOffset.ptr + 2u * parts, parts, width, height, 1u, dCount, stream);
    HIP_CHECK(hipGetLastError());
}

}  // namespace ptrhost

namespace {

// What one call asks for.  The kind says which pointers it needs and what it reports; everything else runFrame reads off the outputs asked for.
enum class Kind { Plain, Covariance, Adaptive, Probe };   // ptr_render_multi; ..._cov; ..._adaptive; the test-only probe, which has no scene
struct Request {
    const char* who = "";
    Kind kind = Kind::Plain;
    const PtrSceneDesc* scene = nullptr;
    const PtrSettings* settings = nullptr;   // the probe fills in width and height only
    uint32_t spp = 0u;
    const PtrAdaptiveParams* params = nullptr;
    const float* samples = nullptr;
    // the devices asked for: the n that `ids` lists (the debug variants), or the first n (n <= 0: all there are)
    const int* ids = nullptr;
    int n = 0;
    bool listed = false;
    int verbose = 0;
    float* outRgb = nullptr;
    float* outCov = nullptr;
    uint32_t* outCount = nullptr;
    float* outAlbedo = nullptr;
    float* outNormal = nullptr;
    PtrRenderStats* stats = nullptr;
    PtrAdaptiveInfo* info = nullptr;
    PtrMultiInfo* multi = nullptr;
    std::vector<int> devices;   // admit fills these two in
    std::vector<char> forceStaged;
};

void runFrame(const Request& rq) {
    const bool probe = rq.kind == Kind::Probe, adaptive = probe || rq.kind == Kind::Adaptive;
    const PtrSettings& settings = *rq.settings;
    const uint32_t parts = static_cast<uint32_t>(rq.devices.size());
    const uint32_t width = settings.width, height = settings.height;
    const size_t pixels = static_cast<size_t>(width) * height;
    if (pastIndexLimit(pixels + static_cast<size_t>(PTR_BAND_ROWS) * width)) throw HipError{"image too large"};
    const auto t0 = Clock::now();
    PreparedScene prepared;
    if (!probe) prepareScene(*rq.scene, prepared);

    std::vector<uint32_t> partBands(parts, 0u);
    for (uint32_t p = 0; p < parts; ++p) partBands[p] = ptr_part_band_count(height, p, parts);
    const int rootDevice = rq.devices[0];
    const bool wantCov = rq.outCov != nullptr, wantCount = adaptive && rq.outCount != nullptr;
    // a partition's band buffer holds cov and count only where they are asked for; on the first device the gather and the image-order outputs
    const uint32_t covAt = 3u, countAt = wantCov ? 9u : 3u, pixelWords = countAt + (wantCount ? 1u : 0u);
    BandGather bands;
    DeviceBuffer<float> image;
    HIP_CHECK(hipSetDevice(rootDevice));
    bands.allocate(partBands, width, height, covAt, countAt, pixelWords);
    image.ensure(pixels * pixelWords);

    HaloExchange ex;
    if (adaptive && parts > 1u) ex.allocate(partBands, width);

    std::vector<std::unique_ptr<PtrDeviceScene>> scenes(parts);
    std::vector<PtrRenderStats> partStats(parts);
    std::vector<hipStream_t> streams(parts, nullptr);   // per call: made by a partition's thread and destroyed by it
    std::vector<double> uploadSeconds(parts, 0.0), stateSeconds(parts, 0.0), renderSeconds(parts, 0.0), workerSeconds(parts, 0.0), waitSeconds(parts, 0.0);
    std::vector<uint64_t> partSamples(parts, 0u);
    std::vector<uint32_t> partAtMax(parts, 0u), published(parts, 0u);
    std::atomic<uint32_t> stagedParts{0};
    PtrAdaptiveInfo info{};   // written by partition 0's thread (every thread computes the same figures)
    uint32_t sharedCount = 0u;
    const double setupSeconds = since(t0) - prepared.seconds;   // the first device's buffers and the exchange memory

    auto body = [&](uint32_t p, const auto& meet) {
        hipStream_t& stream = streams[p];
        const auto w0 = Clock::now();
        auto ds = std::make_unique<PtrDeviceScene>();
        ds->device = rq.devices[p];
        if (!probe) uploadScene(*rq.scene, prepared, *ds);
        uploadSeconds[p] = since(w0);
        HIP_CHECK(hipSetDevice(ds->device));
        HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        const MultiPart mp{p, parts, partBands[p], width, height};
        const size_t myBandPixels = bands.bandPixels(p);
        ds->adaptiveOut.ensure(myBandPixels * pixelWords);   // the partition's rgb, cov and count in band layout
        float* const dRgb = ds->adaptiveOut.ptr;
        float* const dCov = wantCov ? dRgb + myBandPixels * covAt : nullptr;
        uint32_t* const dCount = wantCount ? reinterpret_cast<uint32_t*>(dRgb + myBandPixels * countAt) : nullptr;

        auto handOver = [&] {   // the band buffer travels to the first device in one piece
            if (myBandPixels && sendBandsToRoot(bands.slot(p), rootDevice, dRgb, ds->device, bands.bandBytes(p), rq.forceStaged[p] != 0, stream)) {
                stagedParts.fetch_add(1);
            }
            HIP_CHECK(hipStreamSynchronize(stream));
        };

        if (!adaptive) {
            const auto r0 = Clock::now();
            if (myBandPixels) renderBands(*ds, settings, rq.spp, p, parts, dRgb, stream, 0, &partStats[p], dCov);
            partSamples[p] = partStats[p].samples;   // the partition's pixels, as renderPass counted them, times spp
            handOver();
            renderSeconds[p] = since(r0);
            scenes[p] = std::move(ds);
            return;
        }

        const PtrAdaptiveParams& params = *rq.params;
        std::vector<uint32_t> order;
        partitionPixels(width, height, p, parts, order);
        const uint32_t local = static_cast<uint32_t>(order.size());
        AdaptiveStore& b = ds->adaptive;
        b.ensure(pixels);   // image order: the lists name image pixels, select reads e around them
        DeviceBuffer<float> edge;
        edge.ensure(static_cast<size_t>(mp.bands) * 2u * width);
        PtrRenderStats sum{};
        SampleStep step{nullptr, maxPassItems(ds.get()), b.state(), stream, rq.stats ? &sum : nullptr};
        DeviceBuffer<float4> probeSamples, probeItems;
        if (probe) {
            probeSamples.upload(reinterpret_cast<const float4*>(rq.samples), static_cast<size_t>(params.maxSpp) * pixels);
            // the largest sub-pass of the frame: the source then frees nothing in the middle of it
            const uint64_t mostSpp = std::max(params.minSpp, std::min(params.stepSpp, params.maxSpp));
            probeItems.ensure(static_cast<size_t>(std::max<uint64_t>(local, std::min<uint64_t>(step.maxItems, static_cast<uint64_t>(local) * mostSpp))));
            step.source = gatheredSource(probeSamples.ptr, pixels, params.maxSpp, probeItems, stream);
        } else {
            step.source = tracedSource(*ds, settings, stream);
        }
        if (local) HIP_CHECK(hipMemcpyAsync(b.list(0u), order.data(), local * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
        b.zero(stream);
        HIP_CHECK(hipStreamSynchronize(stream));   // `order` is pageable host memory
        stateSeconds[p] = since(w0) - uploadSeconds[p];

        const auto r0 = Clock::now();
        uint32_t active = local, n = 0u, turn = 0u, rounds = 0u;
        // PTR_VERBOSE=launches: device events around the two halves of the exchange (tools/multi_adaptive_cost.py parses the line)
        EventSet marks;
        const bool timed = parts > 1u && ptr::readKnobs().verboseLaunches;
        if (timed) marks.create(4u);
        const size_t haloBytes = static_cast<size_t>(mp.bands) * 2u * width * sizeof(float);
        for (bool more = true; more;) {
            const uint32_t roundSpp = adaptiveRoundSpp(params, n);
            const uint32_t* list = b.list(turn);
            // 1. trace and update; behind the last update the edge rows of e go to the outbox
            if (active > 0u) {
                addSamples(step, list, active, n, roundSpp, [&](uint32_t, uint32_t, bool last) {
                    if (!last || parts == 1u) return;
                    haloPublish(mp, step.state.e, edge.ptr, ex, stream, marks[0], marks[1]);
                });
                HIP_CHECK(hipStreamSynchronize(stream));   // (the source joined the stream already: the outbox is written)
                partSamples[p] += static_cast<uint64_t>(active) * roundSpp;
            }
            n += roundSpp;
            if (n >= params.maxSpp) partAtMax[p] = active;
            // 2. every partition has published
            if (!meet()) return;
            // 3. the neighbours' rows, select and compact on the own list, the own total
            if (active > 0u) {
                if (parts > 1u) {
                    haloCollect(mp, edge.ptr, step.state.e, ex, stream, marks[2], marks[3]);
                }
                launchAdaptiveSelect(list, active, width, height, step.state, params.maxSpp, params.threshold, b.scratch(), b.list(turn ^ 1u), stream);
                HIP_CHECK(hipGetLastError());
                HIP_CHECK(hipMemcpyAsync(&active, b.scratch().total, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
                HIP_CHECK(hipStreamSynchronize(stream));
                if (timed) {
                    float outMs = 0.0f, inMs = 0.0f;
                    HIP_CHECK(hipEventElapsedTime(&outMs, marks[0], marks[1]));
                    HIP_CHECK(hipEventElapsedTime(&inMs, marks[2], marks[3]));
                    std::fprintf(stderr, "[multi] partition %u round %u: halo %zu bytes each way; pack + copy %.4f ms, copy + unpack %.4f ms\n", p, rounds,
                                 haloBytes, outMs, inMs);
                }
            }
            published[p] = active;
            // 4. every total is published; the outboxes may be overwritten again
            if (!meet()) return;
            // 5. the same total and the same n on every thread: all leave or all go on
            uint64_t total = 0u;
            for (uint32_t q = 0; q < parts; ++q) total += published[q];
            if (p == 0u) {
                if (rounds < PTR_ADAPTIVE_INFO_ROUNDS) info.activeAfter[rounds] = static_cast<uint32_t>(total);
                info.rounds = rounds + 1u;
                sharedCount = n;
            }
            ++rounds;
            turn ^= 1u;
            more = total > 0u && n < params.maxSpp;
        }
        launchMultiFinishBands(mp, step.state, dRgb, dCov, dCount, stream);
        HIP_CHECK(hipGetLastError());
        handOver();
        renderSeconds[p] = since(r0);
        partStats[p] = sum;
        scenes[p] = std::move(ds);
    };

    // a worker, however it ended, joins its stream and launches nothing more; the stream was this call's
    runPartitionThreads(
        rq.devices, workerSeconds.data(), waitSeconds.data(), body, [&](uint32_t p) { return streams[p]; },
        [&](uint32_t p) {
            if (streams[p]) (void)hipStreamDestroy(streams[p]);
        });

    const double partsDone = since(t0);
    HIP_CHECK(hipSetDevice(rootDevice));
    float* const iRgb = image.ptr;
    float* const iCov = image.ptr + pixels * covAt;
    float* const iCount = image.ptr + pixels * countAt;
    bands.interleave(iRgb, wantCov ? iCov : nullptr, wantCount ? iCount : nullptr, nullptr);
    HIP_CHECK(hipMemcpy(rq.outRgb, iRgb, pixels * 3u * sizeof(float), hipMemcpyDeviceToHost));
    if (wantCov) HIP_CHECK(hipMemcpy(rq.outCov, iCov, pixels * 6u * sizeof(float), hipMemcpyDeviceToHost));
    if (wantCount) HIP_CHECK(hipMemcpy(rq.outCount, iCount, pixels * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (!probe && (rq.outAlbedo || rq.outNormal)) {   // the first partition's scene is on the first device
        DeviceBuffer<float4> albedo, normal;
        downloadFirstHit(*scenes[0], settings, 0u, albedo, normal, rq.outAlbedo, rq.outNormal);
    }
    const double gatherSeconds = since(t0) - partsDone;   // interleave, download, feature buffers
    for (uint32_t p = 0; p < parts; ++p) {
        if (scenes[p]) {
            (void)hipSetDevice(scenes[p]->device);
            scenes[p].reset();
        }
    }
    (void)hipSetDevice(rootDevice);
    const double wall = since(t0);

    double slowestRender = 0.0, slowestUpload = 0.0;
    uint64_t samples = 0u;
    for (uint32_t p = 0; p < parts; ++p) {
        slowestRender = std::max(slowestRender, renderSeconds[p]);
        slowestUpload = std::max(slowestUpload, uploadSeconds[p]);
        samples += partSamples[p];
        info.pixelsAtMax += partAtMax[p];
    }
    info.totalSamples = samples;
    if (rq.stats) {
        std::memset(rq.stats, 0, sizeof(*rq.stats));
        rq.stats->totalSeconds = slowestRender;
        rq.stats->avgMsPerSample = slowestRender * 1000.0 / std::max(1u, adaptive ? sharedCount : rq.spp);
        rq.stats->uploadSeconds = prepared.seconds + slowestUpload;
        for (uint32_t p = 0; p < parts; ++p) addLaunchStats(*rq.stats, partStats[p]);
        rq.stats->samples = samples;
    }
    if (rq.info && adaptive) *rq.info = info;
    if (rq.multi) {
        std::memset(rq.multi, 0, sizeof(*rq.multi));
        rq.multi->parts = parts;
        rq.multi->stagedParts = stagedParts.load();
        for (uint32_t p = 0; p < parts; ++p) {
            rq.multi->partSamples[p] = partSamples[p];
            rq.multi->partRenderSeconds[p] = renderSeconds[p];
            rq.multi->partWaitSeconds[p] = waitSeconds[p];
        }
    }
    if (rq.verbose) {
        std::fprintf(stderr, "[ptr] %u device(s): scene preparation %.3f s, slowest upload %.3f s, slowest render + hand-over %.3f s, whole call %.3f s\n", parts,
                     prepared.seconds, slowestUpload, slowestRender, wall);
        const bool plain = rq.kind == Kind::Plain;   // the plain frame reports the render time of each partition and nothing more
        // (tools/multi_adaptive_cost.py parses this line; the partitions' threads are what the whole call has beside the other four)
        if (!plain) {
            std::fprintf(stderr, "[ptr]   outside the partitions' threads: first-device buffers %.4f s, interleave + download %.4f s, release of the scenes %.4f s\n",
                         setupSeconds, gatherSeconds, wall - partsDone - gatherSeconds);
        }
        for (uint32_t p = 0; p < parts; ++p) {
            if (plain) {
                std::fprintf(stderr, "[ptr]   device %d: %u bands, render %.3f s\n", rq.devices[p], partBands[p], renderSeconds[p]);
                continue;
            }
            std::fprintf(stderr, "[ptr]   device %d: %u bands, %llu samples, upload %.4f s, state %.4f s, render %.4f s, of which waiting %.4f s\n", rq.devices[p],
                         partBands[p], static_cast<unsigned long long>(partSamples[p]), uploadSeconds[p], stateSeconds[p], renderSeconds[p], waitSeconds[p]);
        }
    }
}

// The checks every entry point makes before any device call, then the device list.  Returns the C-ABI's code; 0 with rq.devices filled in.
int admit(Request& rq, char* err, size_t cap) {
    const std::string w(rq.who);
    const bool probe = rq.kind == Kind::Probe, adaptive = probe || rq.kind == Kind::Adaptive;
    if (!(probe ? rq.samples != nullptr : rq.scene != nullptr) || !rq.settings || !rq.outRgb || (adaptive && !rq.params) || (rq.listed && !rq.ids)) {
        return nullArgument(rq.who, err, cap);
    }
    std::string bad;
    if (rq.settings->width == 0u || rq.settings->height == 0u) bad = w + ": render size must be non-zero";
    else if (adaptive) bad = badAdaptiveParams(rq.who, *rq.params);
    else if (rq.kind == Kind::Covariance && rq.spp < 2u) bad = w + ": a sample covariance needs spp >= 2";
    if (bad.empty()) bad = badDeviceRequest(w, rq.listed, rq.n);
    if (!bad.empty()) return refuse(err, cap, bad);
    return pickDevices(rq.who, rq.ids, rq.n, rq.listed, rq.settings->height, rq.devices, rq.forceStaged, err, cap);
}

int frame(Request& rq, char* err, size_t cap) {
    if (const int rc = admit(rq, err, cap)) return rc;
    try {
        runFrame(rq);
        return 0;
    }
    PTR_CATCH_ALL(err, cap)
}

}  // namespace

extern "C" {

int ptr_render_multi(const PtrSceneDesc* scene, const PtrSettings* settings, uint32_t spp, int n_devices, int verbose, float* out_rgb,
                     PtrRenderStats* stats, char* err, size_t err_cap) {
    Request rq;
    rq.who = "ptr_render_multi", rq.kind = Kind::Plain;
    rq.scene = scene, rq.settings = settings, rq.spp = std::max(1u, spp);   // (spp 0 renders one sample, as renderBands has it)
    rq.n = n_devices, rq.verbose = verbose;
    rq.outRgb = out_rgb, rq.stats = stats;
    return frame(rq, err, err_cap);
}

int ptr_debug_render_multi_on(const PtrSceneDesc* scene, const PtrSettings* settings, uint32_t spp, const int* device_ids, int n, float* out_rgb,
                              PtrRenderStats* stats, char* err, size_t err_cap) {
    Request rq;
    rq.who = "ptr_debug_render_multi_on", rq.kind = Kind::Plain;
    rq.scene = scene, rq.settings = settings, rq.spp = std::max(1u, spp);
    rq.ids = device_ids, rq.n = n, rq.listed = true;
    rq.outRgb = out_rgb, rq.stats = stats;
    return frame(rq, err, err_cap);
}

int ptr_render_multi_cov(const PtrSceneDesc* scene, const PtrSettings* settings, uint32_t spp, int n_devices, int verbose, float* out_rgb,
                         float* out_cov, float* out_albedo, float* out_normal, PtrRenderStats* stats, PtrMultiInfo* multi_info, char* err,
                         size_t err_cap) {
    Request rq;
    rq.who = "ptr_render_multi_cov", rq.kind = Kind::Covariance;
    rq.scene = scene, rq.settings = settings, rq.spp = spp;
    rq.n = n_devices, rq.verbose = verbose;
    rq.outRgb = out_rgb, rq.outCov = out_cov, rq.outAlbedo = out_albedo, rq.outNormal = out_normal;
    rq.stats = stats, rq.multi = multi_info;
    return frame(rq, err, err_cap);
}

int ptr_render_multi_adaptive(const PtrSceneDesc* scene, const PtrSettings* settings, const PtrAdaptiveParams* params, int n_devices,
                              int verbose, float* out_rgb, float* out_cov, uint32_t* out_count, float* out_albedo, float* out_normal,
                              PtrRenderStats* stats, PtrAdaptiveInfo* adaptive_info, PtrMultiInfo* multi_info, char* err, size_t err_cap) {
    Request rq;
    rq.who = "ptr_render_multi_adaptive", rq.kind = Kind::Adaptive;
    rq.scene = scene, rq.settings = settings, rq.params = params;
    rq.n = n_devices, rq.verbose = verbose;
    rq.outRgb = out_rgb, rq.outCov = out_cov, rq.outCount = out_count, rq.outAlbedo = out_albedo, rq.outNormal = out_normal;
    rq.stats = stats, rq.info = adaptive_info, rq.multi = multi_info;
    return frame(rq, err, err_cap);
}

int ptr_multi_debug_cov_on(const PtrSceneDesc* scene, const PtrSettings* settings, uint32_t spp, const int* device_ids, int n,
                           float* out_rgb, float* out_cov, float* out_albedo, float* out_normal, PtrRenderStats* stats,
                           PtrMultiInfo* multi_info, char* err, size_t err_cap) {
    Request rq;
    rq.who = "ptr_multi_debug_cov_on", rq.kind = Kind::Covariance;
    rq.scene = scene, rq.settings = settings, rq.spp = spp;
    rq.ids = device_ids, rq.n = n, rq.listed = true;
    rq.outRgb = out_rgb, rq.outCov = out_cov, rq.outAlbedo = out_albedo, rq.outNormal = out_normal;
    rq.stats = stats, rq.multi = multi_info;
    return frame(rq, err, err_cap);
}

int ptr_multi_debug_adaptive_on(const PtrSceneDesc* scene, const PtrSettings* settings, const PtrAdaptiveParams* params,
                                const int* device_ids, int n, float* out_rgb, float* out_cov, uint32_t* out_count, float* out_albedo,
                                float* out_normal, PtrRenderStats* stats, PtrAdaptiveInfo* adaptive_info, PtrMultiInfo* multi_info,
                                char* err, size_t err_cap) {
    Request rq;
    rq.who = "ptr_multi_debug_adaptive_on", rq.kind = Kind::Adaptive;
    rq.scene = scene, rq.settings = settings, rq.params = params;
    rq.ids = device_ids, rq.n = n, rq.listed = true;
    rq.outRgb = out_rgb, rq.outCov = out_cov, rq.outCount = out_count, rq.outAlbedo = out_albedo, rq.outNormal = out_normal;
    rq.stats = stats, rq.info = adaptive_info, rq.multi = multi_info;
    return frame(rq, err, err_cap);
}

int ptr_multi_debug_adaptive_frame(uint32_t width, uint32_t height, const PtrAdaptiveParams* params, const float* samples,
                                   const int* device_ids, int n, float* out_rgb, float* out_cov, uint32_t* out_count,
                                   PtrAdaptiveInfo* adaptive_info, char* err, size_t err_cap) {
    PtrSettings size{};
    size.width = width, size.height = height;
    Request rq;
    rq.who = "ptr_multi_debug_adaptive_frame", rq.kind = Kind::Probe;
    rq.settings = &size, rq.params = params, rq.samples = samples;
    rq.ids = device_ids, rq.n = n, rq.listed = true;
    rq.outRgb = out_rgb, rq.outCov = out_cov, rq.outCount = out_count;
    rq.info = adaptive_info;
    return frame(rq, err, err_cap);
}

}  // extern "C"
