// What the two drivers of frames on several devices share on the host - the one-shot frames of multi.cpp (include/ptr_multi.h) and the
// resumable frame of multi_frame.cpp (include/ptr_multi_frame.h): the device list of a call and its refusals, the pinned memory the
// partitions exchange their band-edge rows of e through with the two halves of that exchange, the hand-over of a partition's band
// buffer to the first device, the gather there with its interleave into image order, and the one driver that runs a call's partitions
// on threads which meet at a round barrier (round_barrier.h) and end together when one of them fails.  Implemented in multi.cpp.
// Internal: not part of the C-ABI.
#pragma once

#include <chrono>
#include <string>
#include <vector>

#include "../kernels/multi.h"
#include "device_scene.h"
#include "parallel.h"
#include "round_barrier.h"

namespace ptrhost {

// "<who>: ..." for an id list (listed) or a device count whose length alone is wrong, empty otherwise.  No device call.
std::string badDeviceRequest(const std::string& who, bool listed, int n);
// The devices of a call, after its other arguments were found good: the n that `ids` lists (listed; an id given as -(id + 1) sends that
// partition's bands through pinned host memory) or the first n (n <= 0: all there are; never more than the image has bands).  Returns
// the C-ABI's code - 2 without a device or with fewer than asked for, 1 for an id past the visible ones - or 0 with both vectors filled.
int pickDevices(const char* who, const int* ids, int n, bool listed, uint32_t height, std::vector<int>& devices, std::vector<char>& forceStaged,
                char* err, size_t cap);

// The pinned host memory the partitions exchange their edge rows through (portable: every device's copies may use it).  Partition p
// publishes into its outbox - its edge rows as k_multi_halo_pack lays them out - and collects its neighbours' rows in its inbox.
struct HaloExchange {
    float* host = nullptr;
    std::vector<size_t> offset;   // of partition p's edge rows in either half, in floats; [parts] = the size of a half
    HaloExchange() = default;
    HaloExchange(const HaloExchange&) = delete;
    HaloExchange& operator=(const HaloExchange&) = delete;
    ~HaloExchange() {
        if (host) (void)hipHostFree(host);
    }
    // room for partBands[p] bands of `width` pixels per partition, zeroed: nothing but zeros is published yet
    void allocate(const std::vector<uint32_t>& partBands, uint32_t width);
    // every outbox back to zero: what a reset of all partitions publishes
    void publishZeros();
    float* outbox(uint32_t p) const { return host + offset[p]; }
    float* inbox(uint32_t p) const { return host + offset.back() + offset[p]; }
    size_t haloBytes(uint32_t p) const { return (offset[p + 1u] - offset[p]) * sizeof(float); }
};

// Publish: the first and last row of every band of partition mp.part, from its image-order e array through dEdge (bands * 2 * width
// floats) into its outbox, asynchronous on `stream`; the outbox is written once the stream is joined.  before / after (nullable) are
// recorded around it.
void haloPublish(const ptrk::MultiPart& mp, const float* dE, float* dEdge, const HaloExchange& ex, hipStream_t stream, hipEvent_t before = nullptr,
                 hipEvent_t after = nullptr);
// Collect: the rows above and below every band of partition mp.part, from their owners' outboxes through its inbox and dEdge into its
// image-order e array, asynchronous on `stream`.  Every owner's publish must be complete, and none may publish again before this
// partition's stream is joined.
void haloCollect(const ptrk::MultiPart& mp, float* dEdge, float* dE, const HaloExchange& ex, hipStream_t stream, hipEvent_t before = nullptr,
                 hipEvent_t after = nullptr);

// A partition's band buffer travels to the first device of the frame: a plain copy when it is local, device-to-device over the fabric
// when the two devices can address each other, through pinned host memory otherwise (or with forceStaged, the tests' hook).  Called on
// the partition's thread with `device` current; asynchronous on `stream` except for the staged path.  True when the bytes were staged.
bool sendBandsToRoot(void* dRootDst, int rootDevice, const void* dSrc, int device, size_t bytes, bool forceStaged, hipStream_t stream);

// The gather of the partitions' outputs on the first device.  A partition's outputs are one buffer in band layout - rgb, then cov from
// word covAt of a pixel on, then count from word countAt on, pixelWords in all - so that it travels in one transfer.  Here: the
// partitions' buffers one after the other, and the word each output of each partition starts at (k_multi_interleave's table:
// [output][partition]).
struct BandGather {
    uint32_t parts = 0, width = 0, height = 0, pixelWords = 0;
    std::vector<uint64_t> partPixel;    // where partition p's buffer starts among all of them, in pixels; [parts] = all of them
    std::vector<uint64_t> wordOffset;
    DeviceBuffer<float> gathered;
    DeviceBuffer<uint64_t> dWordOffset;

    // the first device is current
    void allocate(const std::vector<uint32_t>& partBands, uint32_t imageWidth, uint32_t imageHeight, uint32_t covAt, uint32_t countAt, uint32_t words);
    size_t bandPixels(uint32_t p) const { return static_cast<size_t>(partPixel[p + 1u] - partPixel[p]); }
    size_t bandBytes(uint32_t p) const { return bandPixels(p) * pixelWords * sizeof(float); }
    float* slot(uint32_t p) const { return gathered.ptr + wordOffset[p]; }
    // from the gathered buffers into image order (dCov and dCount nullable), asynchronous on `stream` of the first device, which is current
    void interleave(float* dRgb, float* dCov, void* dCount, hipStream_t stream) const;
};

using Clock = std::chrono::steady_clock;
inline double since(Clock::time_point t0) { return std::chrono::duration<double>(Clock::now() - t0).count(); }

// One call's partitions on threads, partition p on devices[p]: body(p, meet) with that device current.  meet() is the round barrier -
// false once a partition has failed, and the body then returns at once.  Every way out of a worker but the regular one releases the
// partitions that wait for it.  However the body ended, the worker joins streamOf(p) (where not null), then runs done(p).  seconds /
// waited (an entry per partition): in the worker and of those in meet().  A failure is thrown with the device's id.
template <typename Body, typename StreamOf, typename Done>
void runPartitionThreads(const std::vector<int>& devices, double* seconds, double* waited, Body&& body, StreamOf&& streamOf, Done&& done) {
    const uint32_t parts = static_cast<uint32_t>(devices.size());
    std::vector<std::string> errors(parts);
    ptr::RoundBarrier barrier(parts);
    auto worker = [&](uint32_t p) {
        const auto t0 = Clock::now();
        waited[p] = 0.0;
        auto meet = [&]() -> bool {
            const auto m0 = Clock::now();
            const bool all = barrier.arriveAndWait();
            waited[p] += since(m0);
            return all;
        };
        try {
            HIP_CHECK(hipSetDevice(devices[p]));
            body(p, meet);
            HIP_CHECK(hipGetLastError());
        } catch (const HipError& e) {
            barrier.fail();
            errors[p] = e.message;
        } catch (const std::exception& e) {
            barrier.fail();
            errors[p] = std::string("exception: ") + e.what();
        } catch (...) {
            barrier.fail();
            errors[p] = "unknown exception";
        }
        if (hipStream_t stream = streamOf(p)) (void)hipStreamSynchronize(stream);
        done(p);
        seconds[p] = since(t0);
    };
    ptr::runOnThreads(parts, worker, [&] { barrier.fail(); });   // (a thread that could not be started never arrives)
    for (uint32_t p = 0; p < parts; ++p) {
        if (!errors[p].empty()) throw HipError{"device " + std::to_string(devices[p]) + ": " + errors[p]};
    }
    if (barrier.failed()) throw HipError{"a partition left the frame early"};
}

}  // namespace ptrhost
