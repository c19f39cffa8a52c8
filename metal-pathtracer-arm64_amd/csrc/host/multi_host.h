// What the two drivers of frames on several devices share on the host - the one-shot frames of multi.cpp (include/ptr_multi.h) and the
// resumable frame of multi_frame.cpp (include/ptr_multi_frame.h): the device list of a call and its refusals, the pinned memory the
// partitions exchange their band-edge rows of e through with the two halves of that exchange, and the hand-over of a partition's band
// buffer to the first device.  Implemented in multi.cpp.  Internal: not part of the C-ABI.
#pragma once

#include <string>
#include <vector>

#include "../kernels/multi.h"
#include "device_scene.h"

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

}  // namespace ptrhost
