// Resumable frames between the rounds of a refine (include/ptr_frame.h, whose text this file follows): the per-element bodies of the
// kernels in frame.hip, written as host + device functions on plain pointers like those of adaptive.h, so that the renderer, the
// test-only frame and a host program that walks the index arithmetic all run the same code, and the launchers.
#pragma once

#include "adaptive.h"

namespace ptrk {

constexpr uint32_t kFrameNoCount = 0xFFFFFFFFu;   // the class minimum of an empty list

// n_min: the count of list entry j folded into a running minimum (j < count; the list names in-image pixels).
PTR_HD uint32_t frameClassMin(uint32_t running, const uint32_t* list, uint32_t j, const uint32_t* n) {
    const uint32_t mine = n[list[j]];
    return mine < running ? mine : running;
}

// S: is list entry j in the class of the round?
PTR_HD bool frameInClass(const uint32_t* list, uint32_t j, const uint32_t* n, uint32_t nMin) { return n[list[j]] == nMin; }

// The next L: an entry outside S stays untouched; an entry of S stays iff Select keeps it (e and n are those after the round's update).
PTR_HD bool frameMergeKeep(const uint32_t* list, uint32_t j, const uint8_t* inS, uint32_t width, uint32_t height, const float* e, const uint32_t* n,
                           uint32_t maxSpp, float threshold) {
    return inS[j] == 0u || adaptiveKeep(list[j], width, height, e, n, maxSpp, threshold);
}

#if defined(__HIPCC__)
// *dMin = min(*dMin, the smallest n of the list's pixels): the caller sets *dMin to kFrameNoCount first.
void launchFrameClassMin(const uint32_t* dList, uint32_t count, const uint32_t* dN, uint32_t* dMin, hipStream_t stream);
// S = the entries of dList whose pixel has nMin samples, in order, into dS; *scratch.total their number; dInS[j] = 1 for them, 0 otherwise.
void launchFrameSplit(const uint32_t* dList, uint32_t count, const uint32_t* dN, uint32_t nMin, uint8_t* dInS, const AdaptiveScratch& scratch,
                      uint32_t* dS, hipStream_t stream);
// Select on S and the merge: dNext = dList without the entries of S that Select drops, in order; *scratch.total its length.
void launchFrameMerge(const uint32_t* dList, uint32_t count, const uint8_t* dInS, uint32_t width, uint32_t height, const AdaptiveState& state,
                      uint32_t maxSpp, float threshold, const AdaptiveScratch& scratch, uint32_t* dNext, hipStream_t stream);
#endif

}  // namespace ptrk
