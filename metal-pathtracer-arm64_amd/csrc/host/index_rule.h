// The one rule every update call's list shares: an entry names an entity of the scene by index, the index is below the scene's count, and
// one call names no index a second time.  Header only, plain C++ (no HIP): the hipcc-compiled check halves (dynamic_host.h) and
// appearance_host.cpp, which tools/appearance_host_check.cpp runs under sanitizers, state it through this.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

namespace ptr {

// named: one byte per entity of the scene, 0 before the call's first entry; an accepted index is marked there.  kind / plural: "mesh" /
// "meshes".  Returns "", "<kind> index N out of range (the scene has C <plural>)" with C = named.size(), or that N was named before.
inline std::string NamedIndexProblem(const char* kind, const char* plural, uint32_t index, std::vector<uint8_t>& named) {
    if (index >= named.size()) {
        return std::string(kind) + " index " + std::to_string(index) + " out of range (the scene has " + std::to_string(named.size()) + " " + plural + ")";
    }
    if (named[index]) return std::string(kind) + " index " + std::to_string(index) + " named twice";
    named[index] = 1;
    return "";
}

}  // namespace ptr
