// What tests/facade_stub.cc (a stub of the C ABI that models an engine by its counts alone) shares with
// tests/facade_sizes.cc: the counts, the byte pattern of every output and the log of every input.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace stub {

// pairwise distinct, so that a confusion of two of them changes a size
struct Counts {
    size_t verts = 7, faces = 5, cloths = 3, links = 11, anchors = 4, hinges = 6, bodies = 2, pins = 8, fields = 9,
           grid_bodies = 10, materials = 13, contacts = 14;
    size_t particles() const { return verts + faces; }
};
extern Counts N;

// one call of an entry point: its name, its scalar arguments (a pointer as 0 / 1 for null / not null) and the bytes it
// read through its input pointers, in argument order
struct Call {
    std::string fn;
    std::vector<long long> args;
    std::vector<unsigned char> bytes;
};
extern std::vector<Call> LOG;

// the byte an output named `what` ("entry point.argument") holds at byte offset k
inline unsigned tag(const char* what) {
    unsigned h = 2166136261u;
    for (const char* p = what; *p; ++p) h = (h ^ (unsigned char)*p) * 16777619u;
    return h;
}
inline unsigned char pattern(const char* what, size_t k) { return (unsigned char)(tag(what) % 251u + 11u * k + 1u); }

// is `v` exactly n items holding the pattern of `what` from its first to its last byte?
template <class R>
bool holds(const std::vector<R>& v, size_t n, const char* what) {
    if (v.size() != n) return false;
    const unsigned char* b = reinterpret_cast<const unsigned char*>(v.data());
    for (size_t k = 0; k < n * sizeof(R); ++k)
        if (b[k] != pattern(what, k)) return false;
    return true;
}

// values the facade does arithmetic on, so that they are numbers and not a byte pattern
inline float tear_limit(size_t cloth) { return 1.5f + 0.25f * float(cloth); }
constexpr double KINETIC = 3.0, KINETIC_AFFINE = 0.5, GRAVITY = -7.0, IN_PLANE = 11.0, NORMAL = 13.0, SHEAR = 17.0, BENDING = 19.0;
constexpr double LINK_ENERGY = 23.0, ANCHOR_ENERGY = 29.0, ANCHOR_QUANTUM = 31.0, WEAVE_TOTAL = 37.0;
constexpr float GUARD_DT = 0.0625f;
constexpr uint32_t BROKEN = 41u, COUPLING = 3u, TOUCHED = 43u;

}  // namespace stub
