// ez_k2_layout.h — the part layout of the K2 parts routes (ez_decompress_parts.hip,
// ez_decompress_segs_parts.hip): the scratch header's words, the records a hint pays for, and the steps
// of the one layout kernel (kp_layout) as functions over plain pointers.  The scratch is sized from the
// caller's in_bytes hint alone (parts_cap); layout_gate is all that keeps a wrong hint from indexing past
// it: with the gate closed no kernel touches a record and the wave route takes the whole batch.
// Plain C++, no HIP: tools/k2_layout_check.cpp holds the steps, run over emulated threads on the host,
// to a serial layout written apart (tests/test_k2_layout.py).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define EZ_LAYOUT_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define EZ_LAYOUT_HD static inline
#endif

namespace ez {

// the scratch's header words: the gate, the batch's parts, and the routes' counters (K2z: parts in the
// first pass, records taken as they stood, parts walked again; K2g the same and the parts filled)
enum : int { kHGate = 0, kHParts = 1, kHFirst = 2, kHJoined = 3, kHAgain = 4, kHFilled = 5, kHWords = 16 };

constexpr int kLayoutThreads = 1024;  // kp_layout's one block

// The records a batch's scratch holds: every stream's parts are at most its bytes / part_bytes, rounded
// up.  0: 2^31 or more, which the 32-bit part indices do not reach (the batch takes the wave route).
EZ_LAYOUT_HD uint64_t parts_cap(uint64_t in_bytes, uint32_t part_bytes, uint64_t count) {
    const uint64_t whole = in_bytes / part_bytes, end = 1ull << 31;
    return whole >= end || count >= end - 1 - whole ? 0 : whole + count + 1;
}

// thread t of T lays out the streams [lo, hi): ceil(count / T) each, none for the threads past the end
struct LayoutRange {
    uint64_t lo, hi;
};
EZ_LAYOUT_HD LayoutRange layout_range(uint64_t count, int T, int t) {
    const uint64_t per = (count + (uint64_t)T - 1) / (uint64_t)T;
    const uint64_t lo = (uint64_t)t * per < count ? (uint64_t)t * per : count;
    return LayoutRange{lo, per < count - lo ? lo + per : count};
}

// One thread, between the threads' counting (base[s] = the parts of stream s, sums[t] = thread t's
// total) and their scans: sums becomes its exclusive scan, and the gate opens only if the batch's real
// extent is within the hint and its parts within the cap the scratch was sized for.  Writes
// hdr[kHGate], hdr[kHParts] and base[count]: all 0 where it stays closed.
EZ_LAYOUT_HD bool layout_gate(uint64_t *sums, int T, const uint64_t *in_off, uint64_t count, uint64_t in_bytes, uint64_t cap, uint32_t *hdr,
                              uint32_t *base) {
    uint64_t run = 0;
    for (int k = 0; k < T; k++) {
        const uint64_t v = sums[k];
        sums[k] = run;
        run += v;
    }
    const bool ok = in_off[count] >= in_off[0] && in_off[count] - in_off[0] <= in_bytes && run <= cap;
    hdr[kHParts] = ok ? (uint32_t)run : 0u;
    hdr[kHGate] = ok ? 1u : 0u;
    base[count] = ok ? (uint32_t)run : 0u;
    return ok;
}

// a thread's part counts become their exclusive scan, in place, from the parts before its range
// (32 bits: wraps only where the gate stays closed)
EZ_LAYOUT_HD void layout_scan(uint32_t *base, LayoutRange r, uint64_t before) {
    for (uint64_t s = r.lo; s < r.hi; s++) {
        const uint32_t parts = base[s];
        base[s] = (uint32_t)before;
        before += parts;
    }
}

}  // namespace ez
