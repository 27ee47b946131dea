// ez_multi_shards.h — the shard arithmetic of the multi-device batch calls (ez_multi.hip): plain C++,
// no HIP, so that tools/multi_shards_check.cpp holds it to a brute-force statement of the rule on the
// host (tests/test_multi_shards.py).
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace ez {
// Contiguous whole-stream shards of a batch, balanced by bytes: shard k is streams [first[k],
// first[k+1]) with first[k] the first stream starting at or after k / nshard of the batch's bytes.
inline std::vector<uint64_t> shard_bounds(const uint64_t *off, uint64_t count, int nshard) {
    std::vector<uint64_t> first((size_t)nshard + 1, count);
    first[0] = 0;
    const uint64_t total = off[count] - off[0];
    uint64_t s = 0;
    for (int k = 1; k < nshard; k++) {
        // (rounded up: a start below total * k / nshard is not "at or after" it; at most total, so no wrap)
        const uint64_t target = off[0] + (uint64_t)(((unsigned __int128)total * (uint64_t)k + (uint64_t)(nshard - 1)) / (uint64_t)nshard);
        while (s < count && off[s] < target) s++;
        first[(size_t)k] = s;
    }
    return first;
}

// a shard's count + 1 offsets, from its first stream's
inline std::vector<uint64_t> rebased(const uint64_t *off, uint64_t first, uint64_t count) {
    std::vector<uint64_t> v(count + 1);
    for (uint64_t t = 0; t <= count; t++) v[t] = off[first + t] - off[first];
    return v;
}
// the largest stream (or slot) between them
inline uint64_t max_span(const std::vector<uint64_t> &off) {
    uint64_t mx = 0;
    for (size_t t = 1; t < off.size(); t++) mx = off[t] - off[t - 1] > mx ? off[t] - off[t - 1] : mx;
    return mx;
}

// whether count + 1 offsets never decrease (the multi-device calls refuse the others before any
// device use: rebased and the shards' buffer sizes subtract them unsigned)
inline bool offsets_ascend(const uint64_t *off, uint64_t count) {
    for (uint64_t s = 0; s < count; s++)
        if (off[s + 1] < off[s]) return false;
    return true;
}
}  // namespace ez
