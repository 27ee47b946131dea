// multi_shards_check.cpp — host check of eazy_amd/csrc/ez_multi_shards.h, the shard arithmetic of the
// multi-device batch calls.  shard_bounds is held to a brute-force statement of its rule: for each k
// in 1..nshard-1, first[k] is the first stream s, scanning from 0, with
// (off[s] - off[0]) * nshard >= total * k in 128 bits (count when there is none).  Per case it also
// asserts first[0] == 0, first[nshard] == count, first never decreases, every shard's bytes are less
// than total / nshard + 1 + the longest stream, and per shard that rebased starts at 0 and ends at the
// shard's bytes and max_span is the longest difference.
//
// Cases: every length vector over {0, 1, 2, 5} with count 0..6, nshard 1..9, off[0] in {0, 7}; one
// stream of 1000 among 60 of 1 (first, middle, last; nshard 1..9); 20 empty streams (off[0] in {0, 7});
// 1, 2 and 3 streams on 4..9 shards; totals of 2^32 - 1, 2^32 + 1, 2^63 and 2^64 - 16 in three streams
// (off[0] in {0, 7}), where a 64-bit product would wrap.  Prints "multi_shards ok: N cases".
//
// Build: g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//        -I eazy_amd/csrc -o tools/multi_shards_check tools/multi_shards_check.cpp
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "ez_multi_shards.h"

typedef unsigned __int128 u128;

static uint64_t g_cases = 0;
static std::string g_what;  // the case at hand, for a failure's message

#define CHECK(c)                                                                                     \
    do {                                                                                             \
        if (!(c)) {                                                                                  \
            std::printf("FAILED %s (line %d): %s\n", #c, __LINE__, g_what.c_str());                  \
            std::exit(1);                                                                            \
        }                                                                                            \
    } while (0)

static void describe(const std::vector<uint64_t> &off, int nshard, const std::vector<uint64_t> &first) {
    g_what = "nshard " + std::to_string(nshard) + ", off";
    for (size_t t = 0; t < off.size() && t < 12; t++) g_what += " " + std::to_string(off[t]);
    g_what += ", first";
    for (uint64_t f : first) g_what += " " + std::to_string(f);
}

// one case: lens from off0 on nshard shards
static void run(const std::vector<uint64_t> &lens, uint64_t off0, int nshard) {
    const uint64_t count = lens.size();
    std::vector<uint64_t> off(count + 1);
    off[0] = off0;
    uint64_t longest = 0;
    for (uint64_t s = 0; s < count; s++) {
        off[s + 1] = off[s] + lens[s];
        longest = lens[s] > longest ? lens[s] : longest;
    }
    const uint64_t total = off[count] - off[0];
    const std::vector<uint64_t> first = ez::shard_bounds(off.data(), count, nshard);
    describe(off, nshard, first);
    CHECK(ez::offsets_ascend(off.data(), count));
    CHECK(first.size() == (size_t)nshard + 1);
    CHECK(first[0] == 0);
    CHECK(first[(size_t)nshard] == count);
    for (int k = 1; k < nshard; k++) {  // the rule, brute force
        uint64_t s = 0;
        while (s < count && !((u128)(off[s] - off[0]) * (u128)nshard >= (u128)total * (u128)k)) s++;
        CHECK(first[(size_t)k] == s);
    }
    for (int k = 0; k < nshard; k++) {
        const uint64_t a = first[(size_t)k], b = first[(size_t)k + 1];
        CHECK(a <= b);
        CHECK(b <= count);
        const uint64_t bytes = off[b] - off[a];
        CHECK((u128)bytes < (u128)(total / (uint64_t)nshard) + 1 + (u128)longest);
        const std::vector<uint64_t> r = ez::rebased(off.data(), a, b - a);
        CHECK(r.size() == b - a + 1);
        CHECK(r[0] == 0);
        CHECK(r[b - a] == bytes);
        uint64_t mx = 0;
        for (uint64_t t = a; t < b; t++) {
            CHECK(r[t - a + 1] - r[t - a] == lens[t]);
            mx = lens[t] > mx ? lens[t] : mx;
        }
        CHECK(ez::max_span(r) == mx);
    }
    g_cases++;
}

int main() {
    // every length vector over {0, 1, 2, 5} with count 0..6
    const uint64_t alphabet[4] = {0, 1, 2, 5};
    for (int count = 0; count <= 6; count++) {
        uint64_t vectors = 1;
        for (int t = 0; t < count; t++) vectors *= 4;
        for (uint64_t v = 0; v < vectors; v++) {
            std::vector<uint64_t> lens((size_t)count);
            uint64_t x = v;
            for (int t = 0; t < count; t++, x /= 4) lens[(size_t)t] = alphabet[x % 4];
            for (int nshard = 1; nshard <= 9; nshard++)
                for (uint64_t off0 : {0ull, 7ull}) run(lens, off0, nshard);
        }
    }
    // one stream of 1000 among 60 of 1: first, in the middle, last
    for (size_t at : {(size_t)0, (size_t)30, (size_t)60}) {
        std::vector<uint64_t> lens(61, 1);
        lens[at] = 1000;
        for (int nshard = 1; nshard <= 9; nshard++) run(lens, 0, nshard);
    }
    // only empty streams
    for (int nshard = 1; nshard <= 9; nshard++)
        for (uint64_t off0 : {0ull, 7ull}) run(std::vector<uint64_t>(20, 0), off0, nshard);
    // fewer streams than shards
    for (int nshard = 4; nshard <= 9; nshard++) {
        run({3}, 0, nshard);
        run({3, 4}, 0, nshard);
        run({3, 4, 5}, 0, nshard);
    }
    // totals where total * k wraps 64 bits, in three streams
    const uint64_t totals[4] = {(1ull << 32) - 1, (1ull << 32) + 1, 1ull << 63, ~0ull - 15};
    for (uint64_t total : totals) {
        const uint64_t a = total / 3, b = total / 2 - a;
        for (int nshard = 1; nshard <= 9; nshard++)
            for (uint64_t off0 : {0ull, 7ull}) run({a, b, total - a - b}, off0, nshard);
    }
    // decreasing offsets are told from ascending ones
    {
        const uint64_t down[4] = {0, 10, 9, 20}, flat[4] = {5, 5, 5, 5}, last[3] = {0, 4, 3};
        g_what = "offsets_ascend";
        CHECK(!ez::offsets_ascend(down, 3));
        CHECK(ez::offsets_ascend(down, 1));
        CHECK(ez::offsets_ascend(flat, 3));
        CHECK(!ez::offsets_ascend(last, 2));
        CHECK(ez::offsets_ascend(last, 0));
    }
    std::printf("multi_shards ok: %llu cases\n", (unsigned long long)g_cases);
    return 0;
}
