// k2_layout_check.cpp — host check of eazy_amd/csrc/ez_k2_layout.h, the part layout of the K2 parts
// routes (kp_layout, ez_decompress_parts.hip).  The layout's steps run over T emulated threads in the
// kernel's order (every thread counts its streams' parts, thread 0 runs the gate, every thread scans its
// range) and are held to a serial layout written here without the header:
//   the threads' ranges are [0, count) in order, ceil(count / T) streams each, the threads past the end
//   hold [count, count);
//   the gate is open iff in_off[count] >= in_off[0], the extent is within the hint and the batch's parts
//   are within the cap (the records the hint pays for: hint / P + count + 1, none from 2^31 on);
//   open: the gate word is 1, the parts word and base[count] are the batch's parts, at most the cap,
//   base[s] is the parts of the streams before s, and every part g of the batch lies in exactly one
//   stream's [base[s], base[s + 1]) (counted part by part);
//   closed: the gate word, the parts word and base[count] are 0.
// parts_cap itself is held to the same sum in 128 bits around 2^31 and at the ends of 64 bits.
//
// Cases (offsets alone, no bytes; in_off[0] = 5), for parts of P = 16,384 and 65,536 bytes:
//   T = 8 and 0, 1, 2, 7, 8, 9, 16, 17, 23 streams, T = 1,024 and 1,025, 2,049 streams; stream s is
//   lens[(s + r) % 8] bytes long, lens = 0, 1, P - 1, P, P + 1, 2 P, 2^31 - 1, 2^31 (no parts), for every
//   r of 0..7 at T = 8 and r = 0 at T = 1,024; each under the hints: the exact extent, one less, 0, 1,
//   four times the extent, four times with in_off[0] past in_off[count], and under the exact extent with
//   a cap of exactly the batch's parts and of one part fewer.
// Prints "k2_layout ok: N cases".
//
// Build: g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//        -I eazy_amd/csrc -o tools/k2_layout_check tools/k2_layout_check.cpp
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "ez_k2_layout.h"

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

// the rule, serial: the records a hint pays for
static uint64_t cap_rule(uint64_t in_bytes, uint64_t P, uint64_t count) {
    const u128 v = (u128)(in_bytes / P) + (u128)count + 1;
    return v >= ((u128)1 << 31) ? 0 : (uint64_t)v;
}

enum { kCapOfHint = -1 };

// one case: the offsets under a hint; cap: kCapOfHint, or the records the scratch is said to hold
static void run(const std::vector<uint64_t> &off, uint64_t P, int T, uint64_t hint, long long cap_given) {
    const uint64_t count = off.size() - 1;
    g_what = "T " + std::to_string(T) + ", P " + std::to_string(P) + ", count " + std::to_string(count) + ", hint " + std::to_string(hint) + ", cap " +
             std::to_string(cap_given) + ", off";
    for (size_t t = 0; t < off.size() && t < 10; t++) g_what += " " + std::to_string(off[t]);
    // the serial layout
    std::vector<uint64_t> want(count + 1);
    uint64_t total = 0;
    for (uint64_t s = 0; s < count; s++) {
        const uint64_t len = off[s + 1] - off[s];
        want[s] = total;
        total += len >= (1ull << 31) ? 0 : len / P + (len % P != 0);
    }
    want[count] = total;
    const uint64_t cap = cap_given == kCapOfHint ? ez::parts_cap(hint, (uint32_t)P, count) : (uint64_t)cap_given;
    if (cap_given == kCapOfHint) CHECK(cap == cap_rule(hint, P, count));
    const bool open = off[count] >= off[0] && off[count] - off[0] <= hint && total <= cap;

    // the kernel's order over T threads; a word of 0xA5 after each array
    std::vector<uint32_t> base(count + 2, 0xa5a5a5a5u), hdr(ez::kHWords + 1, 0xa5a5a5a5u);
    for (int k = 0; k < ez::kHWords; k++) hdr[(size_t)k] = 0;  // (the launcher's memset)
    std::vector<uint64_t> sums((size_t)T);
    const uint64_t per = count / (uint64_t)T + (count % (uint64_t)T != 0);
    uint64_t next = 0;
    for (int t = 0; t < T; t++) {
        const ez::LayoutRange r = ez::layout_range(count, T, t);
        CHECK(r.lo == next && r.hi >= r.lo && r.hi <= count);
        CHECK(r.hi - r.lo == (count - r.lo < per ? count - r.lo : per));
        next = r.hi;
        uint64_t n = 0;
        for (uint64_t s = r.lo; s < r.hi; s++) {
            base[s] = (uint32_t)(want[s + 1] - want[s]);
            n += base[s];
        }
        sums[(size_t)t] = n;
    }
    CHECK(next == count);
    const bool ok = ez::layout_gate(sums.data(), T, off.data(), count, hint, cap, hdr.data(), base.data());
    for (int t = 0; t < T; t++) ez::layout_scan(base.data(), ez::layout_range(count, T, t), sums[(size_t)t]);

    CHECK(ok == open);
    CHECK(hdr[ez::kHGate] == (open ? 1u : 0u));
    CHECK(hdr[ez::kHParts] == (open ? (uint32_t)total : 0u));
    CHECK(base[count] == (open ? (uint32_t)total : 0u));
    CHECK(base[count + 1] == 0xa5a5a5a5u && hdr[ez::kHWords] == 0xa5a5a5a5u);
    for (int k = 2; k < ez::kHWords; k++) CHECK(hdr[(size_t)k] == 0);
    if (open) {
        CHECK(total <= cap && total < (1ull << 31));
        for (uint64_t s = 0; s <= count; s++) CHECK(base[s] == want[s]);
        // every part of the batch in exactly one stream's range
        std::vector<uint8_t> hits(total, 0);
        for (uint64_t s = 0; s < count; s++) {
            CHECK(base[s] <= base[s + 1] && base[s + 1] <= total);
            for (uint64_t g = base[s]; g < base[s + 1]; g++) hits[g]++;
        }
        for (uint64_t g = 0; g < total; g++) CHECK(hits[g] == 1);
    }
    g_cases++;
}

// count streams of lens[(s + r) % 8] bytes under every hint
static void batch(uint64_t count, uint64_t P, int T, int r) {
    const uint64_t lens[8] = {0, 1, P - 1, P, P + 1, 2 * P, (1ull << 31) - 1, 1ull << 31};
    std::vector<uint64_t> off(count + 1);
    off[0] = 5;
    uint64_t parts = 0;
    for (uint64_t s = 0; s < count; s++) {
        const uint64_t len = lens[(s + (uint64_t)r) % 8];
        off[s + 1] = off[s] + len;
        parts += len >= (1ull << 31) ? 0 : (len + P - 1) / P;
    }
    const uint64_t extent = off[count] - off[0];
    for (uint64_t hint : {extent, extent - 1, (uint64_t)0, (uint64_t)1, 4 * extent}) run(off, P, T, hint, kCapOfHint);
    {  // in_off[0] past in_off[count] (an empty batch has no two offsets: it runs as it is)
        std::vector<uint64_t> down = off;
        if (count) down[0] = off[count] + 1;
        run(down, P, T, 4 * extent, kCapOfHint);
    }
    run(off, P, T, extent, (long long)parts);
    run(off, P, T, extent, parts ? (long long)parts - 1 : 0);
}

int main() {
    for (uint64_t P : {(uint64_t)16384, (uint64_t)65536}) {
        for (uint64_t count : {0, 1, 2, 7, 8, 9, 16, 17, 23})
            for (int r = 0; r < 8; r++) batch(count, P, 8, r);
        for (uint64_t count : {1025, 2049}) batch(count, P, ez::kLayoutThreads, 0);
        // parts_cap around 2^31, all of it from the bytes or from the streams, and at the ends of 64 bits
        for (uint64_t sum : {(1ull << 31) - 2, (1ull << 31) - 1, 1ull << 31, (1ull << 31) + 1}) {
            const uint64_t ins[2][2] = {{(sum - 6) * P + (P - 1), 5}, {0, sum - 1}};
            for (const uint64_t *c : ins) {
                g_what = "parts_cap " + std::to_string(c[0]) + " / " + std::to_string(P) + " + " + std::to_string(c[1]) + " + 1";
                CHECK(ez::parts_cap(c[0], (uint32_t)P, c[1]) == (sum >= (1ull << 31) ? 0 : sum));
                CHECK(ez::parts_cap(c[0], (uint32_t)P, c[1]) == cap_rule(c[0], P, c[1]));
                g_cases++;
            }
        }
        const uint64_t ends[4][2] = {{~0ull, 0}, {0, ~0ull}, {~0ull, ~0ull}, {(1ull << 31) * P, 0}};
        for (const uint64_t *c : ends) {
            g_what = "parts_cap " + std::to_string(c[0]) + ", " + std::to_string(c[1]);
            CHECK(ez::parts_cap(c[0], (uint32_t)P, c[1]) == 0 && cap_rule(c[0], P, c[1]) == 0);
            g_cases++;
        }
    }
    std::printf("k2_layout ok: %llu cases\n", (unsigned long long)g_cases);
    return 0;
}
