// What the host checks of the K2 query family share (k2_size_check, k2_size_parts_check, k2_segs_check;
// k2_parse_check takes rnd() and the count printer only):
//   the stream builder    tokens written one by one with the oracle's Encoder, from one fixed-seed
//                         generator (the order of its rnd() calls is part of every check's counts);
//   forms()               every header form of the decoders' tests (tests/k2_streams.py _forms);
//   Padded, serial()      a single walker over the whole chain (kz_serial);
//   oracle()              the oracle's Reader on a stream (oracle/eazy_oracle.c);
//   emu_walk              the host mirror of kz_walk (eazy_amd/csrc/ez_k2_walk.h): the wave's walk of a
//                         block of 64 chunks, the lanes emulated in order over the same per-lane source.
// The emulated LDS arrays are exactly as long as the kernels' and poisoned past what the kernel
// stages, so a sanitizer build of a check shows a step reading outside them.
#pragma once

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../eazy_amd/csrc/ez_k2_parts.h"
#include "../oracle/eazy_oracle.h"

namespace k2check {

typedef std::vector<uint8_t> Bytes;

// one line of a check's counts: the tests read "name value"
#define K2_COUNT(counts, width, f) std::printf("%-*s %llu\n", width, #f, (unsigned long long)(counts).f)

inline uint64_t g_rng = 0x9e3779b97f4a7c15ull;
inline uint64_t rnd() {  // xorshift64*, fixed seed
    g_rng ^= g_rng >> 12;
    g_rng ^= g_rng << 25;
    g_rng ^= g_rng >> 27;
    return g_rng * 0x2545f4914f6cdd1dull;
}

// ---- the Encoder
inline void put(Bytes &v, const uint8_t *p, size_t n) { v.insert(v.end(), p, p + n); }
inline void put(Bytes &v, const Bytes &b) { v.insert(v.end(), b.begin(), b.end()); }
inline void tag(Bytes &v, int tg, int64_t l) {
    uint8_t t[32];
    size_t n = 0;
    if (or_enc_tag(t, &n, tg, l)) std::exit(2);
    put(v, t, n);
}
inline void offset(Bytes &v, int64_t d, int64_t l) {
    uint8_t t[32];
    size_t n = 0;
    if (or_enc_offset(t, &n, d, l)) std::exit(2);
    put(v, t, n);
}
inline void lit_rnd(Bytes &v, int64_t n) {
    tag(v, 0x00, n);
    for (int64_t k = 0; k < n; k++) v.push_back((uint8_t)rnd());
}
inline void cpy(Bytes &v, int64_t d, int64_t n) {
    tag(v, 0x80, n);
    offset(v, d, n);
}
inline void cpy_long(Bytes &v, int64_t d, int64_t n) {  // the long prefix with a distance that does not need it
    tag(v, 0x80, n);
    v.push_back(0xff);
    offset(v, d, 0);
}
inline void meta(Bytes &v, int64_t m, const char *arg, int n) {
    uint8_t t[32];
    size_t k = 0;
    if (or_enc_meta(t, &k, m, n)) std::exit(2);
    put(v, t, k);
    put(v, (const uint8_t *)arg, (size_t)n);
}
inline void magic(Bytes &v) { meta(v, 0 << 3, "eazy", 4); }
inline void rst(Bytes &v, int bsl = 0x14) {  // 80 10 bsl
    const char a = (char)bsl;
    meta(v, 2 << 3, &a, 1);
}
const uint8_t kHdr[9] = {0x80, 0x02, 'e', 'a', 'z', 'y', 0x80, 0x10, 0x14};  // magic, reset to a 1 MiB window
inline void hdr(Bytes &v, int bsl = 0x14) {
    const size_t at = v.size();
    magic(v);
    rst(v, bsl);
    // (the Encoder's metas are kHdr's nine bytes, but for the window)
    if (v.size() != at + 9 || std::memcmp(v.data() + at, kHdr, 8) != 0 || v[at + 8] != (uint8_t)bsl) std::exit(2);
}

// short literals and copies (distances up to maxd) up to exactly `target` bytes of stream
inline void fill_to(Bytes &v, size_t target, int maxd = 200) {
    while (v.size() < target) {
        const size_t left = target - v.size();
        if (left == 1) {
            v.push_back(0);  // (one byte: padding)
        } else if (left <= 100) {
            lit_rnd(v, (int64_t)left - 1);
        } else if (rnd() % 3 == 0) {
            cpy(v, 1 + (int64_t)(rnd() % maxd), 4 + (int64_t)(rnd() % 60));
        } else {
            lit_rnd(v, 1 + (int64_t)(rnd() % 60));
        }
    }
}
inline void tail3(Bytes &v) {
    lit_rnd(v, 5);
    cpy(v, 3, 9);
    lit_rnd(v, 2);
}

struct Form {
    const char *name;
    Bytes b;
    bool big_first;  // needs a 70,000-byte literal before it
};
inline std::vector<Form> forms() {
    std::vector<Form> f;
    auto add = [&](const char *name, bool big) -> Bytes & {
        f.push_back(Form{name, Bytes(), big});
        return f.back().b;
    };
    lit_rnd(add("lit_len0", false), 50);
    lit_rnd(add("lit_len1", false), 200);
    lit_rnd(add("lit_len2", false), 1000);
    lit_rnd(add("lit_len4", false), 70000);
    cpy(add("cpy_plain", false), 30, 20);
    cpy(add("cpy_off1", false), 320, 20);
    cpy(add("cpy_off2", false), 720, 20);
    cpy(add("cpy_len1_off1", false), 500, 200);
    cpy(add("cpy_len2", false), 510, 500);
    cpy(add("cpy_off4", true), 66044 + 20 + 100, 20);
    cpy(add("cpy_len4_run", false), 1, 70000);
    cpy_long(add("cpy_long", false), 40, 20);
    cpy(add("zero_region", false), 0, 64);
    meta(add("break", false), 3 << 3, "", 0);
    meta(add("ver", false), 1 << 3, "\x00", 1);
    meta(add("magic", false), 0 << 3, "eazy", 4);
    static const int pads[5] = {1, 15, 16, 17, 40};
    static const char *pad_names[5] = {"pad1", "pad15", "pad16", "pad17", "pad40"};
    for (int k = 0; k < 5; k++) add(pad_names[k], false).assign((size_t)pads[k], 0);
    return f;
}

// ---- a single walker: the stream with zeros behind it; at(p) = the 16 bytes at stream position p
struct Padded {
    Bytes z;
    explicit Padded(const Bytes &s) : z(s) { z.insert(z.end(), 32, 0); }
    ez::V16 operator()(uint32_t p) const { return ez::kz_at(ez::KzWin{z.data(), 0}, p); }
};

struct Result {
    bool taken;
    uint64_t size;
};
// The chain walked by one lane from the stream's start to its end (kz_serial, which is also the
// lane-per-stream kernel's walk): the result the chunked walks must reproduce whatever the seams and
// the speculation do.
inline Result serial(const Bytes &s) {
    const Padded at(s);
    uint64_t total = 0;
    const bool ok = ez::kz_serial([&](uint32_t p) { return at(p); }, (uint32_t)s.size(), 0x7fffffff, 0, total);
    return Result{ok, total};
}

// ---- the oracle's Reader on b, with BlockSizeLimit `limit` (0: none): its error (OR_OK on a clean
// end); the output is g_out[0 .. olen).  The check's main sizes g_out.
inline Bytes g_out;
inline int oracle(const uint8_t *b, size_t n, int64_t limit, int64_t &olen) {
    int64_t breaks = 0;
    int err;
    olen = 0;
    if (limit == 0) {
        err = or_decompress(b, (int64_t)n, 1 << 16, g_out.data(), (int64_t)g_out.size(), &olen, &breaks);
    } else {  // or_decompress's loop, with the limit set
        or_reader *r = or_reader_new_bytes(b, (int64_t)n);
        or_reader_set(r, limit, 1 << 16, 0, 0);
        for (;;) {
            int64_t got = 0;
            if ((size_t)olen + (1 << 16) > g_out.size()) std::exit(2);
            err = or_reader_read(r, g_out.data() + olen, 1 << 16, &got);
            olen += got;
            if (err == OR_EBREAK) continue;
            if (err == OR_EOF) err = 0;
            if (err != 0 || got == 0) break;
        }
        or_reader_free(r);
    }
    if (err == OR_ESHORTBUF && (size_t)olen + (1 << 16) > g_out.size()) {
        std::printf("the check's output buffer is too small\n");
        std::exit(2);
    }
    return err;
}

// ---- kz_walk on the host
struct EmuStats {
    uint64_t fix_rounds, rewalks, passthrough, merged;
};

// a wave's LDS and what kz_walk leaves in its lanes
template <int C>
struct EmuWave {
    static constexpr int W = C / 32;
    uint8_t *stage;
    uint32_t (*bm)[W];
    uint32_t sexit[ez::kZLanes], a0[ez::kZLanes], x0[ez::kZLanes];  // every lane's speculative exit; entry and exit before the repair
    uint32_t a[ez::kZLanes], x[ez::kZLanes];                       // entry and exit on the true chain
    bool settled;
    size_t stage_bytes;
    // exactly the kernel's LDS (kz_stage_bytes(C) or kp_stage_bytes(C)): an access outside them is one outside the kernel's
    explicit EmuWave(size_t stage_bytes_) : stage_bytes(stage_bytes_) {
        stage = (uint8_t *)std::malloc(stage_bytes);
        bm = (uint32_t(*)[W])std::malloc(sizeof(uint32_t) * W * ez::kZLanes);
    }
    ~EmuWave() {
        std::free(stage);
        std::free(bm);
    }
    EmuWave(const EmuWave &) = delete;
    EmuWave &operator=(const EmuWave &) = delete;
};

// The block of 64 chunks at ps of the stream in[0 .. nb), staged from sbase on, as kz_walk runs it:
// stage, every lane's kz_spec, kz_entry and kz_verify, then the repair rounds.  Returns the staged
// window for the caller's sum.
template <int C>
ez::KzWin emu_walk(EmuWave<C> &wv, const uint8_t *in, uint32_t nb, uint32_t sbase, uint32_t ps, bool known, uint32_t e, EmuStats &stats) {
    using namespace ez;
    const uint32_t end = ps + (uint32_t)kZLanes * C;
    const uint32_t need = (nb < end ? nb : end) + 16 - sbase;
    std::memset(wv.stage, 0xcc, wv.stage_bytes);  // (what the kernel leaves from earlier: never read)
    for (uint32_t o = 0; o < need; o += 16)
        for (uint32_t k = 0; k < 16; k++) wv.stage[o + k] = sbase + o + k < nb ? in[sbase + o + k] : 0;
    const KzWin w{wv.stage, sbase};
    uint32_t first[kZLanes];
    uint32_t *a = wv.a, *x = wv.x;
    for (int l = 0; l < kZLanes; l++) wv.sexit[l] = kz_spec<C>(w, ps, l, nb, known, e, wv.bm[l], first[l]);
    for (int l = 0; l < kZLanes; l++) a[l] = kz_entry(l, ps, C, known, e, first[l], l ? wv.sexit[l - 1] : 0);
    for (int l = 0; l < kZLanes; l++) {
        x[l] = known && l == 0 ? wv.sexit[l] : kz_verify<C>(w, ps, l, nb, wv.bm[l], wv.sexit[l], a[l]);
        uint32_t c0, ce;
        kz_chunk<C>(ps, l, nb, c0, ce);
        if (l > 0 && a[l] >= ce) stats.passthrough++;
        else if (l > 0 && x[l] == wv.sexit[l]) stats.merged++;
        wv.a0[l] = a[l];
        wv.x0[l] = x[l];
    }
    wv.settled = true;
    for (int round = 0;; round++) {
        int jf = -1;
        for (int l = 1; l < kZLanes && jf < 0; l++)
            if (a[l] != x[l - 1]) jf = l;
        if (jf < 0) break;
        if (round >= kZFixRounds) {
            wv.settled = false;
            break;
        }
        stats.fix_rounds++;
        const uint32_t ex = x[jf - 1];
        for (int l = 0; l < kZLanes; l++)
            if (kz_fix<C>(w, ps, l, nb, wv.bm[l], wv.sexit[l], jf, ex, a[l], x[l])) stats.rewalks++;
    }
    return w;
}

}  // namespace k2check
