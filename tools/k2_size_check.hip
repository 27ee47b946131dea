// Host check of K2z's per-lane steps (eazy_amd/csrc/ez_k2_size.h): the same source, compiled for the
// CPU and run over 64 emulated lanes exactly as the kernel runs them (ez_decompress_size.hip: stage,
// speculate, verify and re-walk, sum, reduce, the end checks), for every chunk size, compared per
// stream with the oracle's Reader (oracle/eazy_oracle.c, or_decompress):
//   a stream the Reader reads to EOF without an error is taken, with the Reader's output length,
//   unless it holds a form the fast parse hands over by design; every other stream is handed over.
//   Every stream's result is also the one a single lane gets walking the whole chain in order.
//   k2_size_check            prints the count of every class, exits 1 at the first mismatch
//   k2_size_check FILE       the chunked walk's counts on the one stream in FILE, per chunk size
//
// Streams (tokens written one by one with the oracle's Encoder):
//  - every header form of the decoders' tests (tests/k2_streams.py _forms) with its first byte at
//    each of the last 8 positions before a chunk seam and before a super-block seam;
//  - a 70,000-byte literal entered from every lane;
//  - literals whose bodies parse as 2-byte copies on the other parity, so that speculation stays off
//    the true chain for whole chunks and the re-walk runs (counted);
//  - padding runs of 1 to 40 bytes across seams and at the stream's end;
//  - forms handed over by design (a MetaReset after output, a wide meta);
//  - every stream cut at each of its last 27 bytes.
// The staged bytes past what the kernel stages are poisoned, and the buffers are exactly as long as
// the kernel's, so a sanitizer build of this program shows a step reading outside them.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../eazy_amd/csrc/ez_k2_size.h"
#include "../oracle/eazy_oracle.h"

namespace {

typedef std::vector<uint8_t> Bytes;

struct Counts {
    uint64_t streams, taken, handed_error, handed_design, seam_chunk, seam_super, lit_enter, lit_skip, adversarial, fix_rounds, rewalks, rewalks_adversarial, pad_seam,
        pad_tail, cuts, cuts_taken, cuts_handed_ok, superblocks, passthrough, merged, chunk64, chunk256, chunk1024;
} N;
bool g_adversarial;  // the stream under check is one built to keep speculation off the true chain

uint64_t g_rng = 0x9e3779b97f4a7c15ull;
uint64_t rnd() {  // xorshift64*, fixed seed
    g_rng ^= g_rng >> 12;
    g_rng ^= g_rng << 25;
    g_rng ^= g_rng >> 27;
    return g_rng * 0x2545f4914f6cdd1dull;
}

// ---- the Encoder
void put(Bytes &v, const uint8_t *p, size_t n) { v.insert(v.end(), p, p + n); }
void tag(Bytes &v, int tg, int64_t l) {
    uint8_t t[32];
    size_t n = 0;
    if (or_enc_tag(t, &n, tg, l)) std::exit(2);
    put(v, t, n);
}
void offset(Bytes &v, int64_t d, int64_t l) {
    uint8_t t[32];
    size_t n = 0;
    if (or_enc_offset(t, &n, d, l)) std::exit(2);
    put(v, t, n);
}
void lit_rnd(Bytes &v, int64_t n) {
    tag(v, 0x00, n);
    for (int64_t k = 0; k < n; k++) v.push_back((uint8_t)rnd());
}
void cpy(Bytes &v, int64_t d, int64_t n) {
    tag(v, 0x80, n);
    offset(v, d, n);
}
void cpy_long(Bytes &v, int64_t d, int64_t n) {  // the long prefix with a distance that does not need it
    tag(v, 0x80, n);
    v.push_back(0xff);
    offset(v, d, 0);
}
void meta(Bytes &v, int64_t m, const char *arg, int n) {
    uint8_t t[32];
    size_t k = 0;
    if (or_enc_meta(t, &k, m, n)) std::exit(2);
    put(v, t, k);
    put(v, (const uint8_t *)arg, (size_t)n);
}
const uint8_t kHdr[9] = {0x80, 0x02, 'e', 'a', 'z', 'y', 0x80, 0x10, 0x14};  // magic, reset to a 1 MiB window
void hdr(Bytes &v) { put(v, kHdr, sizeof kHdr); }

// short literals and copies up to exactly `target` bytes of stream
void fill_to(Bytes &v, size_t target) {
    while (v.size() < target) {
        const size_t left = target - v.size();
        if (left == 1) {
            v.push_back(0);  // (one byte: padding)
        } else if (left <= 100) {
            lit_rnd(v, (int64_t)left - 1);
        } else if (rnd() % 3 == 0) {
            cpy(v, 1 + (int64_t)(rnd() % 200), 4 + (int64_t)(rnd() % 60));
        } else {
            lit_rnd(v, 1 + (int64_t)(rnd() % 60));
        }
    }
}
void tail3(Bytes &v) {
    lit_rnd(v, 5);
    cpy(v, 3, 9);
    lit_rnd(v, 2);
}

struct Form {
    const char *name;
    Bytes b;
    bool big_first;  // needs a 70,000-byte literal before it
};
std::vector<Form> forms() {
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

// ---- the kernel's loop over a stream, 64 lanes emulated in order
struct Result {
    bool taken;
    uint64_t size;
};

template <int C>
Result emulate(const uint8_t *in, uint64_t nb64) {
    using namespace ez;
    constexpr int W = C / 32;
    bool bad = nb64 >= (1ull << 31);
    const uint32_t nb = bad ? 0u : (uint32_t)nb64;
    uint32_t sb = 0, maxd = 0;
    uint64_t total = 0;
    int32_t bsl = -1;
    // exactly the kernel's LDS: an access outside them is one outside the kernel's
    uint8_t *stage = (uint8_t *)std::malloc(kz_stage_bytes(C));
    uint32_t(*bm)[W] = (uint32_t(*)[W])std::malloc(sizeof(uint32_t) * W * kZLanes);
    uint32_t sexit[kZLanes], a[kZLanes], x[kZLanes];
    while (!bad && sb < nb) {
        N.superblocks++;
        const uint32_t need = nb - sb + 16 < kz_stage_bytes(C) ? nb - sb + 16 : kz_stage_bytes(C);
        std::memset(stage, 0xcc, kz_stage_bytes(C));  // (what the kernel leaves from earlier: never read)
        for (uint32_t o = 0; o < need; o += 16)
            for (uint32_t k = 0; k < 16; k++) stage[o + k] = sb + o + k < nb ? in[sb + o + k] : 0;
        const KzWin w{stage, sb};
        for (int l = 0; l < kZLanes; l++) sexit[l] = kz_spec<C>(w, sb, l, nb, bm[l]);
        for (int l = 0; l < kZLanes; l++) a[l] = l == 0 ? sb : sexit[l - 1];
        for (int l = 0; l < kZLanes; l++) {
            x[l] = l == 0 ? sexit[0] : kz_verify<C>(w, sb, l, nb, bm[l], sexit[l], a[l]);
            uint32_t c0, ce;
            kz_chunk<C>(sb, l, nb, c0, ce);
            if (l > 0 && a[l] >= ce) N.passthrough++;
            else if (l > 0 && x[l] == sexit[l]) N.merged++;
        }
        for (int round = 0;; round++) {
            int jf = -1;
            for (int l = 1; l < kZLanes && jf < 0; l++)
                if (a[l] != x[l - 1]) jf = l;
            if (jf < 0) break;
            if (round >= kZFixRounds) {
                bad = true;
                break;
            }
            N.fix_rounds++;
            const uint32_t e = x[jf - 1];
            for (int l = 0; l < kZLanes; l++)
                if (kz_fix<C>(w, sb, l, nb, bm[l], sexit[l], jf, e, a[l], x[l])) (g_adversarial ? N.rewalks_adversarial : N.rewalks)++;
        }
        if (bad) break;
        uint64_t run = 0;
        for (int l = 0; l < kZLanes; l++) {
            const KzSum r = kz_sum<C>(w, sb, l, nb, a[l], x[l], 0x7fffffff, 0);
            if ((r.fl & kZBad) || kz_reset_bad(r.fl, total + run)) bad = true;
            if (r.fl & kZReset) bsl = (int32_t)((r.fl >> 8) & 0xff);
            run += r.out;
            maxd = r.maxd > maxd ? r.maxd : maxd;
        }
        total += run;
        if (x[kZLanes - 1] - sb > (uint32_t)kZLanes * C + 65536) N.lit_skip++;
        sb = x[kZLanes - 1];
    }
    if (!bad) bad = !kz_end_ok(sb, nb, total, bsl, maxd);
    std::free(stage);
    std::free(bm);
    return Result{!bad, total};
}

// The same chain walked by one lane from the stream's start to its end (kz_serial, which is also the
// lane-per-stream kernel's walk): the result the chunked walk must reproduce whatever the seams and
// the speculation do.
Result serial(const Bytes &s) {
    using namespace ez;
    Bytes z(s);
    z.insert(z.end(), 32, 0);
    const KzWin w{z.data(), 0};
    uint64_t total = 0;
    const bool ok = kz_serial([&](uint32_t p) { return kz_at(w, p); }, (uint32_t)s.size(), 0x7fffffff, 0, total);
    return Result{ok, total};
}

Bytes g_out;

// one stream against the oracle, for both chunk sizes; design: it holds a form handed over by design
bool check_one(const std::string &name, const Bytes &s, bool design, bool cut) {
    int64_t olen = 0, breaks = 0;
    const int err = or_decompress(s.data(), (int64_t)s.size(), 1 << 16, g_out.data(), (int64_t)g_out.size(), &olen, &breaks);
    if (err == OR_ESHORTBUF) {
        std::printf("the check's output buffer is too small for %s\n", name.c_str());
        std::exit(2);
    }
    // A stream cut inside a meta or a token's header may still read to EOF without an error (a lone
    // 0x80 at the end: continueMetaTag's short buffer leaves i at the input's end, reader.go:272-280,
    // which Read takes for a clean end); k2_scan hands a step past the input over, so such a cut is
    // handed over although the Reader accepts it (counted: cuts_handed_ok).  The serial walk says which.
    const Result one = serial(s);
    const bool want_taken = cut ? one.taken : err == 0 && !design;
    if (cut && !one.taken && err == 0) N.cuts_handed_ok++;
    for (int c = 0; c < 3; c++) {
        const Result r = c == 0 ? emulate<64>(s.data(), s.size()) : (c == 1 ? emulate<256>(s.data(), s.size()) : emulate<1024>(s.data(), s.size()));
        (c == 0 ? N.chunk64 : (c == 1 ? N.chunk256 : N.chunk1024))++;
        if (r.taken != one.taken || (r.taken && r.size != one.size)) {
            std::printf("MISMATCH %s (%zu bytes, chunk %d): serial walk %s size %llu | K2z %s size %llu\n", name.c_str(), s.size(),
                        c == 0 ? 64 : (c == 1 ? 256 : 1024), one.taken ? "taken" : "handed over", (unsigned long long)one.size,
                        r.taken ? "taken" : "handed over", (unsigned long long)r.size);
            std::exit(1);
        }
        if (r.taken != want_taken || (r.taken && (err != 0 || r.size != (uint64_t)olen))) {
            std::printf("MISMATCH %s (%zu bytes, chunk %d): oracle err %d len %lld%s | K2z %s size %llu\n", name.c_str(), s.size(),
                        c == 0 ? 64 : (c == 1 ? 256 : 1024), err, (long long)olen, design ? " (handed over by design)" : "", r.taken ? "taken" : "handed over",
                        (unsigned long long)r.size);
            std::exit(1);
        }
    }
    N.streams++;
    if (want_taken) N.taken++;
    else if (err != 0) N.handed_error++;
    else N.handed_design++;
    return want_taken;
}

// the stream, and the stream cut at each of its last 27 bytes
void check(const std::string &name, const Bytes &s, bool design = false) {
    check_one(name, s, design, false);
    for (size_t cut = 1; cut <= 27 && cut <= s.size(); cut++) {
        const Bytes t(s.begin(), s.end() - (long)cut);
        N.cuts++;
        if (check_one(name + " cut " + std::to_string(cut), t, design, true)) N.cuts_taken++;
    }
}

template <int C>
void streams_for_chunk(const std::vector<Form> &fs) {
    const std::string cn = "C" + std::to_string(C) + " ";
    // the forms before a chunk seam (chunk 3 | 4 of the super-block) and before a super-block seam;
    // the super-block in question starts at 0, or where the 70,000-byte literal ends (lane 0 leaves
    // its chunk there and the other lanes pass it through)
    for (const Form &f : fs)
        for (int seam = 0; seam < 2; seam++)
            for (int d = 1; d <= 8; d++) {
                Bytes s;
                hdr(s);
                if (f.big_first) lit_rnd(s, 70000);
                const size_t base = f.big_first ? s.size() : 0;
                fill_to(s, base + (size_t)(seam == 0 ? 4 : ez::kZLanes) * C - (size_t)d);
                put(s, f.b.data(), f.b.size());
                tail3(s);
                (seam == 0 ? N.seam_chunk : N.seam_super)++;
                check(cn + f.name + (seam == 0 ? " chunk seam -" : " super-block seam -") + std::to_string(d), s);
            }
    // a 70,000-byte literal entered from every lane, then 3 tokens
    for (int lane = 0; lane < ez::kZLanes; lane++) {
        Bytes s;
        hdr(s);
        fill_to(s, (size_t)lane * C + 9 + (size_t)(rnd() % (C - 9)));
        lit_rnd(s, 70000);
        tail3(s);
        N.lit_enter++;
        check(cn + "literal from lane " + std::to_string(lane), s);
    }
    // speculation off the true chain: 258-byte literals at even positions whose bytes at odd
    // positions are copy tags (0x85; the length byte 0x84 of the header too) before a 1-byte
    // offset (0x10), so a chain at an odd position steps 2 bytes and never meets a token start
    for (int n = 40; n <= 200; n += 160) {
        Bytes s;
        hdr(s);
        s.push_back(0);  // (padding: the first literal at position 10)
        for (int k = 0; k < n; k++) {
            tag(s, 0x00, 256);
            for (int q = 0; q < 128; q++) {
                s.push_back(0x10);
                s.push_back(0x85);
            }
        }
        tail3(s);
        N.adversarial++;
        g_adversarial = true;
        check(cn + "copy headers in literal bodies x" + std::to_string(n), s);
        g_adversarial = false;
    }
    // padding runs of 1 to 40 bytes: from d bytes before a seam, and at the stream's end
    for (int n = 1; n <= 40; n++) {
        const int ds[3] = {1, (n + 1) / 2, n};
        for (int seam = 0; seam < 2; seam++)
            for (int k = 0; k < 3; k++) {
                Bytes s;
                hdr(s);
                fill_to(s, (size_t)(seam == 0 ? 7 : ez::kZLanes) * C - (size_t)ds[k]);
                s.insert(s.end(), (size_t)n, 0);
                tail3(s);
                N.pad_seam++;
                check(cn + "pad " + std::to_string(n) + (seam == 0 ? " chunk seam -" : " super-block seam -") + std::to_string(ds[k]), s);
            }
        Bytes s;
        hdr(s);
        fill_to(s, (size_t)2 * C - 5);
        tail3(s);
        s.insert(s.end(), (size_t)n, 0);
        N.pad_tail++;
        check(cn + "pad " + std::to_string(n) + " at the end", s);
    }
}

}  // namespace

// k2_size_check FILE: the walk's counts on one stream from a file (where a stream's time goes)
int one_file(const char *path) {
    std::FILE *f = std::fopen(path, "rb");
    if (!f) return 2;
    Bytes s;
    uint8_t buf[65536];
    for (size_t n; (n = std::fread(buf, 1, sizeof buf, f)) > 0;) put(s, buf, n);
    std::fclose(f);
    for (int c = 0; c < 3; c++) {
        N = Counts();
        const Result r = c == 0 ? emulate<64>(s.data(), s.size()) : (c == 1 ? emulate<256>(s.data(), s.size()) : emulate<1024>(s.data(), s.size()));
        std::printf("chunk %d: %zu bytes, %s, size %llu: superblocks %llu fix_rounds %llu rewalks %llu passthrough %llu merged %llu\n",
                    c == 0 ? 64 : (c == 1 ? 256 : 1024), s.size(), r.taken ? "taken" : "handed over", (unsigned long long)r.size,
                    (unsigned long long)N.superblocks, (unsigned long long)N.fix_rounds, (unsigned long long)N.rewalks,
                    (unsigned long long)N.passthrough, (unsigned long long)N.merged);
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1) return one_file(argv[1]);
    g_out.resize(64 << 20);
    const std::vector<Form> fs = forms();
    streams_for_chunk<64>(fs);
    streams_for_chunk<256>(fs);
    streams_for_chunk<1024>(fs);
    {  // the empty stream, the header alone, forms handed over by design
        check("empty", Bytes());
        Bytes h;
        hdr(h);
        check("header only", h);
        Bytes r = h;
        lit_rnd(r, 1);
        meta(r, 2 << 3, "\x14", 1);
        lit_rnd(r, 1);
        check("reset after output", r, true);
        Bytes wm = h;
        lit_rnd(wm, 3);
        const uint8_t wide_break[3] = {0x80, 0x18 | 6, 0x00};  // a Break with a wide length of 0
        put(wm, wide_break, 3);
        lit_rnd(wm, 3);
        check("wide meta", wm, true);
    }
#define P(f) std::printf("%-18s %llu\n", #f, (unsigned long long)N.f)
    P(streams); P(taken); P(handed_error); P(handed_design); P(seam_chunk); P(seam_super); P(lit_enter); P(lit_skip); P(adversarial);
    P(fix_rounds); P(rewalks); P(rewalks_adversarial); P(pad_seam); P(pad_tail); P(cuts); P(cuts_taken); P(cuts_handed_ok); P(superblocks); P(passthrough); P(merged); P(chunk64); P(chunk256); P(chunk1024);
    std::printf("ok\n");
    return 0;
}
