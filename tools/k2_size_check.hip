// Host check of K2z's per-lane steps (eazy_amd/csrc/ez_k2_size.h): the same source, compiled for the
// CPU and run over 64 emulated lanes exactly as the kernel runs them (ez_decompress_size.hip: the
// wave's walk of a super-block, sum, reduce, the end checks), for every chunk size, compared per
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
// The builder, the serial walk, the oracle call and the wave's walk of a super-block (emu_walk, the
// mirror of kz_walk) are tools/k2_check_common.h's; here are the kernel's loop over a stream around
// them, the stream lists, and the proof that kz_spec's known-entry form is the super-block's.
#include "k2_check_common.h"

using namespace k2check;

namespace {

struct Counts {
    uint64_t streams, taken, handed_error, handed_design, seam_chunk, seam_super, lit_enter, lit_skip, adversarial, fix_rounds, rewalks, rewalks_adversarial, pad_seam,
        pad_tail, cuts, cuts_taken, cuts_handed_ok, superblocks, passthrough, merged, chunk64, chunk256, chunk1024;
} N;
bool g_adversarial;  // the stream under check is one built to keep speculation off the true chain

// The speculative step as it was before the parts route's form (known, e) took its place, lane 0
// starting at sb and every other lane warming up from the chunk before its own: the reference that
// holds kz_spec / kz_entry / kz_verify with (known = true, e = sb) to the same bitmaps, entries and
// exits on every super-block of every stream here.
template <int C>
uint32_t ref_spec(const ez::KzWin &w, uint32_t sb, int lane, uint32_t nb, uint32_t *bm) {
    using namespace ez;
    uint32_t c0, ce;
    kz_chunk<C>(sb, lane, nb, c0, ce);
    for (int k = 0; k < C / 32; k++) bm[k] = 0;
    if (c0 >= nb) return c0;
    uint32_t p = lane == 0 ? sb : c0 - C;
    while (p < c0) p = kz_next(w, p, nb);
    while (p < ce) {
        bm[(p - c0) >> 5] |= 1u << ((p - c0) & 31);
        p = kz_next(w, p, nb);
    }
    return p;
}
template <int C>
void check_unified(const EmuWave<C> &wv, const ez::KzWin &w, uint32_t sb, uint32_t nb) {
    using namespace ez;
    uint32_t bm[C / 32], prev = 0;
    for (int l = 0; l < kZLanes; l++) {
        const uint32_t sexit = ref_spec<C>(w, sb, l, nb, bm);
        const uint32_t a = l == 0 ? sb : prev;
        const uint32_t x = l == 0 ? sexit : kz_verify<C>(w, sb, l, nb, bm, sexit, a);
        if (sexit != wv.sexit[l] || a != wv.a0[l] || x != wv.x0[l] || std::memcmp(bm, wv.bm[l], sizeof bm) != 0) {
            std::printf("MISMATCH super-block at %u, lane %d (chunk %d): kz_spec with a known entry is not the super-block form\n", sb, l, C);
            std::exit(1);
        }
        prev = sexit;
    }
}

// ---- the kernel's loop over a stream, 64 lanes emulated in order
template <int C>
Result emulate(const uint8_t *in, uint64_t nb64) {
    using namespace ez;
    bool bad = nb64 >= (1ull << 31);
    const uint32_t nb = bad ? 0u : (uint32_t)nb64;
    uint32_t sb = 0, maxd = 0;
    uint64_t total = 0;
    int32_t bsl = -1;
    EmuWave<C> wv(kz_stage_bytes(C));
    EmuStats st{};
    while (!bad && sb < nb) {
        N.superblocks++;
        const KzWin w = emu_walk<C>(wv, in, nb, sb, sb, true, sb, st);
        check_unified<C>(wv, w, sb, nb);
        if (!wv.settled) {
            bad = true;
            break;
        }
        uint64_t run = 0;
        for (int l = 0; l < kZLanes; l++) {
            const KzSum r = kz_sum<C>(w, sb, l, nb, wv.a[l], wv.x[l], 0x7fffffff, 0);
            if ((r.fl & kZBad) || kz_reset_bad(r.fl, total + run)) bad = true;
            if (r.fl & kZReset) bsl = (int32_t)((r.fl >> 8) & 0xff);
            run += r.out;
            maxd = r.maxd > maxd ? r.maxd : maxd;
        }
        total += run;
        if (wv.x[kZLanes - 1] - sb > (uint32_t)kZLanes * C + 65536) N.lit_skip++;
        sb = wv.x[kZLanes - 1];
    }
    if (!bad) bad = !kz_end_ok(sb, nb, total, bsl, maxd);
    N.fix_rounds += st.fix_rounds;
    (g_adversarial ? N.rewalks_adversarial : N.rewalks) += st.rewalks;
    N.passthrough += st.passthrough;
    N.merged += st.merged;
    return Result{!bad, total};
}

// one stream against the oracle, for both chunk sizes; design: it holds a form handed over by design
bool check_one(const std::string &name, const Bytes &s, bool design, bool cut) {
    int64_t olen = 0;
    const int err = oracle(s.data(), s.size(), 0, olen);
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
#define P(f) K2_COUNT(N, 18, f)
    P(streams); P(taken); P(handed_error); P(handed_design); P(seam_chunk); P(seam_super); P(lit_enter); P(lit_skip); P(adversarial);
    P(fix_rounds); P(rewalks); P(rewalks_adversarial); P(pad_seam); P(pad_tail); P(cuts); P(cuts_taken); P(cuts_handed_ok); P(superblocks); P(passthrough); P(merged); P(chunk64); P(chunk256); P(chunk1024);
    std::printf("ok\n");
    return 0;
}
