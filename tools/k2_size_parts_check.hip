// Host check of the steps of K2z's parts route (eazy_amd/csrc/ez_k2_parts.h, with ez_k2_size.h's):
// the same source, compiled for the CPU and run over emulated lanes, parts and streams exactly as the
// kernels order them (ez_decompress_parts.hip: the part layout, a wave per part, then a wave per
// stream over 64 records per load), for chunk 256 and chunk 1,024, compared per stream with the
// oracle's Reader (oracle/eazy_oracle.c, or_decompress) and with one lane's walk of the whole chain
// (kz_serial):
//   a stream the Reader reads to EOF without an error is taken, with the Reader's output length,
//   unless it holds a form the fast parse hands over by design; every other stream is handed over.
//   k2_size_parts_check      prints the count of every class, exits 1 at the first mismatch
//
// Streams (tokens written one by one with the oracle's Encoder), per chunk size, P = 64 chunks:
//  - every header form of the decoders' tests (tests/k2_streams.py _forms) with its first byte at
//    each of the last 8 positions before a part seam;
//  - a literal entered from every lane of the first part that ends inside that part or the next,
//    that spans exactly one whole part, and that spans three whole parts;
//  - literals whose bodies parse as 2-byte copies on the other parity, across part seams, so that a
//    part's record starts off the true chain and the part is walked again (counted);
//  - a literal over a whole part whose body is wide metas, a form the parse hands over: the part's
//    record says so, and the stream is taken all the same (counted);
//  - padding runs of 1 to 40 bytes across part seams;
//  - a MetaReset after output in a later part (handed over by design);
//  - every stream cut at each of its last 27 bytes;
//  - the automatic route's probe (kp_probe_wave) on every stream: both of its answers are counted (a
//    stream it leaves to the wave route gets no parts, and the same result from tools/k2_size_check.hip's walk);
//  - a batch of these streams with empty ones and streams shorter than a chunk between them, laid
//    out and searched as the kernels do.
// The builder, the serial walk, the oracle call and the wave's walk of a part (emu_walk, the mirror of
// kz_walk) are tools/k2_check_common.h's; here are the part's record, the part layout and the in-order
// pass around them, and the stream lists.
#include "k2_check_common.h"

using namespace k2check;

namespace {

struct Counts {
    uint64_t streams, taken, handed_error, handed_design, seam_part, lit_within, lit_one_part, lit_many_parts, adversarial, parts, joined, passed, walked,
        walked_adversarial, unsettled, garbage_bad, garbage_bad_taken, pad_seam, reset_late_part, cuts, cuts_taken, cuts_handed_ok, batch_streams,
        batch_short, batch_parts, probe_wave, probe_parts, chunk256, chunk1024;
} N;
bool g_adversarial;  // the stream under check is one built to keep speculation off the true chain

// ---- the kernels' steps, lanes and parts emulated in order
// part_walk of ez_decompress_parts.hip: one part by 64 lanes
template <int C>
ez::KpRec emu_part(const uint8_t *in, uint32_t nb, uint32_t ps, bool known, uint32_t e) {
    using namespace ez;
    EmuWave<C> wv(kp_stage_bytes(C));
    EmuStats st{};
    const KzWin w = emu_walk<C>(wv, in, nb, kp_stage_base(ps, C), ps, known, e, st);
    if (!wv.settled) {
        N.unsettled++;
        return KpRec{0, kPNoEntry, 0, 0, 0};
    }
    KzSum acc{0, 0, 0};
    for (int l = 0; l < kZLanes; l++) kp_append(acc, kz_sum<C>(w, ps, l, nb, wv.a[l], wv.x[l], 0x7fffffff, 0));
    return KpRec{acc.out, wv.a[0], wv.x[kZLanes - 1], acc.maxd, acc.fl};
}

// kp_layout, kp_first and kp_order over a batch: the records are exactly as many as the layout says (the
// layout here is the serial one; kp_layout's thread steps are tools/k2_layout_check.cpp's to check)
template <int C>
std::vector<Result> emulate(const std::vector<const Bytes *> &ins) {
    using namespace ez;
    const uint64_t count = ins.size();
    std::vector<uint32_t> base(count + 1);
    uint64_t run = 0;
    for (uint64_t s = 0; s < count; s++) {
        base[s] = (uint32_t)run;
        run += kp_parts_of(ins[s]->size(), C);
    }
    base[count] = (uint32_t)run;
    KpRec *recs = (KpRec *)std::malloc(sizeof(KpRec) * (run ? run : 1));
    for (uint32_t g = 0; g < (uint32_t)run; g++) {
        const uint64_t s = kp_stream_of(base.data(), count, g);
        if (!(base[s] <= g && g < base[s + 1])) {
            std::printf("MISMATCH part %u of the batch is not one of stream %llu\n", g, (unsigned long long)s);
            std::exit(1);
        }
        recs[g] = emu_part<C>(ins[s]->data(), (uint32_t)ins[s]->size(), (g - base[s]) * kp_part_bytes(C), false, 0);
        N.parts++;
    }
    std::vector<Result> out;
    for (uint64_t s = 0; s < count; s++) {
        const uint64_t nb64 = ins[s]->size();
        KpState S = kp_start(nb64);
        const uint32_t nb = S.bad ? 0u : (uint32_t)nb64;
        const uint32_t n = base[s + 1] - base[s];
        const KpRec *rs = recs + base[s];
        uint32_t j = 0;
        uint64_t bad_untaken = 0;
        while (!S.bad && j < n) {
            const uint32_t m = n - j < (uint32_t)kZLanes ? n - j : (uint32_t)kZLanes;
            for (uint32_t k = 0; k < m && !S.bad; k++) {
                const uint32_t ps = (j + k) * kp_part_bytes(C);
                const uint32_t pe = nb - ps > kp_part_bytes(C) ? ps + kp_part_bytes(C) : nb;
                KpRec r = rs[j + k];
                const int cls = kp_class(S, pe, r);
                if (cls != kPJoin && (r.fl & kZBad)) bad_untaken++;
                if (cls == kPPass) {
                    N.passed++;
                    continue;
                }
                if (cls == kPWalk) {
                    r = emu_part<C>(ins[s]->data(), nb, ps, true, S.e);
                    (g_adversarial ? N.walked_adversarial : N.walked)++;
                } else {
                    N.joined++;
                }
                kp_take(S, r);
            }
            j += m;
            const uint32_t at = S.e / kp_part_bytes(C);
            j = at > j ? at : j;
        }
        const bool ok = kp_end_ok(S, nb);
        N.garbage_bad += bad_untaken;
        if (ok) N.garbage_bad_taken += bad_untaken;
        out.push_back(Result{ok, S.total});
    }
    std::free(recs);
    return out;
}

std::vector<Bytes> g_kept;  // some of the streams, for the batch at the end

// one stream against the oracle, for both chunk sizes; design: it holds a form handed over by design
bool check_one(const std::string &name, const Bytes &s, bool design, bool cut) {
    int64_t olen = 0;
    const int err = oracle(s.data(), s.size(), 0, olen);
    // (a cut inside a header may still read to EOF without an error, and k2_scan hands it over:
    // tools/k2_size_check.hip, cuts_handed_ok.  The serial walk says which.)
    const Result one = serial(s);
    if (!cut && !s.empty()) {  // the automatic route's probe: which route would size this stream (the result is the same)
        const Padded at(s);
        (ez::kp_probe_wave([&](uint32_t p) { return at(p); }, (uint32_t)s.size()) ? N.probe_wave : N.probe_parts)++;
    }
    const bool want_taken = cut ? one.taken : err == 0 && !design;
    if (cut && !one.taken && err == 0) N.cuts_handed_ok++;
    const std::vector<const Bytes *> ins(1, &s);
    for (int c = 0; c < 2; c++) {
        const Result r = c == 0 ? emulate<256>(ins)[0] : emulate<1024>(ins)[0];
        (c == 0 ? N.chunk256 : N.chunk1024)++;
        if (r.taken != one.taken || (r.taken && r.size != one.size)) {
            std::printf("MISMATCH %s (%zu bytes, chunk %d): serial walk %s size %llu | parts %s size %llu\n", name.c_str(), s.size(), c == 0 ? 256 : 1024,
                        one.taken ? "taken" : "handed over", (unsigned long long)one.size, r.taken ? "taken" : "handed over", (unsigned long long)r.size);
            std::exit(1);
        }
        if (r.taken != want_taken || (r.taken && (err != 0 || r.size != (uint64_t)olen))) {
            std::printf("MISMATCH %s (%zu bytes, chunk %d): oracle err %d len %lld%s | parts %s size %llu\n", name.c_str(), s.size(), c == 0 ? 256 : 1024, err,
                        (long long)olen, design ? " (handed over by design)" : "", r.taken ? "taken" : "handed over", (unsigned long long)r.size);
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
    static uint64_t whole = 0;
    if (whole++ % 7 == 0 && s.size() < (300u << 10)) g_kept.push_back(s);
    for (size_t cut = 1; cut <= 27 && cut <= s.size(); cut++) {
        const Bytes t(s.begin(), s.end() - (long)cut);
        N.cuts++;
        if (check_one(name + " cut " + std::to_string(cut), t, design, true)) N.cuts_taken++;
    }
}

template <int C>
void streams_for_chunk(const std::vector<Form> &fs) {
    const std::string cn = "C" + std::to_string(C) + " ";
    const size_t P = ez::kp_part_bytes(C);
    // the forms before the seam of parts 0 | 1, or 1 | 2 behind a 70,000-byte literal at the start
    for (const Form &f : fs)
        for (int d = 1; d <= 8; d++) {
            Bytes s;
            hdr(s);
            if (f.big_first) lit_rnd(s, 70000);
            fill_to(s, (s.size() / P + 1) * P - (size_t)d);
            put(s, f.b.data(), f.b.size());
            tail3(s);
            fill_to(s, s.size() + 300);
            N.seam_part++;
            check(cn + f.name + " part seam -" + std::to_string(d), s);
        }
    // a literal from every lane of the first part: ending within a part's length, spanning exactly
    // one whole part, spanning three whole parts; then tokens up to the next seam and 3 more
    for (int lane = 0; lane < ez::kZLanes; lane++)
        for (int kind = 0; kind < 3; kind++) {
            Bytes s;
            hdr(s);
            fill_to(s, (size_t)lane * C + 9 + (size_t)(rnd() % (C - 9)));
            const size_t at = s.size();
            const size_t len = kind == 0 ? P / 2 : (kind == 1 ? 2 * P - at + 100 + (size_t)(rnd() % 1000) : 4 * P - at + 100 + (size_t)(rnd() % 1000));
            lit_rnd(s, (int64_t)len);
            fill_to(s, (s.size() / P + 1) * P + 40);
            tail3(s);
            (kind == 0 ? N.lit_within : (kind == 1 ? N.lit_one_part : N.lit_many_parts))++;
            check(cn + "literal kind " + std::to_string(kind) + " from lane " + std::to_string(lane), s);
        }
    // speculation off the true chain across part seams: 258-byte literals at even positions whose
    // bytes at odd positions are copy tags (0x85; the length byte 0x84 of the header too) before a
    // 1-byte offset (0x10), so a chain at an odd position steps 2 bytes and never meets a token start
    for (int parts = 2; parts <= 3; parts++) {
        Bytes s;
        hdr(s);
        s.push_back(0);  // (padding: the first literal at position 10)
        while (s.size() < (size_t)parts * P + 700) {
            tag(s, 0x00, 256);
            for (int q = 0; q < 128; q++) {
                s.push_back(0x10);
                s.push_back(0x85);
            }
        }
        tail3(s);
        N.adversarial++;
        g_adversarial = true;
        check(cn + "copy headers in literal bodies over " + std::to_string(parts) + " parts", s);
        g_adversarial = false;
    }
    // a literal over a whole part whose body is wide Breaks (0x80, 0x1e, 0x00: handed over where the
    // chain meets one): the part's own walk meets them, the true chain never does
    for (int phase = 0; phase < 3; phase++) {
        Bytes s;
        hdr(s);
        fill_to(s, P / 2 + (size_t)phase);
        const size_t len = 2 * P;
        tag(s, 0x00, (int64_t)len);
        static const uint8_t wide_break[3] = {0x80, 0x18 | 6, 0x00};
        for (size_t k = 0; k < len; k++) s.push_back(wide_break[k % 3]);
        fill_to(s, (s.size() / P + 1) * P + 40);
        tail3(s);
        check(cn + "wide metas in a literal body, phase " + std::to_string(phase), s);
    }
    // padding runs of 1 to 40 bytes from d bytes before a part seam
    for (int n = 1; n <= 40; n++) {
        const int ds[3] = {1, (n + 1) / 2, n};
        for (int k = 0; k < 3; k++) {
            Bytes s;
            hdr(s);
            fill_to(s, P - (size_t)ds[k]);
            s.insert(s.end(), (size_t)n, 0);
            tail3(s);
            fill_to(s, s.size() + 200);
            N.pad_seam++;
            check(cn + "pad " + std::to_string(n) + " part seam -" + std::to_string(ds[k]), s);
        }
    }
    {  // a MetaReset after output, in the third part
        Bytes s;
        hdr(s);
        fill_to(s, 2 * P + 300);
        meta(s, 2 << 3, "\x14", 1);
        fill_to(s, s.size() + 300);
        N.reset_late_part++;
        check(cn + "reset after output in a later part", s, true);
    }
}

}  // namespace

int main() {
    g_out.resize(64 << 20);
    const std::vector<Form> fs = forms();
    streams_for_chunk<256>(fs);
    streams_for_chunk<1024>(fs);
    {  // the empty stream, the header alone, forms handed over by design in the first part
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
        const uint8_t wide_break[3] = {0x80, 0x18 | 6, 0x00};
        put(wm, wide_break, 3);
        lit_rnd(wm, 3);
        check("wide meta", wm, true);
    }
    {  // a batch: kept streams with empty ones and ones shorter than a chunk between them
        std::vector<Bytes> shorts;
        for (int k = 0; k < 64; k++) {
            Bytes s;
            if (k % 4) {
                hdr(s);
                fill_to(s, 10 + (size_t)(rnd() % 200));
                if (k % 8 == 5) s.pop_back();  // (some of them cut)
            }
            shorts.push_back(s);
        }
        std::vector<const Bytes *> ins;
        for (size_t k = 0; k < g_kept.size(); k++) {
            ins.push_back(&shorts[k % shorts.size()]);
            ins.push_back(&g_kept[k]);
            if (k % 5 == 0) ins.push_back(&shorts[(k + 1) % shorts.size()]);
        }
        for (int c = 0; c < 2; c++) {
            const uint64_t before = N.parts;
            const std::vector<Result> got = c == 0 ? emulate<256>(ins) : emulate<1024>(ins);
            N.batch_parts += N.parts - before;
            for (size_t s = 0; s < ins.size(); s++) {
                const Result one = serial(*ins[s]);
                if (got[s].taken != one.taken || (one.taken && got[s].size != one.size)) {
                    std::printf("MISMATCH batch stream %zu (%zu bytes, chunk %d)\n", s, ins[s]->size(), c == 0 ? 256 : 1024);
                    return 1;
                }
                N.batch_streams++;
                if (ins[s]->size() < 256) N.batch_short++;
            }
        }
    }
#define P(f) K2_COUNT(N, 20, f)
    P(streams); P(taken); P(handed_error); P(handed_design); P(seam_part); P(lit_within); P(lit_one_part); P(lit_many_parts); P(adversarial);
    P(parts); P(joined); P(passed); P(walked); P(walked_adversarial); P(unsettled); P(garbage_bad); P(garbage_bad_taken); P(pad_seam); P(reset_late_part);
    P(cuts); P(cuts_taken); P(cuts_handed_ok); P(batch_streams); P(batch_short); P(batch_parts); P(probe_wave); P(probe_parts); P(chunk256); P(chunk1024);
    std::printf("ok\n");
    return 0;
}
