// Host check of K2g's per-lane steps (eazy_amd/csrc/ez_k2_segs.h, over ez_k2_size.h's walk): the same
// source, compiled for the CPU and run over 64 emulated lanes as the kernel runs them
// (ez_decompress_segs.hip: the wave's walk of a super-block, kg_sum, then the events in lane order
// through kg_cuts), for every chunk size.  Per stream:
//   the cut list (input position, output position), the stop flag and, without a stop, the output
//   total equal a single lane's walk of the whole chain (kg_serial);
//   the number of cuts is the one the stream was built to have (where the builder knows it);
//   decoding each segment alone with the oracle's Reader and concatenating the results gives the whole
//   stream's bytes, every segment but the last ends without an error, and the last one's error is the
//   whole stream's.
//   k2_segs_check             prints the count of every class, exits 1 at the first mismatch
//   k2_segs_check --dump F    also writes every untruncated stream and its cuts to F (the GPU test's input)
//
// Streams (tokens written one by one with the oracle's Encoder): see main().  The builder, the oracle
// call and the wave's walk of a super-block (emu_walk, the mirror of kz_walk) are
// tools/k2_check_common.h's; here are the events and cuts after it, the stream lists and the dump.
#include <utility>

#include "../eazy_amd/csrc/ez_k2_segs.h"
#include "k2_check_common.h"

using namespace k2check;

namespace {

typedef std::vector<std::pair<uint32_t, uint64_t>> Cuts;

struct Counts {
    uint64_t streams, cuts_found, with_cuts, stops, stops_with_cuts, seam_chunk, seam_super, packed, packed_chunk, empty_segment, header_only,
        metas_cut, pad_cut, break_cut, adversarial, fix_rounds, rewalks, rewalks_adversarial, lit_enter, windows, overflow_stop, zero_reach,
        err_magic, err_ver, err_meta, err_limit, trunc_in_seg, trunc_joined, tail_cuts, oracle_segments, superblocks, events, chunk64, chunk256,
        chunk1024;
} N;
bool g_adversarial;  // the stream under check is one built to keep speculation off the true chain
std::FILE *g_dump;

// ---- the Encoder's forms of this check
void lit_of(Bytes &v, const Bytes &body) {
    tag(v, 0x00, (int64_t)body.size());
    put(v, body);
}
void ver0(Bytes &v) { meta(v, 1 << 3, "\x00", 1); }
void brk(Bytes &v) { meta(v, 3 << 3, "", 0); }
// a segment's tokens, about n bytes of stream
void body(Bytes &v, size_t n, int maxd = 200) { fill_to(v, v.size() + n, maxd); }

// ---- the kernel's loop over a stream, 64 lanes emulated in order
struct Walk {
    Cuts cuts;
    bool stop;
    uint64_t total;
};

template <int C>
Walk emulate(const uint8_t *in, uint64_t nb64, int64_t limit) {
    using namespace ez;
    const int32_t lim32 = k2_lim32(limit);
    const uint32_t nb = nb64 >= (1ull << 31) ? 0u : (uint32_t)nb64;
    Walk wk;
    auto cut = [&](uint32_t i, uint32_t pos, uint64_t out) {
        if (i != wk.cuts.size()) {
            std::printf("cut %u recorded as cut %zu\n", i, wk.cuts.size());
            std::exit(1);
        }
        wk.cuts.push_back(std::make_pair(pos, out));
    };
    KgState st = kg_start();
    uint32_t sb = 0;
    EmuWave<C> wv(kz_stage_bytes(C));
    EmuStats es{};
    while (!st.stop && sb < nb) {
        N.superblocks++;
        const KzWin w = emu_walk<C>(wv, in, nb, sb, sb, true, sb, es);
        if (!wv.settled) {
            st.stop = true;
            break;
        }
        KgSum r[kZLanes];
        for (int l = 0; l < kZLanes; l++) r[l] = kg_sum<C>(w, sb, l, nb, wv.a[l], wv.x[l], lim32, limit);
        for (int l = 0; l < kZLanes && !st.stop; l++) {  // (the kernel: the prefix up to each event, then kg_cuts on every lane)
            st.total += r[l].out;
            st.maxd = r[l].maxd > st.maxd ? r[l].maxd : st.maxd;
            if (r[l].fl == 0) continue;
            N.events++;
            const uint32_t before = st.ncut;
            kg_cuts<C>(w, sb, l, nb, r[l].epos, wv.x[l], lim32, limit, st, cut);
            if (st.ncut - before >= 2) N.packed_chunk++;
        }
        sb = wv.x[kZLanes - 1];
    }
    N.fix_rounds += es.fix_rounds;
    (g_adversarial ? N.rewalks_adversarial : N.rewalks) += es.rewalks;
    wk.stop = st.stop;
    wk.total = st.total;
    return wk;
}

// The same chain walked by one lane from the stream's start to its end.
Walk serial(const Bytes &s, int64_t limit) {
    using namespace ez;
    const Padded at(s);
    Walk wk;
    const KgState st = kg_serial([&](uint32_t p) { return at(p); }, (uint32_t)s.size(), k2_lim32(limit), limit,
                                 [&](uint32_t, uint32_t pos, uint64_t out) { wk.cuts.push_back(std::make_pair(pos, out)); });
    wk.stop = st.stop;
    wk.total = st.total;
    return wk;
}

// the oracle's Reader on b: its output and its error (OR_OK on a clean end)
int oracle(const uint8_t *b, size_t n, int64_t limit, Bytes &out) {
    int64_t olen = 0;
    const int err = k2check::oracle(b, n, limit, olen);
    out.assign(g_out.begin(), g_out.begin() + olen);
    return err;
}

void dump(const std::string &name, const Bytes &s, int64_t limit, const Walk &w) {
    if (!g_dump) return;
    const uint64_t h[5] = {name.size(), (uint64_t)limit, s.size(), w.cuts.size(), w.stop ? 1u : 0u};
    std::fwrite(h, 8, 5, g_dump);
    std::fwrite(name.data(), 1, name.size(), g_dump);
    std::fwrite(s.data(), 1, s.size(), g_dump);
    for (const auto &c : w.cuts) {
        const uint64_t v[2] = {c.first, c.second};
        std::fwrite(v, 8, 2, g_dump);
    }
}

// one stream: the three chunked walks against the serial one, and the segments against the oracle;
// want: the cuts it was built to have (-1: whatever the serial walk finds); returns the cuts
size_t check_one(const std::string &name, const Bytes &s, int64_t limit, int want, bool dumped) {
    const Walk one = serial(s, limit);
    if (want >= 0 && one.cuts.size() != (size_t)want) {
        std::printf("MISMATCH %s (%zu bytes): built to have %d cuts, the serial walk finds %zu\n", name.c_str(), s.size(), want, one.cuts.size());
        std::exit(1);
    }
    for (int c = 0; c < 3; c++) {
        const Walk r = c == 0 ? emulate<64>(s.data(), s.size(), limit) : (c == 1 ? emulate<256>(s.data(), s.size(), limit) : emulate<1024>(s.data(), s.size(), limit));
        (c == 0 ? N.chunk64 : (c == 1 ? N.chunk256 : N.chunk1024))++;
        if (r.cuts != one.cuts || r.stop != one.stop || (!r.stop && r.total != one.total)) {
            std::printf("MISMATCH %s (%zu bytes, chunk %d): serial walk %zu cuts stop %d total %llu | K2g %zu cuts stop %d total %llu\n", name.c_str(),
                        s.size(), c == 0 ? 64 : (c == 1 ? 256 : 1024), one.cuts.size(), (int)one.stop, (unsigned long long)one.total, r.cuts.size(),
                        (int)r.stop, (unsigned long long)r.total);
            for (size_t k = 0; k < one.cuts.size() || k < r.cuts.size(); k++)
                std::printf("  cut %zu: serial (%lld, %lld) | K2g (%lld, %lld)\n", k, k < one.cuts.size() ? (long long)one.cuts[k].first : -1,
                            k < one.cuts.size() ? (long long)one.cuts[k].second : -1, k < r.cuts.size() ? (long long)r.cuts[k].first : -1,
                            k < r.cuts.size() ? (long long)r.cuts[k].second : -1);
            std::exit(1);
        }
    }
    // the segments, each decoded alone
    Bytes whole, part, cat;
    const int werr = oracle(s.data(), s.size(), limit, whole);
    for (size_t g = 0; g <= one.cuts.size(); g++) {
        const size_t i0 = g == 0 ? 0 : one.cuts[g - 1].first, i1 = g == one.cuts.size() ? s.size() : one.cuts[g].first;
        const int err = oracle(s.data() + i0, i1 - i0, limit, part);
        N.oracle_segments++;
        const bool last = g == one.cuts.size();
        if (cat.size() != (g == 0 ? 0 : one.cuts[g - 1].second) || (last ? err != werr : err != 0)) {
            std::printf("MISMATCH %s (%zu bytes): segment %zu of %zu [%zu, %zu): oracle err %d (whole stream %d), output before it %zu, cut says %llu\n",
                        name.c_str(), s.size(), g, one.cuts.size() + 1, i0, i1, err, werr, cat.size(),
                        (unsigned long long)(g == 0 ? 0 : one.cuts[g - 1].second));
            std::exit(1);
        }
        put(cat, part);
    }
    if (cat != whole) {
        std::printf("MISMATCH %s (%zu bytes): the segments' outputs joined (%zu bytes) are not the whole stream's (%zu bytes)\n", name.c_str(), s.size(),
                    cat.size(), whole.size());
        std::exit(1);
    }
    for (size_t g = 1; g < one.cuts.size(); g++)
        if (one.cuts[g].second == one.cuts[g - 1].second) N.empty_segment++;
    N.streams++;
    N.cuts_found += one.cuts.size();
    if (!one.cuts.empty()) N.with_cuts++;
    if (one.stop) N.stops++;
    if (one.stop && !one.cuts.empty()) N.stops_with_cuts++;
    if (dumped) dump(name, s, limit, one);
    return one.cuts.size();
}

// the stream, and the stream cut at each of its last 27 bytes
void check(const std::string &name, const Bytes &s, int want, int64_t limit = 0, bool tails = true) {
    check_one(name, s, limit, want, true);
    for (size_t cut = 1; tails && cut <= 27 && cut <= s.size(); cut++) {
        const Bytes t(s.begin(), s.end() - (long)cut);
        N.tail_cuts++;
        check_one(name + " cut " + std::to_string(cut), t, limit, -1, false);
    }
}

// literal bodies that read as Reset metas (80 10 14 ...) or as whole headers
Bytes resets_body(size_t n, size_t phase) {
    static const uint8_t r[3] = {0x80, 0x10, 0x14};
    Bytes b;
    for (size_t k = 0; k < n; k++) b.push_back(r[(k + phase) % 3]);
    return b;
}
Bytes headers_body(size_t n, size_t phase) {
    Bytes b;
    for (size_t k = 0; k < n; k++) b.push_back(kHdr[(k + phase) % 9]);
    return b;
}

template <int C>
void streams_for_chunk() {
    const std::string cn = "C" + std::to_string(C) + " ";
    // Seams: a late Reset whose tag byte lies at each of the last 8 positions before a chunk seam
    // (chunk 3 | 4) and before a super-block seam, so the 3-byte meta straddles both
    for (int seam = 0; seam < 2; seam++)
        for (int d = 1; d <= 8; d++) {
            Bytes s;
            hdr(s);
            fill_to(s, (size_t)(seam == 0 ? 4 : ez::kZLanes) * C - (size_t)d);
            rst(s);
            tail3(s);
            (seam == 0 ? N.seam_chunk : N.seam_super)++;
            check(cn + (seam == 0 ? "reset chunk seam -" : "reset super-block seam -") + std::to_string(d), s, 1);
        }
    // Packed Resets: 2, 3 and 40 of them with a 1-byte literal after each, from 5 bytes into chunk 1
    for (int n : {2, 3, 40}) {
        Bytes s;
        hdr(s);
        fill_to(s, (size_t)C + 5);
        for (int k = 0; k < n; k++) {
            rst(s);
            lit_rnd(s, 1);
        }
        tail3(s);
        N.packed++;
        check(cn + "packed resets x" + std::to_string(n), s, n);
    }
    // Padding of 1, 15, 16, 17 and 40 bytes before a Reset tag, the run across a chunk seam
    for (int n : {1, 15, 16, 17, 40}) {
        Bytes s;
        hdr(s);
        fill_to(s, (size_t)5 * C - (size_t)(n + 1) / 2);
        s.insert(s.end(), (size_t)n, 0);
        const size_t at = s.size();
        rst(s);
        tail3(s);
        N.pad_cut++;
        check(cn + "pad " + std::to_string(n) + " before a reset", s, 1);
        if (serial(s, 0).cuts[0].first != at) {
            std::printf("MISMATCH %s: the cut is not at the Reset's tag byte\n", (cn + "pad " + std::to_string(n)).c_str());
            std::exit(1);
        }
    }
    // Literals that look like Resets and headers, long enough that whole chunks of speculation start
    // inside them, at every phase; a real Reset between and after them
    for (int kind = 0; kind < 2; kind++)
        for (size_t phase = 0; phase < 3; phase++) {
            Bytes s;
            hdr(s);
            s.push_back(0);
            for (int k = 0; k < 6; k++) {
                lit_of(s, kind == 0 ? resets_body((size_t)3 * C + 1 + (size_t)k, phase + (size_t)k) : headers_body((size_t)3 * C + 2 + (size_t)k, phase * 3 + (size_t)k));
                if (k == 2) rst(s, 0x10);
            }
            rst(s);
            tail3(s);
            N.adversarial++;
            g_adversarial = true;
            check(cn + (kind == 0 ? "resets" : "headers") + " in literal bodies, phase " + std::to_string(phase), s, 2);
            g_adversarial = false;
        }
    // the size check's adversary (literal bodies that parse as 2-byte copies on the other parity, which
    // keep speculation off the true chain for whole chunks), with a Reset after every tenth literal
    {
        Bytes s;
        hdr(s);
        s.push_back(0);  // (padding: the first literal at position 10)
        for (int k = 0; k < 40; k++) {
            tag(s, 0x00, 256);
            for (int q = 0; q < 128; q++) {
                s.push_back(0x10);
                s.push_back(0x85);
            }
            if (k % 10 == 9) {
                rst(s);
                s.push_back(0);  // (the next literal at an even position again)
            }
        }
        tail3(s);
        N.adversarial++;
        g_adversarial = true;
        check(cn + "copy headers in literal bodies, resets between", s, 4);
        g_adversarial = false;
    }
    // Long literal: 70,000 bytes followed by a Reset, entered from every lane
    for (int lane = 0; lane < ez::kZLanes; lane++) {
        Bytes s;
        hdr(s);
        fill_to(s, (size_t)lane * C + 9 + (size_t)(rnd() % (C - 9)));
        lit_rnd(s, 70000);
        rst(s);
        tail3(s);
        N.lit_enter++;
        check(cn + "literal from lane " + std::to_string(lane) + " then a reset", s, 1, 0, false);
    }
}

// four segments with windows of 1 << bsl; what(s, g) writes segment g's tokens after its Reset
template <class F>
Bytes four(int bsl, F what) {
    Bytes s;
    for (int g = 0; g < 4; g++) {
        if (g == 0) hdr(s, bsl);
        else rst(s, bsl);
        what(s, g);
    }
    return s;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 3 && std::strcmp(argv[1], "--dump") == 0) {
        g_dump = std::fopen(argv[2], "wb");
        if (!g_dump) return 2;
    } else if (argc != 1) {
        return 2;
    }
    g_out.resize(16 << 20);
    streams_for_chunk<64>();
    streams_for_chunk<256>();
    streams_for_chunk<1024>();
    {  // packed forms that do not depend on the chunk
        Bytes e;
        check("empty", e, 0);
        Bytes h;
        hdr(h);
        N.header_only++;
        check("header only", h, 0);
        Bytes h2 = h;
        rst(h2, 0x0a);
        N.header_only++;
        check("header and a second reset", h2, 0);
        Bytes a = h2;
        lit_rnd(a, 40);
        cpy(a, 1000, 30);  // (within the second Reset's 1 KiB window)
        check("a reset straight after the header's own is no cut", a, 0);
        Bytes t = h;
        lit_rnd(t, 7);
        rst(t);
        rst(t);
        lit_rnd(t, 3);
        check("two resets with nothing between them", t, 2);
        Bytes n = h;
        lit_rnd(n, 7);
        rst(n);
        check("a reset at the very end", n, 1);
        Bytes nh;
        lit_rnd(nh, 7);
        rst(nh);
        lit_rnd(nh, 7);
        check("output before any reset", nh, 0);
    }
    {  // Magic and Ver metas between the segments; whole headers joined; Break metas either side of a cut
        Bytes s;
        hdr(s);
        body(s, 300);
        magic(s);
        ver0(s);
        rst(s);
        magic(s);
        ver0(s);
        body(s, 300);
        N.metas_cut++;
        check("magic and ver metas around a cut", s, 1);
        Bytes j;
        for (int g = 0; g < 3; g++) {
            hdr(j, 0x10 + g);
            ver0(j);
            body(j, 200 + 100 * (size_t)g);
        }
        N.metas_cut++;
        check("three whole streams joined", j, 2);
        Bytes b;
        hdr(b);
        body(b, 100);
        brk(b);
        rst(b);
        brk(b);
        body(b, 100);
        brk(b);
        N.break_cut++;
        check("break metas on either side of a cut", b, 1);
    }
    {  // Segments that differ
        Bytes s;
        hdr(s, 10);
        body(s, 2000, 1000);
        rst(s, 20);
        body(s, 9000, 200);
        cpy(s, 5000, 40);
        body(s, 500, 4000);
        rst(s, 10);
        body(s, 2000, 1000);
        N.windows++;
        check("a window per segment: 10, 20, 10", s, 2);
        Bytes f;
        hdr(f, 10);
        body(f, 3000, 900);
        rst(f, 20);
        lit_rnd(f, 50);
        cpy(f, 5000, 40);  // fits its own window, not the one before; reaches before its segment's start
        body(f, 300);
        rst(f, 20);
        body(f, 300);
        N.windows++;
        check("a distance that fits its own segment's window only", f, 2);
        Bytes o;
        hdr(o, 20);
        body(o, 9000, 200);
        cpy(o, 5000, 40);
        rst(o, 10);
        lit_rnd(o, 50);
        cpy(o, 5000, 40);  // ErrOverflow: the previous segment's window would have held it
        body(o, 300);
        rst(o, 10);
        body(o, 300);
        N.overflow_stop++;
        check("a distance that fits the previous segment's window only", o, 1);
        Bytes z;
        hdr(z);
        body(z, 500);
        rst(z);
        cpy(z, 100, 20);  // before its segment's start: the zeroed block
        cpy(z, 1, 50);
        lit_rnd(z, 9);
        cpy(z, 300, 40);
        rst(z);
        cpy(z, 0, 64);
        N.zero_reach++;
        check("copies that reach before their segment's start", z, 2);
    }
    // Errors in segment 2 of 4 (segments 0 .. 3): exactly the cuts before it
    for (int kind = 0; kind < 4; kind++) {
        const Bytes s = four(kind == 3 ? 16 : 20, [&](Bytes &v, int g) {
            body(v, 150);
            if (g == 2) {
                if (kind == 0) meta(v, 0 << 3, "eazx", 4);
                else if (kind == 1) meta(v, 1 << 3, "\x01", 1);
                else if (kind == 2) meta(v, 5 << 3, "\x00", 1);
                else lit_rnd(v, 70000);  // (over a BlockSizeLimit of 64 KiB)
            }
            body(v, 150);
        });
        (kind == 0 ? N.err_magic : (kind == 1 ? N.err_ver : (kind == 2 ? N.err_meta : N.err_limit)))++;
        static const char *names[4] = {"bad magic", "ver 1", "an unsupported meta", "a length over BlockSizeLimit"};
        check(std::string(names[kind]) + " in segment 2 of 4", s, 2, kind == 3 ? 65536 : 0);
    }
    {  // BlockSizeLimit below segment 2's window: its Reset is refused, so it is no cut
        Bytes s;
        for (int g = 0; g < 4; g++) {
            if (g == 0) hdr(s, 16);
            else rst(s, g == 2 ? 20 : 16);
            body(s, 300);
        }
        N.err_limit++;
        check("BlockSizeLimit below the window of segment 2 of 4", s, 1, 65536);
    }
    {  // truncation of segment 2 at each of its last 27 bytes: the stream ending there, and segment 3 joined on
        Bytes p[4];
        for (int g = 0; g < 4; g++) {
            if (g == 0) hdr(p[g]);
            else rst(p[g]);
            body(p[g], 200);
            tail3(p[g]);
        }
        for (size_t cut = 1; cut <= 27; cut++) {
            Bytes s = p[0];
            put(s, p[1]);
            s.insert(s.end(), p[2].begin(), p[2].end() - (long)cut);
            N.trunc_in_seg++;
            check_one("segment 2 of 3 cut " + std::to_string(cut), s, 0, 2, true);
            put(s, p[3]);
            N.trunc_joined++;
            const size_t n = check_one("segment 2 of 4 cut " + std::to_string(cut) + ", segment 3 joined on", s, 0, -1, true);
            if (n < 2) {
                std::printf("MISMATCH: the cuts before a truncated segment are lost\n");
                return 1;
            }
        }
    }
    if (g_dump) std::fclose(g_dump);
#define P(f) K2_COUNT(N, 20, f)
    P(streams); P(cuts_found); P(with_cuts); P(stops); P(stops_with_cuts); P(seam_chunk); P(seam_super); P(packed); P(packed_chunk); P(empty_segment);
    P(header_only); P(metas_cut); P(pad_cut); P(break_cut); P(adversarial); P(fix_rounds); P(rewalks); P(rewalks_adversarial); P(lit_enter);
    P(windows); P(overflow_stop); P(zero_reach); P(err_magic); P(err_ver); P(err_meta); P(err_limit); P(trunc_in_seg); P(trunc_joined);
    P(tail_cuts); P(oracle_segments); P(superblocks); P(events); P(chunk64); P(chunk256); P(chunk1024);
    std::printf("ok\n");
    return 0;
}
