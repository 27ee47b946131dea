// Host check of K2b's per-lane steps (eazy_amd/csrc/ez_k2_brk.h, over ez_k2_size.h's walk): the same
// source, compiled for the CPU and run over 64 emulated lanes as the kernel runs them
// (ez_decompress_brk.hip: the wave's walk of a super-block, kb_sum, the in-order prefixes, the events in
// lane order through kb_walk, and the fill pass's second kb_sum with each lane's bases), for every chunk
// size.  Per stream, the chunked walk's verdict (taken, or a stop that sends the stream to the exact
// decoder), Break count, positions and total are compared with two references:
//   kb_serial, a single lane's walk of the whole chain;
//   the oracle's Reader: the byte totals at each OR_EBREAK of a read-to-EOF loop, the final size and
//   error.  A stream the walk takes has the Reader's positions and size and ends without an error.
//   k2_brk_check             prints the count of every class, exits 1 at the first mismatch
//   k2_brk_check --dump F    also writes streams with their limit and the Reader's size, status and
//                            positions to F (the GPU test's input)
//
// Streams (tokens written one by one with the oracle's Encoder): see main().  The builder and the
// wave's walk of a super-block (emu_walk, the mirror of kz_walk) are tools/k2_check_common.h's.
#include "../eazy_amd/csrc/ez_k2_brk.h"
#include "k2_check_common.h"

using namespace k2check;

namespace {

typedef std::vector<uint64_t> Pos;

struct Counts {
    uint64_t streams, breaks_found, with_breaks, taken, stops, seam_chunk, seam_super, first, before_reset, around_reset, packed, packed_chunk,
        empty_message, pad, metas, adversarial, fix_rounds, rewalks, rewalks_adversarial, lit_enter, four_segments, err_magic, err_ver, err_meta,
        err_brklen, err_limit, trunc, lone_80, unlisted, tail_cuts, superblocks, events, chunk64, chunk256, chunk1024;
} N;
bool g_adversarial;  // the stream under check is one built to keep speculation off the true chain
std::FILE *g_dump;

// ---- the Encoder's forms of this check
void lit_of(Bytes &v, const Bytes &body) {
    tag(v, 0x00, (int64_t)body.size());
    put(v, body);
}
void ver0(Bytes &v) { meta(v, 1 << 3, "\x00", 1); }
void brk(Bytes &v) {
    const size_t at = v.size();
    meta(v, 3 << 3, "", 0);
    if (v.size() != at + 2 || v[at] != 0x80 || v[at + 1] != 0x1f) std::exit(2);
}
void body(Bytes &v, size_t n, int maxd = 200) { fill_to(v, v.size() + n, maxd); }

// ---- the kernel's loop over a stream, 64 lanes emulated in order
struct Walk {
    Pos pos;
    bool ok;  // the walk takes the stream (else the exact decoder does)
    uint64_t total;
};

void fail(const char *what) {
    std::printf("MISMATCH: %s\n", what);
    std::exit(1);
}

template <int C>
Walk emulate(const uint8_t *in, uint64_t nb64, int64_t limit) {
    using namespace ez;
    const int32_t lim32 = k2_lim32(limit);
    Walk wk;
    wk.ok = false;
    wk.total = 0;
    if (nb64 >= (1ull << 31)) return wk;
    const uint32_t nb = (uint32_t)nb64;
    auto put_at = [&](uint32_t k, uint64_t out) {  // (the fill pass's store to brk_pos[brk_idx[s] + k]: each entry once)
        if (wk.pos.size() <= k) wk.pos.resize((size_t)k + 1, ~0ull);
        if (wk.pos[k] != ~0ull) fail("a Break position was stored twice");
        wk.pos[k] = out;
    };
    const auto none = [](uint32_t, uint64_t) {};
    KbState st = kb_start();
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
        KbSum r[kZLanes];
        uint64_t io[kZLanes];
        uint32_t ib[kZLanes];
        for (int l = 0; l < kZLanes; l++) {
            r[l] = kb_sum<C>(w, sb, l, nb, wv.a[l], wv.x[l], lim32, limit, none);
            io[l] = (l ? io[l - 1] : 0) + r[l].out;  // (the wave's inclusive prefixes)
            ib[l] = (l ? ib[l - 1] : 0) + r[l].nbrk;
            if (r[l].nbrk >= 2) N.packed_chunk++;
        }
        uint64_t base = 0;
        uint32_t bbase = 0;
        int from = 0;
        auto fill = [&](int to) {
            for (int l = from; l <= to; l++) {
                if (r[l].nbrk == 0) continue;
                const uint64_t ob = st.total + (io[l] - r[l].out - base);
                const uint32_t bb = st.nbrk + (ib[l] - r[l].nbrk - bbase);
                (void)kb_sum<C>(w, sb, l, nb, wv.a[l], wv.x[l], lim32, limit, [&](uint32_t i, uint64_t out) { put_at(bb + i, ob + out); });
            }
        };
        auto maxd_of = [&](int lo, int hi) {
            for (int l = lo; l <= hi; l++) st.maxd = r[l].maxd > st.maxd ? r[l].maxd : st.maxd;
        };
        for (int j = 0; j < kZLanes && !st.stop; j++) {
            if (r[j].fl == 0) continue;
            N.events++;
            fill(j);
            st.total += io[j] - base;
            base = io[j];
            st.nbrk += ib[j] - bbase;
            bbase = ib[j];
            maxd_of(from, j);
            from = j + 1;
            kb_walk<C>(w, sb, j, nb, r[j].epos, wv.x[j], lim32, limit, st, put_at);
        }
        if (st.stop) break;
        fill(kZLanes - 1);
        st.total += io[kZLanes - 1] - base;
        st.nbrk += ib[kZLanes - 1] - bbase;
        maxd_of(from, kZLanes - 1);
        sb = wv.x[kZLanes - 1];
    }
    N.fix_rounds += es.fix_rounds;
    (g_adversarial ? N.rewalks_adversarial : N.rewalks) += es.rewalks;
    wk.ok = kb_end_ok(st, sb, nb);
    wk.total = st.total;
    if (wk.ok) {
        if (wk.pos.size() != st.nbrk) fail("the stores of the fill pass are not the count pass's Breaks");
        for (uint64_t p : wk.pos)
            if (p == ~0ull) fail("a Break position was never stored");
    }
    return wk;
}

// The same chain walked by one lane from the stream's start to its end.
Walk serial(const Bytes &s, int64_t limit) {
    using namespace ez;
    const Padded at(s);
    Walk wk;
    uint32_t end = 0;
    const KbState st = kb_serial([&](uint32_t p) { return at(p); }, (uint32_t)s.size(), k2_lim32(limit), limit,
                                 [&](uint32_t k, uint64_t out) {
                                     if (k != wk.pos.size()) fail("the serial walk numbers its Breaks out of order");
                                     wk.pos.push_back(out);
                                 },
                                 &end);
    wk.ok = kb_end_ok(st, end, (uint32_t)s.size());
    wk.total = st.total;
    return wk;
}

// the oracle's Reader on b, read to EOF: the byte total at every ErrBreak, the final size and error
struct Ref {
    Pos pos;
    uint64_t size;
    int err;
};
Ref reader(const Bytes &s, int64_t limit) {
    Ref ref;
    ref.size = 0;
    or_reader *r = or_reader_new_bytes(s.data(), (int64_t)s.size());
    if (limit != 0) or_reader_set(r, limit, 1 << 16, 0, 0);
    for (;;) {
        int64_t got = 0;
        ref.err = or_reader_read(r, g_out.data(), 1 << 16, &got);
        ref.size += (uint64_t)got;
        if (ref.err == OR_EBREAK) {
            ref.pos.push_back(ref.size);
            continue;
        }
        if (ref.err == OR_EOF) ref.err = 0;
        if (ref.err != 0 || got == 0) break;
    }
    or_reader_free(r);
    return ref;
}

void dump(const std::string &name, const Bytes &s, int64_t limit, const Ref &ref) {
    if (!g_dump) return;
    const uint64_t h[6] = {name.size(), (uint64_t)limit, s.size(), ref.pos.size(), ref.size, (uint64_t)ref.err};
    std::fwrite(h, 8, 6, g_dump);
    std::fwrite(name.data(), 1, name.size(), g_dump);
    std::fwrite(s.data(), 1, s.size(), g_dump);
    std::fwrite(ref.pos.data(), 8, ref.pos.size(), g_dump);
}

void show(const char *who, const Walk &w) {
    std::printf("  %s: taken %d total %llu breaks %zu:", who, (int)w.ok, (unsigned long long)w.total, w.pos.size());
    for (size_t k = 0; k < w.pos.size() && k < 12; k++) std::printf(" %llu", (unsigned long long)w.pos[k]);
    std::printf("\n");
}

// one stream: the three chunked walks against the serial one, and both against the Reader; want: the
// ErrBreaks the Reader is to return (-1: whatever it finds), taken: the walk is to take it (-1: either);
// returns the Reader's result
Ref check_one(const std::string &name, const Bytes &s, int64_t limit, int want, int taken, bool dumped) {
    const Walk one = serial(s, limit);
    const Ref ref = reader(s, limit);
    if (want >= 0 && ref.pos.size() != (size_t)want) {
        std::printf("MISMATCH %s (%zu bytes): built to have %d Breaks, the Reader returns %zu\n", name.c_str(), s.size(), want, ref.pos.size());
        std::exit(1);
    }
    if (taken >= 0 && one.ok != (taken != 0)) {
        std::printf("MISMATCH %s (%zu bytes): built to be %s, the serial walk says taken %d\n", name.c_str(), s.size(),
                    taken ? "taken" : "handed over", (int)one.ok);
        std::exit(1);
    }
    if (one.ok && (ref.err != 0 || ref.size != one.total || ref.pos != one.pos)) {
        std::printf("MISMATCH %s (%zu bytes): the Reader ends with error %d, size %llu, %zu Breaks\n", name.c_str(), s.size(), ref.err,
                    (unsigned long long)ref.size, ref.pos.size());
        show("serial walk", one);
        std::exit(1);
    }
    for (int c = 0; c < 3; c++) {
        const Walk r = c == 0 ? emulate<64>(s.data(), s.size(), limit) : (c == 1 ? emulate<256>(s.data(), s.size(), limit) : emulate<1024>(s.data(), s.size(), limit));
        (c == 0 ? N.chunk64 : (c == 1 ? N.chunk256 : N.chunk1024))++;
        if (r.ok != one.ok || (r.ok && (r.pos != one.pos || r.total != one.total))) {
            std::printf("MISMATCH %s (%zu bytes, chunk %d)\n", name.c_str(), s.size(), c == 0 ? 64 : (c == 1 ? 256 : 1024));
            show("serial walk", one);
            show("K2b", r);
            std::exit(1);
        }
    }
    for (size_t k = 1; k < ref.pos.size(); k++) {
        if (ref.pos[k] < ref.pos[k - 1]) fail("the Reader's positions decrease");
        if (ref.pos[k] == ref.pos[k - 1]) N.empty_message++;
    }
    N.streams++;
    N.breaks_found += ref.pos.size();
    if (!ref.pos.empty()) N.with_breaks++;
    (one.ok ? N.taken : N.stops)++;
    if (dumped) dump(name, s, limit, ref);
    return ref;
}

// the stream, and the stream cut at each of its last 27 bytes (those are not dumped)
void check(const std::string &name, const Bytes &s, int want, int64_t limit = 0, bool tails = true, int taken = 1) {
    check_one(name, s, limit, want, taken, true);
    for (size_t cut = 1; tails && cut <= 27 && cut <= s.size(); cut++) {
        const Bytes t(s.begin(), s.end() - (long)cut);
        N.tail_cuts++;
        check_one(name + " cut " + std::to_string(cut), t, limit, -1, -1, false);
    }
}

Bytes cycle_body(const uint8_t *pat, size_t np, size_t n, size_t phase) {
    Bytes b;
    for (size_t k = 0; k < n; k++) b.push_back(pat[(k + phase) % np]);
    return b;
}

template <int C>
void streams_for_chunk() {
    const std::string cn = "C" + std::to_string(C) + " ";
    // Seams: a Break whose tag byte lies at each of the last 8 positions before a chunk seam (chunk 3 | 4)
    // and before a super-block seam (at -1 the two bytes straddle it), output before and after it
    for (int seam = 0; seam < 2; seam++)
        for (int d = 1; d <= 8; d++) {
            Bytes s;
            hdr(s);
            fill_to(s, (size_t)(seam == 0 ? 4 : ez::kZLanes) * C - (size_t)d);
            brk(s);
            tail3(s);
            brk(s);
            (seam == 0 ? N.seam_chunk : N.seam_super)++;
            check(cn + (seam == 0 ? "break chunk seam -" : "break super-block seam -") + std::to_string(d), s, 2);
        }
    // Packed Breaks: 2, 3 and 5,000 back to back from 5 bytes into chunk 1 (5,000: more Breaks in a chunk
    // than a chunk has lanes' worth of anything, over several super-blocks at the small chunks)
    for (int n : {2, 3, 5000}) {
        Bytes s;
        hdr(s);
        fill_to(s, (size_t)C + 5);
        for (int k = 0; k < n; k++) brk(s);
        tail3(s);
        brk(s);
        N.packed++;
        check(cn + "packed breaks x" + std::to_string(n), s, n + 1, 0, n != 5000);
    }
    // Padding of 1, 15, 16, 17 and 40 bytes before and after a Break, the run across a chunk seam
    for (int n : {1, 15, 16, 17, 40}) {
        Bytes s;
        hdr(s);
        fill_to(s, (size_t)5 * C - (size_t)(n + 1) / 2);
        s.insert(s.end(), (size_t)n, 0);
        brk(s);
        s.insert(s.end(), (size_t)n, 0);
        brk(s);
        tail3(s);
        s.insert(s.end(), (size_t)n, 0);
        N.pad++;
        check(cn + "pad " + std::to_string(n) + " around breaks", s, 2);
    }
    // Literals made of Breaks (80 1f), of Resets (80 10 14) and of whole headers, long enough that whole
    // chunks of speculation start inside them, at every phase; real Breaks between and after them
    for (int kind = 0; kind < 3; kind++)
        for (size_t phase = 0; phase < 3; phase++) {
            static const uint8_t kb[2] = {0x80, 0x1f}, kr[3] = {0x80, 0x10, 0x14};
            Bytes s;
            hdr(s);
            s.push_back(0);
            for (int k = 0; k < 6; k++) {
                const size_t n = (size_t)3 * C + 1 + (size_t)k;
                lit_of(s, kind == 0 ? cycle_body(kb, 2, n, phase + (size_t)k) : (kind == 1 ? cycle_body(kr, 3, n, phase + (size_t)k) : cycle_body(kHdr, 9, n, phase * 3 + (size_t)k)));
                if (k % 2 == 1) brk(s);
            }
            brk(s);
            tail3(s);
            N.adversarial++;
            g_adversarial = true;
            check(cn + (kind == 0 ? "breaks" : (kind == 1 ? "resets" : "headers")) + " in literal bodies, phase " + std::to_string(phase), s, 4);
            g_adversarial = false;
        }
    // the size check's adversary (literal bodies that parse as 2-byte copies on the other parity, which
    // keep speculation off the true chain for whole chunks), with a Break after every tenth literal
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
            if (k % 10 == 9) brk(s);  // (two bytes: the next literal at an even position again)
        }
        tail3(s);
        N.adversarial++;
        g_adversarial = true;
        check(cn + "copy headers in literal bodies, breaks between", s, 4);
        g_adversarial = false;
    }
    // Long literal: 70,000 bytes followed by a Break, entered from every lane
    for (int lane = 0; lane < ez::kZLanes; lane++) {
        Bytes s;
        hdr(s);
        fill_to(s, (size_t)lane * C + 9 + (size_t)(rnd() % (C - 9)));
        lit_rnd(s, 70000);
        brk(s);
        tail3(s);
        N.lit_enter++;
        check(cn + "literal from lane " + std::to_string(lane) + " then a break", s, 1, 0, false);
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
    g_out.resize(1 << 16);
    streams_for_chunk<64>();
    streams_for_chunk<256>();
    streams_for_chunk<1024>();
    {  // forms that do not depend on the chunk
        Bytes e;
        check("empty", e, 0);
        Bytes o;
        brk(o);
        N.first++;
        check("a break and nothing else", o, 1);
        Bytes h;
        hdr(h);
        check("header only", h, 0);
        Bytes f = h;
        brk(f);
        lit_rnd(f, 40);
        brk(f);
        N.first++;
        if (check_one("a break before any output", f, 0, 2, 1, true).pos[0] != 0) fail("a Break before any output is not at 0");
        Bytes b;  // before the magic, between the magic and the header's Reset
        brk(b);
        magic(b);
        brk(b);
        rst(b);
        lit_rnd(b, 7);
        brk(b);
        N.before_reset++;
        const Ref rb = check_one("breaks before the header's reset", b, 0, 3, 1, true);
        if (rb.pos[0] != 0 || rb.pos[1] != 0 || rb.pos[2] != 7) fail("Breaks before the header's Reset are not at 0");
        Bytes a = h;  // right before and right after a Reset that follows output: the total goes on across it
        lit_rnd(a, 30);
        brk(a);
        rst(a);
        brk(a);
        lit_rnd(a, 12);
        cpy(a, 5, 9);
        brk(a);
        rst(a, 0x0a);
        rst(a);
        brk(a);
        N.around_reset++;
        const Ref ra = check_one("breaks on either side of a reset after output", a, 0, 4, 1, true);
        if (ra.pos[0] != 30 || ra.pos[1] != 30 || ra.pos[2] != 51 || ra.pos[3] != 51) fail("the total does not go on across a Reset");
        for (size_t cut = 1; cut <= 27; cut++) {
            N.tail_cuts++;
            check_one("breaks on either side of a reset after output cut " + std::to_string(cut), Bytes(a.begin(), a.end() - (long)cut), 0, -1, -1, false);
        }
    }
    {  // Magic and Ver metas with Breaks around them
        Bytes s;
        hdr(s);
        body(s, 300);
        brk(s);
        magic(s);
        brk(s);
        ver0(s);
        brk(s);
        body(s, 300);
        magic(s);
        ver0(s);
        brk(s);
        N.metas++;
        check("breaks around magic and ver metas", s, 4);
    }
    {  // Streams of 4 segments with Breaks in each, windows of their own
        for (int bsl : {10, 20}) {
            const Bytes s = four(bsl, [&](Bytes &v, int g) {
                for (int k = 0; k <= g; k++) {
                    body(v, 150, 900);
                    brk(v);
                }
                if (g == 2) brk(v);
            });
            N.four_segments++;
            check("four segments with breaks in each, window " + std::to_string(bsl), s, 1 + 2 + 4 + 4);
        }
        Bytes o;  // a distance only the previous segment's window holds: ErrOverflow, the exact decoder's
        hdr(o, 20);
        body(o, 9000, 200);
        brk(o);
        cpy(o, 5000, 40);
        rst(o, 10);
        lit_rnd(o, 50);
        brk(o);
        cpy(o, 5000, 40);
        brk(o);
        N.unlisted++;
        check("a break behind a distance over its segment's window", o, 2, 0, false, 0);
    }
    // An error in the middle, Breaks before it (3) and after it (2): those after are not listed
    for (int kind = 0; kind < 5; kind++) {
        Bytes s;
        hdr(s, kind == 4 ? 16 : 20);
        for (int k = 0; k < 3; k++) {
            body(s, 150);
            brk(s);
        }
        if (kind == 0) meta(s, 0 << 3, "eazx", 4);
        else if (kind == 1) meta(s, 1 << 3, "\x01", 1);
        else if (kind == 2) meta(s, 5 << 3, "\x00", 1);
        else if (kind == 3) meta(s, 3 << 3, "\x07", 1);  // 80 18 xx: a Break with a length
        else lit_rnd(s, 70000);                           // (over a BlockSizeLimit of 64 KiB)
        if (kind == 3 && (s[s.size() - 3] != 0x80 || s[s.size() - 2] != 0x18)) return 2;
        for (int k = 0; k < 2; k++) {
            body(s, 150);
            brk(s);
        }
        (kind == 0 ? N.err_magic : (kind == 1 ? N.err_ver : (kind == 2 ? N.err_meta : (kind == 3 ? N.err_brklen : N.err_limit))))++;
        N.unlisted++;
        static const char *names[5] = {"bad magic", "ver 1", "an unsupported meta", "a break with a length", "a length over BlockSizeLimit"};
        const Ref r = check_one(std::string(names[kind]) + " between breaks", s, kind == 4 ? 65536 : 0, 3, 0, true);
        static const int errs[5] = {OR_EBADMAGIC, OR_EUNSUPVER, OR_EUNSUPMETA, OR_EUNSUPMETA, OR_EBLOCKLIMIT};
        if (r.err != errs[kind]) fail("the Reader's error is not the one the stream was built to have");
    }
    {  // truncation at each of the last 27 bytes of a stream that ends in Breaks (cut 1: a lone trailing 0x80)
        Bytes s;
        hdr(s);
        for (int k = 0; k < 3; k++) {
            body(s, 60);
            brk(s);
        }
        lit_rnd(s, 9);
        cpy(s, 300, 20);
        brk(s);
        lit_rnd(s, 3);
        brk(s);
        brk(s);
        for (size_t cut = 0; cut <= 27; cut++) {
            const Bytes t(s.begin(), s.end() - (long)cut);
            if (cut) N.trunc++;
            const Ref r = check_one("a stream that ends in breaks cut " + std::to_string(cut), t, 0, -1, cut == 0 ? 1 : -1, true);
            if (cut == 1) {
                // (the Reader consumes a meta's first byte before it finds the input short, reader.go:276-279: whatever
                // it makes of the end, the walk hands the stream over and the five whole Breaks stand)
                if (t.back() != 0x80 || r.pos.size() != 5 || serial(t, 0).ok) fail("a lone trailing 0x80 behind 5 Breaks is not the exact decoder's");
                N.lone_80++;
            }
        }
    }
    if (g_dump) std::fclose(g_dump);
#define P(f) K2_COUNT(N, 20, f)
    P(streams); P(breaks_found); P(with_breaks); P(taken); P(stops); P(seam_chunk); P(seam_super); P(first); P(before_reset); P(around_reset);
    P(packed); P(packed_chunk); P(empty_message); P(pad); P(metas); P(adversarial); P(fix_rounds); P(rewalks); P(rewalks_adversarial);
    P(lit_enter); P(four_segments); P(err_magic); P(err_ver); P(err_meta); P(err_brklen); P(err_limit); P(trunc); P(lone_80); P(unlisted);
    P(tail_cuts); P(superblocks); P(events); P(chunk64); P(chunk256); P(chunk1024);
    std::printf("ok\n");
    return 0;
}
