// Host check of the steps of K2b's parts route (eazy_amd/csrc/ez_k2_brk_parts.h, over ez_k2_parts.h's
// grid, ez_k2_segs_parts.h's record, ez_k2_brk.h's state and ez_k2_size.h's walk): the same source,
// compiled for the CPU and run over emulated lanes, parts and streams exactly as the kernels order them
// (ez_decompress_brk_parts.hip: the part layout, a wave per part whose lanes' sums are joined as a
// tree, a wave per stream over 64 records per load that leaves every part's entry state and the
// stream's verdict, then a wave per part that stores the part's Break positions from its entry state;
// emu_block is the mirror of kb_block, ez_k2_brk_walk.h), for chunk 256 and chunk 1,024.  Per stream:
//   the verdict (taken, or handed whole to the exact decoder), and for a taken stream the Break count,
//   the total and every position, equal a single lane's walk of the whole chain (kb_serial, kb_end_ok);
//   every position is stored exactly once, and only the parts whose true chain holds a Break are
//   walked by the fill;
//   a stream the route takes has the oracle Reader's ErrBreak positions, size and clean end.
//   k2_brk_parts_check             prints the count of every class, exits 1 at the first mismatch
//   k2_brk_parts_check --dump F    also writes every untruncated stream to F with the Reader's size,
//                                  status and positions and, per chunk size, whether the route takes
//                                  it, its parts and its parts that hold a Break (the GPU test's input)
//
// Streams (tokens written one by one with the oracle's Encoder) of 2 to 6 parts, P = 64 chunks: see
// streams_for_chunk() and main().  The builder, the oracle and the wave's walk of a part (emu_walk, the
// mirror of kz_walk) are tools/k2_check_common.h's.
#include <set>

#include "../eazy_amd/csrc/ez_k2_brk_parts.h"
#include "k2_check_common.h"

using namespace k2check;

namespace {

typedef std::vector<uint64_t> Pos;

struct Counts {
    uint64_t streams, breaks_found, taken, stops, parts, joined, passed, again, again_adversarial, again_entry, again_marked, walk_marked, filled,
        fill_skipped, fill_handed, dead_parts, seam_before, seam_after, many_breaks, straddle, first_output, behind_reset, around_reset_seam, spanned,
        adversarial, far_window_stop, handover_late, err_mid, tail_cuts, batch_streams, batch_short, batch_empty, unsettled, chunk256, chunk1024;
} N;
bool g_adversarial;  // the stream under check is one built to keep speculation off the true chain
std::FILE *g_dump;

void fail(const char *what) {
    std::printf("MISMATCH: %s\n", what);
    std::exit(1);
}

// ---- the Encoder's forms of this check
void lit_of(Bytes &v, const Bytes &body) {
    tag(v, 0x00, (int64_t)body.size());
    put(v, body);
}
void brk(Bytes &v) {
    const size_t at = v.size();
    meta(v, 3 << 3, "", 0);
    if (v.size() != at + 2 || v[at] != 0x80 || v[at + 1] != 0x1f) std::exit(2);
}
void body(Bytes &v, size_t n, int maxd = 200) { fill_to(v, v.size() + n, maxd); }
Bytes cycle_body(const uint8_t *pat, size_t np, size_t n, size_t phase) {
    Bytes b;
    for (size_t k = 0; k < n; k++) b.push_back(pat[(k + phase) % np]);
    return b;
}

struct Walk {
    Pos pos;
    bool ok;  // the route takes the stream (else the exact decoder does)
    uint64_t total;
    uint32_t parts, holds;  // its parts, and those whose true chain holds a Break (the fill's)
};

// ---- the kernels' steps, lanes and parts emulated in order
// part_rec of ez_decompress_brk_parts.hip: one part by 64 lanes, their sums joined as the kernel's tree
template <int C>
ez::KqRec emu_rec(const uint8_t *in, uint32_t nb, uint32_t ps, int32_t lim32, int64_t limit) {
    using namespace ez;
    EmuWave<C> wv(kp_stage_bytes(C));
    EmuStats st{};
    const KzWin w = emu_walk<C>(wv, in, nb, kp_stage_base(ps, C), ps, false, 0, st);
    if (!wv.settled) {
        N.unsettled++;
        return kq_rec_unsettled();
    }
    KqSum r[kZLanes];
    for (int l = 0; l < kZLanes; l++) r[l] = kq_sum<C>(w, ps, l, nb, wv.a[l], wv.x[l], lim32, limit);
    for (int d = 1; d < kZLanes; d <<= 1)
        for (int l = 0; l < kZLanes; l += 2 * d) kq_append(r[l], r[l + d]);
    return kq_rec(r[0], wv.a[0], wv.x[kZLanes - 1]);
}

// kb_block: the part at ps from the true position e, with the state; fill_on: the filling body
template <int C, class Put>
uint32_t emu_block(const uint8_t *in, uint32_t nb, uint32_t ps, uint32_t e, int32_t lim32, int64_t limit, ez::KbState &st, bool fill_on, Put put) {
    using namespace ez;
    EmuWave<C> wv(kp_stage_bytes(C));
    EmuStats es{};
    const KzWin w = emu_walk<C>(wv, in, nb, kp_stage_base(ps, C), ps, true, e, es);
    if (!wv.settled) {
        N.unsettled++;
        st.stop = true;
        return e;
    }
    const auto none = [](uint32_t, uint64_t) {};
    const auto put0 = [&](uint32_t k, uint64_t out) {
        if (fill_on) put(k, out);
    };
    KbSum r[kZLanes];
    uint64_t io[kZLanes];
    uint32_t ib[kZLanes];
    for (int l = 0; l < kZLanes; l++) {
        r[l] = kb_sum<C>(w, ps, l, nb, wv.a[l], wv.x[l], lim32, limit, none);
        io[l] = (l ? io[l - 1] : 0) + r[l].out;  // (the wave's inclusive prefixes)
        ib[l] = (l ? ib[l - 1] : 0) + r[l].nbrk;
    }
    uint64_t base = 0;
    uint32_t bbase = 0;
    int from = 0;
    auto fill = [&](int to) {
        for (int l = from; fill_on && l <= to; l++) {
            if (r[l].nbrk == 0) continue;
            const uint64_t ob = st.total + (io[l] - r[l].out - base);
            const uint32_t bb = st.nbrk + (ib[l] - r[l].nbrk - bbase);
            (void)kb_sum<C>(w, ps, l, nb, wv.a[l], wv.x[l], lim32, limit, [&](uint32_t i, uint64_t out) { put(bb + i, ob + out); });
        }
    };
    auto maxd_of = [&](int lo, int hi) {
        for (int l = lo; l <= hi; l++) st.maxd = r[l].maxd > st.maxd ? r[l].maxd : st.maxd;
    };
    for (int j = 0; j < kZLanes; j++) {
        if (r[j].fl == 0) continue;
        fill(j);
        st.total += io[j] - base;
        base = io[j];
        st.nbrk += ib[j] - bbase;
        bbase = ib[j];
        maxd_of(from, j);
        from = j + 1;
        kb_walk<C>(w, ps, j, nb, r[j].epos, wv.x[j], lim32, limit, st, put0);
        if (st.stop) return e;
    }
    fill(kZLanes - 1);
    st.total += io[kZLanes - 1] - base;
    st.nbrk += ib[kZLanes - 1] - bbase;
    maxd_of(from, kZLanes - 1);
    return wv.x[kZLanes - 1];
}

// kp_layout (the serial layout; its thread steps are tools/k2_layout_check.cpp's to check), kq_first,
// kq_order and kq_fill over a batch; a stream without parts is the wave route's
// (tools/k2_brk_check.hip holds that one to the same serial walk: here it is the serial walk itself)
Walk serial(const Bytes &s, int64_t limit, uint32_t P);
template <int C>
std::vector<Walk> emulate(const std::vector<const Bytes *> &ins, int64_t limit) {
    using namespace ez;
    const int32_t lim32 = k2_lim32(limit);
    const uint64_t count = ins.size();
    constexpr uint32_t P = kp_part_bytes(C);
    std::vector<uint32_t> base(count + 1), handed(count, 0xa5a5a5a5u);
    uint64_t run = 0;
    for (uint64_t s = 0; s < count; s++) {
        base[s] = (uint32_t)run;
        run += kp_parts_of(ins[s]->size(), C);
    }
    base[count] = (uint32_t)run;
    // (dirty scratch: what the kernels find there must not matter)
    KqRec *recs = (KqRec *)std::malloc(sizeof(KqRec) * (run ? run : 1));
    KqEnt *ents = (KqEnt *)std::malloc(sizeof(KqEnt) * (run ? run : 1));
    std::memset(recs, 0xa5, sizeof(KqRec) * (run ? run : 1));
    std::memset(ents, 0xa5, sizeof(KqEnt) * (run ? run : 1));
    for (uint32_t g = 0; g < (uint32_t)run; g++) {  // the first pass: a wave per part
        const uint64_t s = kp_stream_of(base.data(), count, g);
        if (!(base[s] <= g && g < base[s + 1])) fail("a part of the batch is not one of the stream the search finds");
        recs[g] = emu_rec<C>(ins[s]->data(), (uint32_t)ins[s]->size(), (g - base[s]) * P, lim32, limit);
        if (recs[g].r.fl & kSWalk) N.walk_marked++;
        N.parts++;
    }
    std::vector<Walk> out(count);
    for (uint64_t s = 0; s < count; s++) {  // the order pass: a wave per stream
        const uint32_t n = base[s + 1] - base[s];
        if (n == 0) {
            out[s] = serial(*ins[s], limit, P);
            continue;
        }
        const uint32_t nb = (uint32_t)ins[s]->size();
        const uint8_t *b = ins[s]->data();
        const KqRec *rs = recs + base[s];
        KqEnt *es = ents + base[s];
        KqState S = kq_start();
        uint32_t j = 0;
        while (j < n) {
            if (S.st.stop || S.e >= nb) {
                for (uint32_t q = j; q < n; q++) es[q] = kq_ent(S, false, false), N.dead_parts++;
                break;
            }
            const uint32_t at = S.e / P;
            if (at > j) {
                const uint32_t to = at < n ? at : n;
                for (uint32_t q = j; q < to; q++) es[q] = kq_ent(S, false, false), N.passed++;
                j = to;
                continue;
            }
            const uint32_t m = n - j < (uint32_t)kZLanes ? n - j : (uint32_t)kZLanes;
            uint32_t k = 0;
            for (; k < m && !S.st.stop; k++) {
                const uint32_t ps = (j + k) * P;
                const uint32_t pe = nb - ps > P ? ps + P : nb;
                const KqRec r = rs[j + k];
                const int cls = kq_class(S, pe, r);
                const KqState in = S;
                if (cls == kSPass) {
                    N.passed++;
                } else if (cls == kSAgain) {
                    const uint32_t x = emu_block<C>(b, nb, ps, S.e, lim32, limit, S.st, false, [](uint32_t, uint64_t) {});
                    if (!S.st.stop) S.e = x;
                    (g_adversarial ? N.again_adversarial : N.again)++;
                    (r.r.ent != in.e ? N.again_entry : N.again_marked)++;
                } else {
                    kq_take(S, r);
                    N.joined++;
                }
                es[j + k] = kq_ent(in, cls != kSPass, S.st.nbrk != in.st.nbrk);
            }
            j += k;
        }
        Walk &wk = out[s];
        wk.ok = kb_end_ok(S.st, S.e, nb);
        handed[s] = wk.ok ? 0u : 1u;
        wk.total = S.st.total;
        wk.parts = n;
        wk.holds = 0;
        wk.pos.assign(wk.ok ? S.st.nbrk : 0, ~0ull);  // (brk_idx[s] = 0 for a stream handed over)
    }
    for (uint32_t g = 0; g < (uint32_t)run; g++) {  // the fill: a wave per part
        if (!kq_fills(ents[g])) {
            N.fill_skipped++;
            continue;
        }
        const uint64_t s = kp_stream_of(base.data(), count, g);
        if (handed[s]) {
            N.fill_handed++;
            continue;
        }
        Walk &wk = out[s];
        KqState S = kq_from(ents[g]);
        uint32_t stored = 0;
        auto put_at = [&](uint32_t k, uint64_t o) {
            if (k >= wk.pos.size() || wk.pos[k] != ~0ull) fail("fill: a Break position stored twice or out of range");
            wk.pos[k] = o;
            stored++;
        };
        (void)emu_block<C>(ins[s]->data(), (uint32_t)ins[s]->size(), (g - base[s]) * P, S.e, lim32, limit, S.st, true, put_at);
        if (stored == 0) fail("fill: a part staged again stores nothing");
        wk.holds++;
        N.filled++;
    }
    for (uint64_t s = 0; s < count; s++)
        for (uint64_t p : out[s].pos)
            if (p == ~0ull) fail("a Break position was never stored");
    std::free(recs);
    std::free(ents);
    return out;
}

// The same chain walked by one lane from the stream's start to its end (kb_serial), and the parts of
// P bytes that hold a Break of it.
Walk serial(const Bytes &s, int64_t limit, uint32_t P) {
    using namespace ez;
    const Padded at(s);
    const uint32_t nb = (uint32_t)s.size();
    const int32_t lim32 = k2_lim32(limit);
    Walk wk;
    uint32_t end = 0;
    const KbState st = kb_serial([&](uint32_t p) { return at(p); }, nb, lim32, limit,
                                 [&](uint32_t k, uint64_t out) {
                                     if (k != wk.pos.size()) fail("the serial walk numbers its Breaks out of order");
                                     wk.pos.push_back(out);
                                 },
                                 &end);
    wk.ok = kb_end_ok(st, end, nb);
    wk.total = st.total;
    wk.parts = kp_parts_of(nb, P / kZLanes);
    // where the Breaks lie: the same steps once more, by position
    std::set<uint32_t> held;
    KbState t = kb_start();
    uint32_t p = 0;
    while (p < nb && !t.stop) {
        const uint32_t before = t.nbrk;
        const uint32_t np = kb_step(at(p), p, nb, lim32, limit, t, [](uint32_t, uint64_t) {});
        if (t.nbrk != before) held.insert(p / P);
        p = np;
    }
    wk.holds = (uint32_t)held.size();
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

void dump(const std::string &name, const Bytes &s, int64_t limit, const Ref &ref, const Walk &w256, const Walk &w1024) {
    if (!g_dump) return;
    const uint64_t h[12] = {name.size(), (uint64_t)limit, s.size(), ref.pos.size(), ref.size, (uint64_t)ref.err,
                            w256.ok ? 1u : 0u, w256.parts, w256.holds, w1024.ok ? 1u : 0u, w1024.parts, w1024.holds};
    std::fwrite(h, 8, 12, g_dump);
    std::fwrite(name.data(), 1, name.size(), g_dump);
    std::fwrite(s.data(), 1, s.size(), g_dump);
    std::fwrite(ref.pos.data(), 8, ref.pos.size(), g_dump);
}

bool same(const Walk &r, const Walk &one) { return r.ok == one.ok && (!r.ok || (r.pos == one.pos && r.total == one.total && r.holds == one.holds)); }

void show(const char *who, const Walk &w) {
    std::printf("  %s: taken %d total %llu breaks %zu parts %u holding %u:", who, (int)w.ok, (unsigned long long)w.total, w.pos.size(), w.parts, w.holds);
    for (size_t k = 0; k < w.pos.size() && k < 12; k++) std::printf(" %llu", (unsigned long long)w.pos[k]);
    std::printf("\n");
}

std::vector<std::pair<Bytes, int64_t>> g_kept;  // the whole streams, for the batch at the end

// want: the ErrBreaks the Reader is to return (-1: whatever it finds); taken: the route is to take it (-1: either)
void check_one(const std::string &name, const Bytes &s, int64_t limit, int want, int taken, bool whole_stream) {
    const Ref ref = reader(s, limit);
    if (want >= 0 && ref.pos.size() != (size_t)want) {
        std::printf("MISMATCH %s (%zu bytes): built to have %d Breaks, the Reader returns %zu\n", name.c_str(), s.size(), want, ref.pos.size());
        std::exit(1);
    }
    const std::vector<const Bytes *> ins(1, &s);
    Walk got[2];
    for (int c = 0; c < 2; c++) {
        const Walk one = serial(s, limit, c == 0 ? ez::kp_part_bytes(256) : ez::kp_part_bytes(1024));
        if (taken >= 0 && one.ok != (taken != 0)) {
            std::printf("MISMATCH %s (%zu bytes): built to be %s, the serial walk says taken %d\n", name.c_str(), s.size(), taken ? "taken" : "handed over",
                        (int)one.ok);
            std::exit(1);
        }
        if (one.ok && (ref.err != 0 || ref.size != one.total || ref.pos != one.pos)) {
            std::printf("MISMATCH %s (%zu bytes): the Reader ends with error %d, size %llu, %zu Breaks\n", name.c_str(), s.size(), ref.err,
                        (unsigned long long)ref.size, ref.pos.size());
            show("serial walk", one);
            std::exit(1);
        }
        got[c] = c == 0 ? emulate<256>(ins, limit)[0] : emulate<1024>(ins, limit)[0];
        (c == 0 ? N.chunk256 : N.chunk1024)++;
        if (!same(got[c], one) || got[c].parts != one.parts) {
            std::printf("MISMATCH %s (%zu bytes, chunk %d)\n", name.c_str(), s.size(), c == 0 ? 256 : 1024);
            show("serial walk", one);
            show("parts", got[c]);
            std::exit(1);
        }
        if (c == 0) (one.ok ? N.taken : N.stops)++;
    }
    N.streams++;
    N.breaks_found += ref.pos.size();
    if (whole_stream) {
        dump(name, s, limit, ref, got[0], got[1]);
        g_kept.push_back(std::make_pair(s, limit));
    }
}

// the stream, and the stream cut at each of its last 27 bytes
void check(const std::string &name, const Bytes &s, int want, int64_t limit = 0, bool tails = false, int taken = 1) {
    check_one(name, s, limit, want, taken, true);
    for (size_t cut = 1; tails && cut <= 27 && cut <= s.size(); cut++) {
        const Bytes t(s.begin(), s.end() - (long)cut);
        N.tail_cuts++;
        check_one(name + " cut " + std::to_string(cut), t, limit, -1, -1, false);
    }
}

template <int C>
void streams_for_chunk() {
    const std::string cn = "C" + std::to_string(C) + " ";
    const size_t P = ez::kp_part_bytes(C);
    static const uint8_t kb[2] = {0x80, 0x1f}, kr[3] = {0x80, 0x10, 0x14};
    // Part seam: a Break whose 80 lies at each of the last 8 positions before the seam of parts 0 | 1 (at -1
    // the 1f is the next part's first byte) and at the first position after it; one more in part 2
    for (int d = 8; d >= 0; d--) {
        Bytes s;
        hdr(s);
        fill_to(s, P - (size_t)d);
        brk(s);
        fill_to(s, 2 * P + 100);
        brk(s);
        body(s, 300);
        tail3(s);
        (d ? N.seam_before : N.seam_after)++;
        check(cn + (d ? "break part seam -" + std::to_string(d) : "break at a part's first byte"), s, 2, 0, d == 1);
    }
    {  // 5,000 Breaks back to back across the seam of parts 0 | 1
        Bytes s;
        hdr(s);
        fill_to(s, P - 5001);
        for (int k = 0; k < 5000; k++) brk(s);
        fill_to(s, 2 * P + 200);
        brk(s);
        tail3(s);
        N.many_breaks++;
        check(cn + "5000 breaks across a seam", s, 5001);
    }
    // 2 and 3 Breaks with nothing between them, straddling the seam at every offset
    for (int n = 2; n <= 3; n++)
        for (int off = 1; off < 2 * n; off++) {
            Bytes s;
            hdr(s);
            fill_to(s, P - (size_t)off);
            for (int k = 0; k < n; k++) brk(s);
            body(s, P / 2);
            tail3(s);
            N.straddle++;
            check(cn + std::to_string(n) + " breaks with nothing between, seam -" + std::to_string(off), s, n);
        }
    {  // a Break before the stream's first output byte in part 0 (and before the header's Reset)
        Bytes s;
        brk(s);
        hdr(s);
        brk(s);
        fill_to(s, P + P / 2);
        brk(s);
        tail3(s);
        N.first_output++;
        check(cn + "breaks before the first output byte", s, 3);
    }
    {  // a part whose only Breaks lie behind a Reset (part 1), none in parts 0 and 2
        Bytes s;
        hdr(s);
        fill_to(s, P + 300);
        rst(s);
        brk(s);
        lit_rnd(s, 3);
        brk(s);
        fill_to(s, 2 * P + P / 2);
        tail3(s);
        N.behind_reset++;
        check(cn + "a part whose only breaks lie behind a reset", s, 2);
    }
    // a Break right before and right after a Reset at a seam: the Reset ends at the seam, straddles it, starts at it
    for (int d = 3; d >= 0; d--) {
        Bytes s;
        hdr(s);
        fill_to(s, P - 2 - (size_t)d);
        brk(s);
        rst(s, 0x12);
        brk(s);
        fill_to(s, 2 * P + 50);
        brk(s);
        rst(s);
        brk(s);
        tail3(s);
        N.around_reset_seam++;
        check(cn + "breaks around a reset at a seam -" + std::to_string(d), s, 4);
    }
    {  // a literal over exactly one whole part whose body is all 80 1f (part 1 is passed through and counts nothing)
        Bytes s;
        hdr(s);
        fill_to(s, P - 50);
        lit_of(s, cycle_body(kb, 2, P + 100, 0));
        brk(s);
        body(s, 300);
        tail3(s);
        N.spanned++;
        check(cn + "a literal of breaks over a whole part", s, 1);
    }
    // literal bodies made of 80 1f, of 80 10 14 and of whole headers across the seams (parts walked
    // again), real Breaks between and after them
    for (int kind = 0; kind < 3; kind++)
        for (size_t phase = 0; phase < 3; phase++) {
            Bytes s;
            hdr(s);
            s.push_back(0);
            for (int k = 0; k < 6; k++) {
                const size_t n = P / 2 + 1 + (size_t)k;
                lit_of(s, kind == 0 ? cycle_body(kb, 2, n, phase + (size_t)k) : (kind == 1 ? cycle_body(kr, 3, n, phase + (size_t)k) : cycle_body(kHdr, 9, n, phase * 3 + (size_t)k)));
                if (k % 2 == 1) brk(s);
                if (k == 2) rst(s, 0x10);
            }
            brk(s);
            tail3(s);
            N.adversarial++;
            g_adversarial = true;
            check(cn + (kind == 0 ? "breaks" : (kind == 1 ? "resets" : "headers")) + " in literal bodies, phase " + std::to_string(phase), s, 4);
            g_adversarial = false;
        }
    {  // literal bodies that parse as 2-byte copies on the other parity, a Break after every tenth literal, over 3 parts
        Bytes s;
        hdr(s);
        s.push_back(0);  // (padding: the first literal at position 10)
        int k = 0, breaks = 0;
        while (s.size() < 3 * P + 700) {
            tag(s, 0x00, 256);
            for (int q = 0; q < 128; q++) {
                s.push_back(0x10);
                s.push_back(0x85);
            }
            if (k++ % 10 == 9) {
                brk(s);  // (two bytes: the next literal at an even position again)
                breaks++;
            }
        }
        tail3(s);
        N.adversarial++;
        g_adversarial = true;
        check(cn + "copy headers in literal bodies, breaks between", s, breaks);
        g_adversarial = false;
    }
    {  // a segment that opens in part 0 and closes in part 2, with a distance only the other segment's
        // window holds: Breaks in parts 0 and 1, the stop in part 2, the whole stream handed over
        Bytes s;
        hdr(s, 20);
        body(s, P / 2);
        brk(s);
        cpy(s, 5000, 40);
        rst(s, 10);
        lit_rnd(s, 50);
        brk(s);
        cpy(s, 5000, 40);
        fill_to(s, P + P / 2);
        brk(s);
        fill_to(s, 2 * P + 100);
        rst(s, 10);
        body(s, P / 2);
        brk(s);
        N.far_window_stop++;
        check(cn + "a segment over three parts with a distance past its window", s, 2, 0, false, 0);
    }
    {  // a form the parse hands over in part 2, Breaks in parts 0 and 1
        Bytes s;
        hdr(s);
        fill_to(s, P / 2);
        brk(s);
        fill_to(s, P + P / 2);
        brk(s);
        fill_to(s, 2 * P + P / 2);
        static const uint8_t wide_break[3] = {0x80, 0x18 | 6, 0x00};
        put(s, wide_break, 3);
        body(s, 300);
        brk(s);
        N.handover_late++;
        check(cn + "a wide meta in part 2, breaks before it", s, -1, 0, false, 0);
    }
    // an error in the middle, Breaks on both sides: those after it are not listed
    for (int kind = 0; kind < 5; kind++) {
        Bytes s;
        hdr(s, kind == 4 ? 16 : 20);
        for (int k = 0; k < 3; k++) {
            body(s, P * 7 / 20);
            brk(s);
        }
        if (kind == 0) meta(s, 0 << 3, "eazx", 4);
        else if (kind == 1) meta(s, 1 << 3, "\x01", 1);
        else if (kind == 2) meta(s, 5 << 3, "\x00", 1);
        else if (kind == 3) meta(s, 3 << 3, "\x07", 1);  // 80 18 xx: a Break with a length
        else lit_rnd(s, 70000);                           // (over a BlockSizeLimit of 64 KiB)
        for (int k = 0; k < 2; k++) {
            body(s, P * 7 / 20);
            brk(s);
        }
        N.err_mid++;
        check(cn + "error kind " + std::to_string(kind) + " between breaks", s, 3, kind == 4 ? 65536 : 0, false, 0);
    }
    {  // truncation at each of the last 27 bytes of a stream of 3 parts that ends in Breaks
        Bytes s;
        hdr(s);
        for (int k = 0; k < 5; k++) {
            body(s, P / 2);
            brk(s);
        }
        lit_rnd(s, 9);
        cpy(s, 300, 20);
        brk(s);
        lit_rnd(s, 3);
        brk(s);
        brk(s);
        check(cn + "a stream of three parts that ends in breaks", s, 8, 0, true);
    }
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
    streams_for_chunk<256>();
    streams_for_chunk<1024>();
    if (g_dump) std::fclose(g_dump);
    g_dump = nullptr;
    // batches: the whole streams of each BlockSizeLimit with empty and 10-byte streams between them,
    // laid out and searched as the kernels do
    for (int64_t limit : {(int64_t)0, (int64_t)65536}) {
        std::vector<Bytes> shorts(3);
        hdr(shorts[1]);
        shorts[1].push_back(0);
        hdr(shorts[2]);
        shorts[2].pop_back();
        lit_rnd(shorts[2], 1);
        std::vector<const Bytes *> ins;
        for (size_t k = 0; k < g_kept.size(); k++) {
            if (g_kept[k].second != limit) continue;
            ins.push_back(&shorts[k % 3]);
            ins.push_back(&g_kept[k].first);
            if (k % 5 == 0) ins.push_back(&shorts[(k + 1) % 3]);
        }
        ins.push_back(&shorts[0]);
        for (int c = 0; c < 2; c++) {
            const std::vector<Walk> got = c == 0 ? emulate<256>(ins, limit) : emulate<1024>(ins, limit);
            for (size_t s = 0; s < ins.size(); s++) {
                if (!same(got[s], serial(*ins[s], limit, c == 0 ? ez::kp_part_bytes(256) : ez::kp_part_bytes(1024)))) {
                    std::printf("MISMATCH batch stream %zu (%zu bytes, chunk %d)\n", s, ins[s]->size(), c == 0 ? 256 : 1024);
                    return 1;
                }
                N.batch_streams++;
                if (ins[s]->empty()) N.batch_empty++;
                else if (ins[s]->size() <= 10) N.batch_short++;
            }
        }
    }
#define P(f) K2_COUNT(N, 20, f)
    P(streams); P(breaks_found); P(taken); P(stops); P(parts); P(joined); P(passed); P(again); P(again_adversarial); P(again_entry); P(again_marked);
    P(walk_marked); P(filled); P(fill_skipped); P(fill_handed); P(dead_parts); P(seam_before); P(seam_after); P(many_breaks); P(straddle);
    P(first_output); P(behind_reset); P(around_reset_seam); P(spanned); P(adversarial); P(far_window_stop); P(handover_late); P(err_mid);
    P(tail_cuts); P(batch_streams); P(batch_short); P(batch_empty); P(unsettled); P(chunk256); P(chunk1024);
    std::printf("ok\n");
    return 0;
}
