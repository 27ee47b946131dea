// Host check of the steps of K2g's parts route (eazy_amd/csrc/ez_k2_segs_parts.h, over ez_k2_parts.h's
// grid, ez_k2_segs.h's state and ez_k2_size.h's walk): the same source, compiled for the CPU and run
// over emulated lanes, parts and streams exactly as the kernels order them
// (ez_decompress_segs_parts.hip: the part layout, a wave per part whose lanes' sums are joined as a
// tree, a wave per stream over 64 records per load that leaves every part's entry state, then a wave
// per part that fills the cuts in from its entry state), for chunk 256 and chunk 1,024.  Per stream:
//   the cut list (input position, output before), the stop, and the size query's verdict and total
//   equal a single lane's walk of the whole chain (kg_serial, kg_end_ok);
//   the number of cuts is the one the stream was built to have;
//   decoding each segment alone with the oracle's Reader and joining the results gives the whole
//   stream's bytes, every segment but the last ends without an error, and the last one's error is the
//   whole stream's.
//   k2_segs_parts_check             prints the count of every class, exits 1 at the first mismatch
//   k2_segs_parts_check --dump F    also writes every untruncated stream and its cuts to F, in
//                                   k2_segs_check's format (the GPU test's input)
//
// Streams (tokens written one by one with the oracle's Encoder) of 2 to 6 parts, P = 64 chunks: see
// streams_for_chunk() and main().  The builder, the oracle call and the wave's walk of a part
// (emu_walk, the mirror of kz_walk) are tools/k2_check_common.h's.
#include <utility>

#include "../eazy_amd/csrc/ez_k2_segs_parts.h"
#include "k2_check_common.h"

using namespace k2check;

namespace {

typedef std::vector<std::pair<uint32_t, uint64_t>> Cuts;

struct Counts {
    uint64_t streams, cuts_found, stops, parts, joined, passed, again, again_adversarial, again_entry, again_marked, walk_marked, take_plain, take_lead, take_first,
        stop_first, filled, fill_walked, fill_skipped, dead_parts, seam_before, seam_after, packed40, empty_straddle, lead_not_cuts, lead_all_cuts,
        many_cuts, lit_whole_part, adversarial, far_window_stop, exact_window, handover_then_resets, err_seg2, tail_cuts, sized_ok, sized_handed,
        batch_streams, batch_short, batch_empty, oracle_segments, unsettled, chunk256, chunk1024;
} N;
bool g_adversarial;  // the stream under check is one built to keep speculation off the true chain
std::FILE *g_dump;

void lit_of(Bytes &v, const Bytes &body) {
    tag(v, 0x00, (int64_t)body.size());
    put(v, body);
}
void body(Bytes &v, size_t n, int maxd = 200) { fill_to(v, v.size() + n, maxd); }

struct Walk {
    Cuts cuts;
    bool stop;
    bool sized;  // the size query's verdict (kg_end_ok)
    uint64_t total;
};

// ---- the kernels' steps, lanes and parts emulated in order
// part_rec of ez_decompress_segs_parts.hip: one part by 64 lanes, their sums joined as the kernel's tree
template <int C>
ez::KsRec emu_rec(const uint8_t *in, uint32_t nb, uint32_t ps, int32_t lim32, int64_t limit) {
    using namespace ez;
    EmuWave<C> wv(kp_stage_bytes(C));
    EmuStats st{};
    const KzWin w = emu_walk<C>(wv, in, nb, kp_stage_base(ps, C), ps, false, 0, st);
    if (!wv.settled) {
        N.unsettled++;
        return ks_rec_unsettled();
    }
    KsSum r[kZLanes];
    for (int l = 0; l < kZLanes; l++) r[l] = ks_sum<C>(w, ps, l, nb, wv.a[l], wv.x[l], lim32, limit);
    for (int d = 1; d < kZLanes; d <<= 1)
        for (int l = 0; l < kZLanes; l += 2 * d) ks_append(r[l], r[l + d]);
    return ks_rec(r[0], wv.a[0], wv.x[kZLanes - 1]);
}

// ks_block: the part at ps from the true position e, with the state
template <int C, class Cut>
uint32_t emu_block(const uint8_t *in, uint32_t nb, uint32_t ps, uint32_t e, int32_t lim32, int64_t limit, ez::KgState &st, Cut cut) {
    using namespace ez;
    EmuWave<C> wv(kp_stage_bytes(C));
    EmuStats es{};
    const KzWin w = emu_walk<C>(wv, in, nb, kp_stage_base(ps, C), ps, true, e, es);
    if (!wv.settled) {
        N.unsettled++;
        st.stop = true;
        return e;
    }
    KgSum r[kZLanes];
    for (int l = 0; l < kZLanes; l++) r[l] = kg_sum<C>(w, ps, l, nb, wv.a[l], wv.x[l], lim32, limit);
    for (int l = 0; l < kZLanes; l++) {  // (the kernel: the prefix up to each event, then kg_cuts on every lane)
        st.total += r[l].out;
        st.maxd = r[l].maxd > st.maxd ? r[l].maxd : st.maxd;
        if (r[l].fl == 0) continue;
        kg_cuts<C>(w, ps, l, nb, r[l].epos, wv.x[l], lim32, limit, st, cut);
        if (st.stop) return e;
    }
    return wv.x[kZLanes - 1];
}

// kp_layout (the serial layout; its thread steps are tools/k2_layout_check.cpp's to check), ks_first,
// ks_order and ks_fill over a batch; a stream without parts is the wave route's
// (tools/k2_segs_check.hip holds that one to the same serial walk: here it is the serial walk itself)
Walk serial(const Bytes &s, int64_t limit);
template <int C>
std::vector<Walk> emulate(const std::vector<const Bytes *> &ins, int64_t limit) {
    using namespace ez;
    const int32_t lim32 = k2_lim32(limit);
    const uint64_t count = ins.size();
    constexpr uint32_t P = kp_part_bytes(C);
    std::vector<uint32_t> base(count + 1);
    uint64_t run = 0;
    for (uint64_t s = 0; s < count; s++) {
        base[s] = (uint32_t)run;
        run += kp_parts_of(ins[s]->size(), C);
    }
    base[count] = (uint32_t)run;
    // (dirty scratch: what the kernels find there must not matter)
    KsRec *recs = (KsRec *)std::malloc(sizeof(KsRec) * (run ? run : 1));
    KsEnt *ents = (KsEnt *)std::malloc(sizeof(KsEnt) * (run ? run : 1));
    std::memset(recs, 0xa5, sizeof(KsRec) * (run ? run : 1));
    std::memset(ents, 0xa5, sizeof(KsEnt) * (run ? run : 1));
    for (uint32_t g = 0; g < (uint32_t)run; g++) {
        const uint64_t s = kp_stream_of(base.data(), count, g);
        if (!(base[s] <= g && g < base[s + 1])) {
            std::printf("MISMATCH part %u of the batch is not one of stream %llu\n", g, (unsigned long long)s);
            std::exit(1);
        }
        recs[g] = emu_rec<C>(ins[s]->data(), (uint32_t)ins[s]->size(), (g - base[s]) * P, lim32, limit);
        if (recs[g].fl & kSWalk) N.walk_marked++;
        N.parts++;
    }
    std::vector<Walk> out(count);
    for (uint64_t s = 0; s < count; s++) {
        const uint32_t n = base[s + 1] - base[s];
        if (n == 0) {
            out[s] = serial(*ins[s], limit);
            continue;
        }
        const uint32_t nb = (uint32_t)ins[s]->size();
        const uint8_t *b = ins[s]->data();
        const KsRec *rs = recs + base[s];
        KsEnt *es = ents + base[s];
        KsState S = ks_start();
        uint32_t j = 0;
        while (j < n) {
            if (S.st.stop || S.e >= nb) {
                for (uint32_t q = j; q < n; q++) es[q] = ks_ent(S, false), N.dead_parts++;
                break;
            }
            const uint32_t at = S.e / P;
            if (at > j) {
                const uint32_t to = at < n ? at : n;
                for (uint32_t q = j; q < to; q++) es[q] = ks_ent(S, false), N.passed++;
                j = to;
                continue;
            }
            const uint32_t m = n - j < (uint32_t)kZLanes ? n - j : (uint32_t)kZLanes;
            uint32_t k = 0;
            for (; k < m && !S.st.stop; k++) {
                const uint32_t ps = (j + k) * P;
                const uint32_t pe = nb - ps > P ? ps + P : nb;
                const KsRec r = rs[j + k];
                const int cls = ks_class(S, pe, r);
                es[j + k] = ks_ent(S, cls != kSPass);
                if (cls == kSPass) {
                    N.passed++;
                    continue;
                }
                if (cls == kSAgain) {
                    const uint32_t x = emu_block<C>(b, nb, ps, S.e, lim32, limit, S.st, [](uint32_t, uint32_t, uint64_t) {});
                    if (!S.st.stop) S.e = x;
                    (g_adversarial ? N.again_adversarial : N.again)++;
                    (r.ent != S.e ? N.again_entry : N.again_marked)++;
                } else {
                    const bool lead = r.nreset != 0 && S.st.total == 0 && r.nlead != 0;
                    ks_take(S, r);
                    N.joined++;
                    if (r.nreset == 0) N.take_plain++;
                    else if (lead) N.take_lead++;
                    else if (S.st.stop) N.stop_first++;
                    else N.take_first++;
                }
            }
            j += k;
        }
        Walk &wk = out[s];
        wk.stop = S.st.stop;
        wk.total = S.st.total;
        wk.sized = kg_end_ok(S.st, S.e, nb);
        wk.cuts.assign(S.st.ncut, std::make_pair(0xa5a5a5a5u, (uint64_t)0xa5a5a5a5a5a5a5a5ull));
    }
    for (uint32_t g = 0; g < (uint32_t)run; g++) {  // the fill: a wave per part
        if (!ks_fills(recs[g], ents[g])) {
            N.fill_skipped++;
            continue;
        }
        const uint64_t s = kp_stream_of(base.data(), count, g);
        Walk &wk = out[s];
        KsState S = ks_from(ents[g]);
        auto cut = [&](uint32_t i, uint32_t pos, uint64_t o) {
            if (i >= wk.cuts.size() || wk.cuts[i].first != 0xa5a5a5a5u) {
                std::printf("MISMATCH fill: cut %u of %zu written twice or out of range\n", i, wk.cuts.size());
                std::exit(1);
            }
            wk.cuts[i] = std::make_pair(pos, o);
        };
        (void)emu_block<C>(ins[s]->data(), (uint32_t)ins[s]->size(), (g - base[s]) * P, S.e, lim32, limit, S.st, cut);
        N.fill_walked++;
        if (S.st.ncut != ents[g].ncut) N.filled++;
    }
    std::free(recs);
    std::free(ents);
    return out;
}

// The same chain walked by one lane from the stream's start to its end.
Walk serial(const Bytes &s, int64_t limit) {
    using namespace ez;
    const Padded at(s);
    Walk wk;
    uint32_t end = 0;
    const KgState st = kg_serial([&](uint32_t p) { return at(p); }, (uint32_t)s.size(), k2_lim32(limit), limit,
                                 [&](uint32_t, uint32_t pos, uint64_t out) { wk.cuts.push_back(std::make_pair(pos, out)); }, &end);
    wk.stop = st.stop;
    wk.total = st.total;
    wk.sized = kg_end_ok(st, end, (uint32_t)s.size());
    return wk;
}

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

bool same(const Walk &r, const Walk &one) {
    return r.cuts == one.cuts && r.stop == one.stop && r.sized == one.sized && (r.stop || r.total == one.total);
}

std::vector<std::pair<Bytes, int64_t>> g_kept;  // the whole streams, for the batch at the end

size_t check_one(const std::string &name, const Bytes &s, int64_t limit, int want, bool whole_stream) {
    const Walk one = serial(s, limit);
    if (want >= 0 && one.cuts.size() != (size_t)want) {
        std::printf("MISMATCH %s (%zu bytes): built to have %d cuts, the serial walk finds %zu\n", name.c_str(), s.size(), want, one.cuts.size());
        std::exit(1);
    }
    const std::vector<const Bytes *> ins(1, &s);
    for (int c = 0; c < 2; c++) {
        const Walk r = c == 0 ? emulate<256>(ins, limit)[0] : emulate<1024>(ins, limit)[0];
        (c == 0 ? N.chunk256 : N.chunk1024)++;
        if (!same(r, one)) {
            std::printf("MISMATCH %s (%zu bytes, chunk %d): serial walk %zu cuts stop %d sized %d total %llu | parts %zu cuts stop %d sized %d total %llu\n",
                        name.c_str(), s.size(), c == 0 ? 256 : 1024, one.cuts.size(), (int)one.stop, (int)one.sized, (unsigned long long)one.total,
                        r.cuts.size(), (int)r.stop, (int)r.sized, (unsigned long long)r.total);
            for (size_t k = 0; k < one.cuts.size() || k < r.cuts.size(); k++)
                std::printf("  cut %zu: serial (%lld, %lld) | parts (%lld, %lld)\n", k, k < one.cuts.size() ? (long long)one.cuts[k].first : -1,
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
            std::printf("MISMATCH %s (%zu bytes): segment %zu of %zu [%zu, %zu): oracle err %d (whole stream %d), output before it %zu\n", name.c_str(),
                        s.size(), g, one.cuts.size() + 1, i0, i1, err, werr, cat.size());
            std::exit(1);
        }
        put(cat, part);
    }
    if (cat != whole) {
        std::printf("MISMATCH %s (%zu bytes): the segments' outputs joined (%zu bytes) are not the whole stream's (%zu bytes)\n", name.c_str(), s.size(),
                    cat.size(), whole.size());
        std::exit(1);
    }
    if (one.sized && (werr != 0 || one.total != whole.size())) {
        std::printf("MISMATCH %s (%zu bytes): sized as %llu, the oracle reads %zu bytes with err %d\n", name.c_str(), s.size(),
                    (unsigned long long)one.total, whole.size(), werr);
        std::exit(1);
    }
    (one.sized ? N.sized_ok : N.sized_handed)++;
    N.streams++;
    N.cuts_found += one.cuts.size();
    if (one.stop) N.stops++;
    if (whole_stream) {
        dump(name, s, limit, one);
        g_kept.push_back(std::make_pair(s, limit));
    }
    return one.cuts.size();
}

// the stream, and the stream cut at each of its last 27 bytes
void check(const std::string &name, const Bytes &s, int want, int64_t limit = 0, bool tails = false) {
    check_one(name, s, limit, want, true);
    for (size_t cut = 1; tails && cut <= 27 && cut <= s.size(); cut++) {
        const Bytes t(s.begin(), s.end() - (long)cut);
        N.tail_cuts++;
        check_one(name + " cut " + std::to_string(cut), t, limit, -1, false);
    }
}

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
    const size_t P = ez::kp_part_bytes(C);
    // a Reset at each of the last 8 positions before the seam of parts 0 | 1 and at the first after it; one more in part 2
    for (int d = 8; d >= 0; d--) {
        Bytes s;
        hdr(s);
        fill_to(s, P - (size_t)d);
        rst(s);
        fill_to(s, 2 * P + 100);
        rst(s);
        body(s, 300);
        tail3(s);
        (d ? N.seam_before : N.seam_after)++;
        check(cn + (d ? "reset part seam -" + std::to_string(d) : "reset at a part's first byte"), s, 2, 0, d == 1 || d == 0);
    }
    {  // 40 Resets in one part, a 1-byte literal after each (more than 15 cuts)
        Bytes s;
        hdr(s);
        fill_to(s, P + 50);
        for (int k = 0; k < 40; k++) {
            rst(s);
            lit_rnd(s, 1);
        }
        fill_to(s, 2 * P + 200);
        tail3(s);
        N.packed40++;
        check(cn + "40 resets in one part", s, 40);
    }
    // 2 and 3 Resets with nothing between them, straddling the seam at every offset
    for (int n = 2; n <= 3; n++)
        for (int off = 1; off < 3 * n; off++) {
            Bytes s;
            hdr(s);
            fill_to(s, P - (size_t)off);
            for (int k = 0; k < n; k++) rst(s);
            body(s, P / 2);
            tail3(s);
            N.empty_straddle++;
            check(cn + std::to_string(n) + " resets with nothing between, seam -" + std::to_string(off), s, n);
        }
    // leading Resets before the stream's first output byte that run across a seam: no cuts; with one
    // output byte in the part before: all cuts
    for (int first = 0; first < 2; first++)
        for (int form = 0; form < 2; form++) {
            Bytes s;
            hdr(s);
            if (first) lit_rnd(s, 1);
            if (form == 0) {  // padding up to 4 bytes before the seam, then 4 Resets
                s.insert(s.end(), P - 4 - s.size(), 0);
                for (int k = 0; k < 4; k++) rst(s);
            } else {  // Resets all the way, 7 of them past the seam
                while (s.size() < P + 20) rst(s);
            }
            const size_t resets = form == 0 ? 4 : (P + 20 - 9 - (size_t)(first ? 2 : 0) + 2) / 3;
            body(s, P / 2);
            rst(s);
            body(s, 100);
            tail3(s);
            (first ? N.lead_all_cuts : N.lead_not_cuts)++;
            check(cn + (first ? "resets across a seam after one output byte, form " : "leading resets across a seam, form ") + std::to_string(form), s,
                  first ? (int)resets + 1 : 1);
        }
    {  // more than 15 cuts over several parts: 24 segments of a quarter part
        Bytes s;
        for (int g = 0; g < 24; g++) {
            if (g == 0) hdr(s);
            else rst(s, 0x10 + g % 5);
            body(s, P / 4 + (size_t)g);
        }
        tail3(s);
        N.many_cuts++;
        check(cn + "24 segments over 6 parts", s, 23, 0, true);
    }
    {  // a literal that spans exactly one whole part, then a Reset (part 1 is passed through)
        Bytes s;
        hdr(s);
        fill_to(s, P - 50);
        lit_rnd(s, (int64_t)P + 100);
        rst(s);
        body(s, 300);
        tail3(s);
        N.lit_whole_part++;
        check(cn + "a literal over a whole part then a reset", s, 1);
    }
    // literal bodies made of 80 10 14 and of whole headers across the seams (parts walked again)
    for (int kind = 0; kind < 2; kind++)
        for (size_t phase = 0; phase < 3; phase++) {
            Bytes s;
            hdr(s);
            s.push_back(0);
            for (int k = 0; k < 6; k++) {
                lit_of(s, kind == 0 ? resets_body(P / 2 + 1 + (size_t)k, phase + (size_t)k) : headers_body(P / 2 + 2 + (size_t)k, phase * 3 + (size_t)k));
                if (k == 2) rst(s, 0x10);
            }
            rst(s);
            tail3(s);
            N.adversarial++;
            g_adversarial = true;
            check(cn + (kind == 0 ? "resets" : "headers") + " in literal bodies, phase " + std::to_string(phase), s, 2);
            g_adversarial = false;
        }
    {  // literal bodies that parse as 2-byte copies on the other parity, a Reset after every tenth literal, over 3 parts
        Bytes s;
        hdr(s);
        s.push_back(0);  // (padding: the first literal at position 10)
        int k = 0, resets = 0;
        while (s.size() < 3 * P + 700) {
            tag(s, 0x00, 256);
            for (int q = 0; q < 128; q++) {
                s.push_back(0x10);
                s.push_back(0x85);
            }
            if (k++ % 10 == 9) {
                rst(s);
                s.push_back(0);  // (the next literal at an even position again)
                resets++;
            }
        }
        tail3(s);
        N.adversarial++;
        g_adversarial = true;
        check(cn + "copy headers in literal bodies, resets between", s, resets);
        g_adversarial = false;
    }
    // a segment that opens in part 0 and closes in part 2, with a distance only the other segment's
    // window holds (the stop lands in part 2; the later Resets are no cuts), and with its longest
    // distance exactly its window
    for (int exact = 0; exact < 2; exact++) {
        Bytes s;
        hdr(s, 20);
        body(s, P / 2);
        cpy(s, 5000, 40);
        rst(s, 10);
        lit_rnd(s, 50);
        cpy(s, exact ? 1024 : 5000, 40);
        fill_to(s, 2 * P + 100);
        rst(s, 10);
        body(s, P / 2);
        rst(s, 10);
        fill_to(s, 3 * P + 100);
        rst(s, 12);
        body(s, 200);
        tail3(s);
        (exact ? N.exact_window : N.far_window_stop)++;
        check(cn + (exact ? "a segment over three parts whose longest distance is its window" : "a segment over three parts with a distance past its window"), s,
              exact ? 4 : 1);
    }
    {  // a form the parse hands over in part 1, Resets in part 2
        Bytes s;
        hdr(s);
        fill_to(s, P / 2);
        rst(s);
        fill_to(s, P + P / 2);
        static const uint8_t wide_break[3] = {0x80, 0x18 | 6, 0x00};
        put(s, wide_break, 3);
        fill_to(s, 2 * P + 100);
        rst(s);
        body(s, 300);
        rst(s);
        body(s, 100);
        N.handover_then_resets++;
        check(cn + "a wide meta in part 1, resets in part 2", s, 1);
    }
    // an error in segment 2 of 4, the segments 0.7 parts each, and truncation at each of the last 27 bytes
    for (int kind = 0; kind < 3; kind++) {
        Bytes s;
        for (int g = 0; g < 4; g++) {
            if (g == 0) hdr(s);
            else rst(s);
            body(s, P * 7 / 20);
            if (g == 2) {
                if (kind == 0) meta(s, 0 << 3, "eazx", 4);
                else if (kind == 1) meta(s, 1 << 3, "\x01", 1);
                else meta(s, 5 << 3, "\x00", 1);
            }
            body(s, P * 7 / 20);
        }
        tail3(s);
        N.err_seg2++;
        check(cn + "error kind " + std::to_string(kind) + " in segment 2 of 4", s, 2, 0, kind == 0);
    }
    {  // BlockSizeLimit below segment 2's window: its Reset is refused
        Bytes s;
        for (int g = 0; g < 4; g++) {
            if (g == 0) hdr(s, 16);
            else rst(s, g == 2 ? 20 : 16);
            body(s, P * 7 / 10);
        }
        N.err_seg2++;
        check(cn + "BlockSizeLimit below the window of segment 2 of 4", s, 1, 65536);
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
    g_out.resize(16 << 20);
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
                if (!same(got[s], serial(*ins[s], limit))) {
                    std::printf("MISMATCH batch stream %zu (%zu bytes, chunk %d)\n", s, ins[s]->size(), c == 0 ? 256 : 1024);
                    return 1;
                }
                N.batch_streams++;
                if (ins[s]->empty()) N.batch_empty++;
                else if (ins[s]->size() <= 10) N.batch_short++;
            }
        }
    }
#define P(f) K2_COUNT(N, 22, f)
    P(streams); P(cuts_found); P(stops); P(parts); P(joined); P(passed); P(again); P(again_adversarial); P(again_entry); P(again_marked); P(walk_marked); P(take_plain); P(take_lead);
    P(take_first); P(stop_first); P(filled); P(fill_walked); P(fill_skipped); P(dead_parts); P(seam_before); P(seam_after); P(packed40);
    P(empty_straddle); P(lead_not_cuts); P(lead_all_cuts); P(many_cuts); P(lit_whole_part); P(adversarial); P(far_window_stop); P(exact_window);
    P(handover_then_resets); P(err_seg2); P(tail_cuts); P(sized_ok); P(sized_handed); P(batch_streams); P(batch_short); P(batch_empty);
    P(oracle_segments); P(unsettled); P(chunk256); P(chunk1024);
    std::printf("ok\n");
    return 0;
}
