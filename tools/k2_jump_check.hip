// Host check of K2j's steps (eazy_amd/csrc/ez_k2_jump.h): the same source, compiled for the CPU, run
// stage by stage as ez_decompress_jump.hip's kernels run it, on a batch in one byte vector with
// offsets and K2j's own workspace layout (JLayout), compared per stream with the oracle's Reader
// (oracle/eazy_oracle.c) and with one in-order k2_scan walk of the whole stream:
//   a taken stream's size and bytes are the Reader's; taken or handed over is the in-order walk's
//   verdict; a stream handed over is an error of the Reader's or a hand-over by design (a MetaReset
//   after output, a slot too small, a cut the Reader still accepts); in a continuation (c_on) the stop
//   (tstop, tj, tL) is the in-order partial walk's.
//   k2_jump_check      prints the count of every class, exits 1 at the first mismatch
// The kernels' chunk-per-lane stages (kj_spec, kj_verify, kj_tok) run per block of 64 chunks over a
// staging buffer of exactly kJStage bytes, filled as kj_stage fills it and poisoned elsewhere; a read
// outside what was filled fails the check.  The wave-level stages (kj_init, kj_fix's loop, kj_scan's
// scan, kj_place, kj_expand's loop over the pieces, kj_jump, kj_gather, kj_final) are mirrored serially
// below, each under the name of the kernel it mirrors.  The extent guard (kj_guarded) is not run: the
// workspace is sized from the real extents.
// Every stream is decoded between two short streams (its chunks then start inside a block, at an odd
// batch offset, and a cut token reads the next stream's bytes), cut at each of its last 27 bytes, and
// alone as a continuation, whole and cut.  The chunk size is jchunk's: streams that start with a
// 100,000-byte literal put their batch above 96 KiB (1 KiB chunks), the others below (256 bytes).
#include <algorithm>
#include <map>

#include "../eazy_amd/csrc/ez_k2_jump.h"
#include "k2_check_common.h"

using namespace k2check;
using namespace ez;

namespace {

struct Counts {
    uint64_t runs, streams, taken, handed_error, handed_design, jc256, jc1024, blocks, seams, lit_enter, passthrough, merged, repairs,
        phase_repairs, bodies, pad_seam, pad_tail, cuts, cuts_taken, cuts_handed_ok, c_on, stops, tails, multi, empty, one_chunk,
        late_reset, no_reset, far_distance, short_slot, breaks;
} N;
bool g_phase;  // the stream under check is the off-phase one

[[noreturn]] void fail(const std::string &name, const char *what) {
    std::printf("MISMATCH %s: %s\n", name.c_str(), what);
    std::exit(1);
}

struct Batch {
    Bytes in;
    std::vector<uint64_t> in_off{0}, out_off{0};
    void add(const Bytes &s, uint64_t cap) {
        put(in, s);
        in_off.push_back(in.size());
        out_off.push_back(out_off.back() + cap);
    }
    uint64_t count() const { return in_off.size() - 1; }
};
struct Res {
    bool taken, nospace;
    uint64_t size;
    int32_t tstop, tj;
    int64_t tL;
    std::vector<uint64_t> breaks;
};

// ---- kj_stage: the block's staging, [first live chunk's start, last live chunk's end + 16) in 16-byte pieces
struct HostStage {
    const uint8_t *buf;
    uint64_t base, filled;
    V16 operator()(uint64_t y) const {
        if (y < base || y - base + 16 > filled) {
            std::printf("MISMATCH: a step read batch offset %llu outside the staged [%llu, %llu)\n", (unsigned long long)y, (unsigned long long)base,
                        (unsigned long long)(base + filled));
            std::exit(1);
        }
        V16 v;
        std::memcpy(&v, buf + (y - base), 16);
        return v;
    }
};
// every block of 64 chunks: start(K) = the first stream position lane K stages; body(c, K, S) for its live lanes
template <class Start, class Body>
void blocks(const DecompressArgs &A, const JWork &W, Start start, Body body) {
    static uint8_t stage[kJStage];
    const uint64_t total = A.in_off[A.count];
    for (uint32_t cb = 0; cb < W.cbase[A.count]; cb += 64) {
        KjChunk K[64];
        uint64_t base = ~0ull, stop = 0, filled = 0;
        for (uint32_t l = 0; l < 64; l++) {
            K[l] = kj_chunk(cb + l, W.cbase, (uint32_t)A.count, A.in_off, W.head, W.jc);
            if (!K[l].live) continue;
            base = std::min(base, K[l].b0 + (uint64_t)start(K[l]));
            stop = std::max(stop, K[l].b0 + (uint64_t)K[l].ce);
        }
        stop += 16;
        std::memset(stage, 0xcc, sizeof stage);
        for (uint64_t y = base; y < stop; y += 16, filled += 16) {  // (no live lane: base > stop)
            if (filled + 16 > (uint64_t)kJStage) fail("staging", "a block stages more than kJStage bytes");
            for (uint64_t k = 0; k < 16; k++) stage[filled + k] = y + k < total ? A.in[y + k] : 0;
        }
        N.blocks++;
        for (uint32_t l = 0; l < 64; l++)
            if (K[l].live) body(cb + l, K[l], HostStage{stage, base, filled});
    }
}

// ---- the stages on the host.  c_on: one stream, a continuation from its start (no history, no window yet)
std::vector<Res> emulate(const Batch &B, bool c_on, Bytes &out) {
    static Bytes ws;
    static std::vector<uint64_t> brk;
    const uint64_t count = B.count(), in_total = B.in.size(), out_bytes = B.out_off[count];
    const uint64_t out_total = out_bytes + 16;  // (launch_decompress_jump's, without a history)
    const JLayout Y(count, in_total, out_total);
    if (ws.size() < Y.total) ws.resize(Y.total);
    const JWork W = Y.bind(ws.data(), in_total, out_bytes);
    std::memset(W.pass, 0, 8 * (kJPasses + 2));
    std::memset(W.ptr, 0xff, 4 * out_total + 16);
    out.assign(out_bytes + 16, 0xa5);
    brk.assign(1 + kJRec, 0);
    int64_t end_state[8] = {0};
    DecompressArgs A{};
    A.in = B.in.data(), A.in_off = B.in_off.data(), A.out = out.data(), A.out_off = B.out_off.data(), A.count = count;
    A.breaks = count == 1 ? brk.data() : nullptr, A.breaks_cap = kJRec, A.end_state = count == 1 ? end_state : nullptr;
    A.c_on = c_on, A.c_bsl = -1;
    (W.jc == 256 ? N.jc256 : N.jc1024)++;
    N.runs++;
    // kj_init
    uint32_t carry = 0;
    for (uint64_t s = 0; s < count; s++) {
        const uint64_t nb = A.in_off[s + 1] - A.in_off[s], cap = A.out_off[s + 1] - A.out_off[s];
        JHead h{};
        h.state = (nb >= (1ull << 31) || cap >= (1ull << 32) - 2 || A.out_off[s + 1] - jg0(A) >= (1ull << 32) - 2) ? 1u : 0u;
        h.bsl = -1;
        h.tstop = (int32_t)nb;
        h.nchunk = nb == 0 ? 1u : (uint32_t)((nb + W.jc - 1) / W.jc);
        h.chunk0 = W.cbase[s] = carry;
        W.head[s] = h;
        carry += h.nchunk;
    }
    W.cbase[count] = carry;
    if (carry > Y.chunks) fail("layout", "more chunks than the workspace holds");
    // kj_spec
    blocks(A, W, [](const KjChunk &K) { return kj_warm0(K.c0); }, [&](uint32_t c, const KjChunk &K, const HostStage &S) {
        W.sexit[c] = (uint32_t)kj_spec_walk(S, K.b0, K.c0, K.ce, W.bits + (uint64_t)c * kJW);
    });
    // kj_verify
    blocks(A, W, [](const KjChunk &K) { return K.c0; }, [&](uint32_t c, const KjChunk &K, const HostStage &S) {
        const int32_t a = K.c0 == 0 ? 0 : (int32_t)W.sexit[c - 1];
        W.entry[c] = (uint32_t)a;
        W.cnt[c] = (uint32_t)kj_follow(S, K.b0, a, K.c0, K.ce, W.bits + (uint64_t)c * kJW, W.sexit + c);
        if (K.c0 != 0 && a >= K.ce) N.passthrough++;
        else if (K.c0 != 0 && W.cnt[c] == W.sexit[c]) N.merged++;
    });
    // kj_fix: the wave's loop, the chunks in order (the first wrongly entered chunk at or after k)
    for (uint64_t s = 0; s < count; s++) {
        JHead &H = W.head[s];
        if (H.state) continue;
        const int32_t nb = (int32_t)(A.in_off[s + 1] - A.in_off[s]);
        const uint32_t c00 = H.chunk0, nch = H.nchunk;
        uint32_t *texit = W.cnt;
        for (uint32_t k = 1; k < nch;) {
            uint32_t jf = k;
            while (jf < nch && texit[c00 + jf - 1] == W.sexit[c00 + jf - 1]) jf++;
            if (jf >= nch) break;
            const int32_t e = (int32_t)texit[c00 + jf - 1];
            const uint32_t kw = kj_holder(e, jf, nb, nch, W.jc);
            for (uint32_t x = jf; x < kw; x++) W.entry[c00 + x] = texit[c00 + x] = (uint32_t)e;
            if (kw >= nch) break;
            const int32_t cs = (int32_t)kw * W.jc, ce = cs + W.jc < nb ? cs + W.jc : nb;
            W.entry[c00 + kw] = (uint32_t)e;
            texit[c00 + kw] = (uint32_t)kj_follow(KjBatch{A.in, in_total}, A.in_off[s], e, cs, ce, W.bits + (uint64_t)(c00 + kw) * kJW, W.sexit + c00 + kw);
            (g_phase ? N.phase_repairs : N.repairs)++;
            k = kw + 1;
        }
        if (kj_chain_bad((int32_t)texit[c00 + nch - 1], nb, c_on)) H.state = 1;
    }
    // kj_tok
    blocks(A, W, [](const KjChunk &K) { return K.c0; }, [&](uint32_t c, const KjChunk &K, const HostStage &S) {
        const auto on_break = [&](uint64_t o) {
            const uint64_t at = A.breaks[0]++;
            if (at < A.breaks_cap) A.breaks[1 + at] = ((uint64_t)c << 32) | (o & 0xffffffffull);
        };
        const KjSum r = kj_tok_walk(S, K.b0, K.nb, K.ce, (int32_t)W.entry[c], k2_lim32(0), 0, c_on, W.ltok + (uint64_t)c * kJRec, W.head[K.s],
                                    A.breaks != nullptr, on_break);
        W.cnt[c] = r.n, W.cout[c] = r.out, W.cflag[c] = r.fl, W.cmaxd[c] = r.maxd;
    });
    // kj_scan: the wave's scan over the chunks in order, then lane 0's checks
    std::vector<Res> res(count);
    uint64_t tok_alloc = 0;
    for (uint64_t s = 0; s < count; s++) {
        JHead &H = W.head[s];
        if (H.state) continue;
        uint64_t tc = 0, oc = 0;
        int32_t bsl = c_on ? A.c_bsl : -1;
        bool bad = false;
        uint32_t maxd = 0;
        for (uint32_t c = H.chunk0; c < H.chunk0 + H.nchunk; c++) {
            const uint32_t fl = W.cflag[c];
            maxd = std::max(maxd, W.cmaxd[c]);
            W.ctbase[c] = tc, W.cobase[c] = oc;
            if (kj_chunk_bad(fl, oc, c_on && A.c_pos0 != 0)) bad = true;
            if (fl & kJFReset) bsl = (int32_t)((fl >> 8) & 0xff);
            tc += W.cnt[c], oc += W.cout[c];
        }
        if (!bad) bad = kj_stream_bad(oc, bsl, maxd, A.out_off[s + 1] - A.out_off[s], c_on, H, (int32_t)(A.in_off[s + 1] - A.in_off[s]), res[s].nospace);
        if (!bad) {
            H.tok0 = tok_alloc;
            tok_alloc += tc;
            if (tok_alloc > W.tok_cap) bad = true;
        }
        H.bsl = bsl, H.total = oc, H.ntok = tc;
        if (bad) H.state = 1;
    }
    // kj_place
    for (uint32_t c = 0; c < W.cbase[count]; c++) {
        const JHead &H = W.head[last_le(W.cbase, (uint32_t)count, c)];
        for (uint32_t k = 0; !H.state && k < W.cnt[c]; k++) {
            JTok t = W.ltok[(uint64_t)c * kJRec + k];
            t.dst += (uint32_t)W.cobase[c];
            W.tok[H.tok0 + W.ctbase[c] + k] = t;
        }
    }
    // kj_expand: kj_piece on every 16-byte piece of the ptr array's grid that holds output of a stream
    // (a whole piece inside one stream's output, else the stream's bytes of it)
    const uint64_t g0 = jg0(A);
    for (uint64_t s = 0; s < count; s++) {
        const JHead &H = W.head[s];
        for (uint64_t x = A.out_off[s], end = x + H.total; !H.state && x < end;) {
            const uint32_t n = (uint32_t)(std::min<uint64_t>(end, (x & ~15ull) + 16) - x);
            uint32_t by[4] = {0, 0, 0, 0}, pt[16];
            kj_piece(A, W, H, (uint32_t)s, x, n, g0, by, pt);
            for (uint32_t k = 0; k < n; k++) {
                out[x + k] = (uint8_t)(by[k >> 2] >> (8 * (k & 3)));
                W.ptr[x - g0 + k] = pt[k];
            }
            x += n;
        }
    }
    // kj_jump to the fixed point, then kj_gather
    const uint64_t pend = out_bytes - g0;
    for (bool changed = true; changed;) {
        changed = false;
        for (uint64_t p = 0; p < pend; p++) {
            const uint32_t q = W.ptr[p];
            if (q >= kJZero || q == (uint32_t)p) continue;
            if (q >= pend) fail("pointers", "a pointer past the batch's output");
            changed |= W.ptr[q] != q;
            W.ptr[p] = W.ptr[q];
        }
    }
    for (uint64_t p = 0; p < pend; p++) {
        const uint32_t q = W.ptr[p];
        if (q != kJGap && q != (uint32_t)p) out[g0 + p] = q == kJZero ? (uint8_t)0 : out[g0 + q];
    }
    // kj_final
    for (uint64_t s = 0; s < count; s++) {
        const JHead &H = W.head[s];
        res[s].taken = !H.state, res[s].size = H.total, res[s].tstop = H.tstop, res[s].tj = H.tj, res[s].tL = H.tL;
        for (uint64_t k = 0; A.breaks && !H.state && k < A.breaks[0]; k++)
            res[s].breaks.push_back(W.cobase[A.breaks[1 + k] >> 32] + (A.breaks[1 + k] & 0xffffffffull));
    }
    return res;
}

// ---- one walker over stream s of the batch, in order, with the full k2_scan and K2j's stream checks
Res in_order(const Batch &B, uint64_t s, bool c_on) {
    const KjBatch at{B.in.data(), B.in.size()};
    const uint64_t b0 = B.in_off[s];
    const int32_t nb = (int32_t)(B.in_off[s + 1] - b0);
    Res r{true, false, 0, nb, 0, 0, {}};
    JHead H{};
    H.tstop = nb;
    int32_t p = 0, bsl = -1;
    uint32_t maxd = 0;
    bool stopped = false;
    while (p < nb && !stopped) {
        K2Tok t;
        const V16 h = at(b0 + (uint64_t)p);
        const int k = k2_scan(h, p, nb, k2_lim32(0), 0, t, c_on);
        if (k == kParseHandOver || (k == kScanReset && r.size != 0)) r.taken = false;
        if (!r.taken) return r;
        if (k == kScanTail) {
            H.tstop = p, H.tj = t.adv ? t.j : 0, H.tL = t.adv ? t.L : 0;
            stopped = true;
        } else if (k == kScanReset) {
            bsl = (int32_t)t.marg;
        } else if (k == kParseToken) {
            r.size += (uint64_t)t.L;
            maxd = t.cp && t.D > maxd ? t.D : maxd;
        } else if (((uint32_t)h.lo & 0xffffu) == (0x80u | ((kMetaBreak | kMetaLen0) << 8))) {
            r.breaks.push_back(r.size);
        }
        p += t.adv;
    }
    r.taken = (stopped || !kj_chain_bad(p, nb, c_on)) && !kj_stream_bad(r.size, bsl, maxd, B.out_off[s + 1] - B.out_off[s], c_on, H, nb, r.nospace);
    r.tstop = H.tstop, r.tj = H.tj, r.tL = H.tL;
    return r;
}

// the oracle's Reader on a stream: its error and its output; kept for the streams that recur (the two
// short ones, every uncut stream), not for the cuts
struct Want {
    int err;
    Bytes out;
};
Want reader(const Bytes &s) {
    int64_t olen = 0;
    const int err = oracle(s.data(), s.size(), 0, olen);
    return Want{err, Bytes(g_out.begin(), g_out.begin() + olen)};
}
const Want &want_of(const Bytes &s) {
    static std::map<Bytes, Want> cache;
    auto it = cache.find(s);
    return it != cache.end() ? it->second : cache.emplace(s, reader(s)).first->second;
}

// One run.  streams[k]: design = handed over although the Reader accepts it; full: the uncut stream of
// a cut one (its output holds the cut's as a prefix), else null
struct Item {
    Bytes s;
    uint64_t cap;
    bool design;
    const Bytes *full;
};
// returns whether stream `focus` was taken
bool run(const std::string &name, const std::vector<Item> &items, bool c_on, size_t focus) {
    Batch B;
    for (const Item &i : items) B.add(i.s, i.cap);
    Bytes out;
    const std::vector<Res> got = emulate(B, c_on, out);
    for (size_t k = 0; k < items.size(); k++) {
        const Item &i = items[k];
        const std::string nm = name + " [stream " + std::to_string(k) + (c_on ? ", c_on]" : "]");
        const Res ref = in_order(B, k, c_on);
        const Res &r = got[k];
        if (r.taken != ref.taken || r.nospace != ref.nospace) fail(nm, r.taken ? "taken, the in-order walk hands it over" : "handed over, the in-order walk takes it");
        N.streams++;
        if (c_on && (r.tstop != ref.tstop || r.tj != ref.tj || r.tL != ref.tL)) fail(nm, "the continuation's stop is not the in-order walk's");
        if (c_on && r.nospace) fail(nm, "a continuation's output and tail do not fit a slot of the Reader's output length");
        const Want &w = want_of(i.full ? *i.full : i.s);
        const Want cut = i.full ? reader(i.s) : Want{0, Bytes()};
        const int err = i.full ? cut.err : w.err;
        if (!r.taken) {
            if (err != 0) N.handed_error++;
            else if (i.design) N.handed_design++;
            else if (i.full) N.cuts_handed_ok++;  // (a cut the Reader reads to a clean end: k2_size_check.hip, check_one)
            else fail(nm, "handed over, but the Reader accepts it and no design rule hands it over");
            continue;
        }
        N.taken++;
        if (i.design) fail(nm, "taken, but built to be handed over");
        if (r.size != ref.size) fail(nm, "size differs from the in-order walk's");
        std::vector<uint64_t> bs = r.breaks;  // (recorded unordered, in one-stream batches only)
        std::sort(bs.begin(), bs.end());
        if (items.size() == 1 && bs != ref.breaks) fail(nm, "Break positions differ from the in-order walk's");
        N.breaks += bs.size();
        // a whole stream: the Reader's output; a cut one or a continuation: the whole tokens' output, a prefix of it
        if (!c_on && (err != 0 || r.size != (i.full ? cut : w).out.size())) fail(nm, "taken, but not the Reader's size");
        if (r.size > w.out.size() || !std::equal(w.out.begin(), w.out.begin() + (long)r.size, out.begin() + (long)B.out_off[k])) fail(nm, "bytes differ from the Reader's");
        if (c_on) {
            N.c_on++;
            if (r.tstop < (int32_t)i.s.size()) N.stops++;
            if (r.tj > 0) N.tails++;
        }
    }
    return got[focus].taken;
}

Bytes g_before, g_after;  // the short streams around every stream under check
std::vector<Item> between(const Item &i) {
    return {Item{g_before, want_of(g_before).out.size() + 3, false, nullptr}, i, Item{g_after, want_of(g_after).out.size() + 1, false, nullptr}};
}
// the stream between the two short ones, alone as a continuation, and both again cut at each of its last 27 bytes
void check(const std::string &name, const Bytes &s, bool design = false) {
    const uint64_t cap = want_of(s).out.size() + 5;
    run(name, between(Item{s, cap, design, nullptr}), false, 1);
    if (!design) run(name, {Item{s, cap, false, nullptr}}, true, 0);
    for (size_t cut = 1; cut <= 27 && cut <= s.size(); cut++) {
        const Item t{Bytes(s.begin(), s.end() - (long)cut), cap, design, &s};
        const std::string nm = name + " cut " + std::to_string(cut);
        N.cuts++;
        if (run(nm, between(t), false, 1)) N.cuts_taken++;
        // (the continuation's slot: exactly what the Reader gets out of the cut stream, a literal's bytes at its end included)
        if (!design) run(nm, {Item{t.s, reader(t.s).out.size(), false, &s}}, true, 0);
    }
}

// a stream's start: the header, and for 1 KiB chunks a 100,000-byte literal
Bytes start(bool big, int bsl = 0x14) {
    Bytes s;
    hdr(s, bsl);
    if (big) lit_rnd(s, 100000);
    return s;
}
// the next chunk seam at least `room` bytes after the stream's present end
size_t seam_after(const Bytes &s, bool big, size_t room) {
    const size_t jc = big ? 1024 : 256;
    return (s.size() + room + jc - 1) / jc * jc + 2 * jc;
}

void streams_for_chunk(bool big, const std::vector<Form> &fs) {
    const std::string cn = big ? "C1024 " : "C256 ";
    // every form with its first byte 0 .. min(its length, 16) bytes before a chunk seam
    for (const Form &f : fs)
        for (size_t d = 0; d <= std::min<size_t>(f.b.size(), 16); d++) {
            Bytes s = start(big);
            if (f.big_first) lit_rnd(s, 70000);
            fill_to(s, seam_after(s, big, 0) - d);
            put(s, f.b);
            tail3(s);
            N.seams++;
            check(cn + f.name + " seam -" + std::to_string(d), s);
        }
    // a 70,000-byte literal that starts at several places of a chunk: the chunks inside it are entered past their ends
    for (int k = 0; k < 4; k++) {
        Bytes s = start(big);
        fill_to(s, seam_after(s, big, 0) + 9 + (size_t)(rnd() % 200));
        lit_rnd(s, 70000);
        tail3(s);
        N.lit_enter++;
        check(cn + "long literal " + std::to_string(k), s);
    }
    // literal bodies that parse as tokens (tests/test_gpu_k2j.py body_streams), with short copies into them
    for (const Bytes &fill : {Bytes{0x00}, Bytes{0x80, 0x80}, Bytes{0x7e}, Bytes{0xfc}, Bytes{0xfd}, Bytes{0xfe}, Bytes{0xff}}) {
        const int64_t n = 3000;
        Bytes s = start(big);
        tag(s, 0x00, n);
        for (int64_t k = 0; k < n; k++) s.push_back(fill[(size_t)k % fill.size()]);
        cpy(s, 100, 20), cpy(s, n - 1, 50), cpy(s, 1, 30), lit_rnd(s, 1), cpy(s, n / 2, 300);
        N.bodies++;
        check(cn + "body of " + std::to_string(fill[0]), s);
    }
    // padding runs from d bytes before a seam, and at the end of a stream that another one follows
    for (int n : {1, 15, 16, 17, 40}) {
        for (int d : {1, (n + 1) / 2, n}) {
            Bytes s = start(big);
            fill_to(s, seam_after(s, big, 0) - (size_t)d);
            s.insert(s.end(), (size_t)n, 0);
            tail3(s);
            N.pad_seam++;
            check(cn + "pad " + std::to_string(n) + " seam -" + std::to_string(d), s);
        }
        Bytes s = start(big);
        fill_to(s, seam_after(s, big, 0) - 5);
        tail3(s);
        s.insert(s.end(), (size_t)n, 0);
        N.pad_tail++;
        check(cn + "pad " + std::to_string(n) + " at the end", s);
    }
    // invalid streams: a MetaReset after output, a token before any MetaReset, a distance past a 1 KiB
    // window, a slot one byte short
    {
        Bytes s = start(big);
        fill_to(s, seam_after(s, big, 0) + 700);
        rst(s);
        lit_rnd(s, 40);  // (every cut keeps the MetaReset)
        tail3(s);
        N.late_reset++;
        check(cn + "late reset", s, true);
        Bytes f = start(big);  // (the first token of its chunk: only the scan's output before the chunk shows it)
        fill_to(f, seam_after(f, big, 0));
        rst(f), lit_rnd(f, 40), tail3(f);
        check(cn + "late reset at a seam", f, true);
        Bytes m;
        magic(m);
        lit_rnd(m, 40);
        if (big) lit_rnd(m, 100000);
        N.no_reset++;
        check(cn + "no reset", m);
        Bytes w = start(big, 10);
        lit_rnd(w, 2000);
        cpy(w, 1024, 20);   // (the window itself: taken)
        fill_to(w, seam_after(w, big, 0) + 40, 100);
        cpy(w, 1025, 20);
        tail3(w);
        if (want_of(w).err != OR_EOVERFLOW) fail(cn + "far distance", "the Reader does not report ErrOverflow");
        N.far_distance++;
        check(cn + "far distance", w);
        Bytes q = start(big);
        fill_to(q, seam_after(q, big, 0) + 300);
        tail3(q);
        const uint64_t need = want_of(q).out.size();
        N.short_slot++;
        if (run(cn + "short slot", between(Item{q, need - 1, true, nullptr}), false, 1)) fail(cn + "short slot", "taken");
        if (!run(cn + "exact slot", between(Item{q, need, false, nullptr}), false, 1)) fail(cn + "exact slot", "handed over");
    }
}

}  // namespace

int main() {
    g_out.resize(64 << 20);
    hdr(g_before), fill_to(g_before, 301), tail3(g_before);
    hdr(g_after), lit_rnd(g_after, 77), cpy(g_after, 5, 40);
    const std::vector<Form> fs = forms();
    streams_for_chunk(false, fs);
    streams_for_chunk(true, fs);
    for (int nbytes : {40000, 140000})  // tests/test_gpu_k2j.py phase_stream: speculation never meets the true chain
        for (int first : {12, 13}) {
            Bytes s;
            hdr(s);
            tag(s, 0x00, first);
            for (int k = 0; k < first; k++) s.push_back((uint8_t)(65 + k));
            while ((int)s.size() + 2 <= nbytes) s.push_back(0x86), s.push_back(0x05);
            g_phase = true;
            check("off-phase " + std::to_string(nbytes) + " / " + std::to_string(first), s);
            g_phase = false;
        }
    {  // batch shapes: three streams with lengths that are no chunk multiples, an empty one, a one-chunk one
        Bytes a = start(false), b = start(true), c = start(false), one = start(false);
        fill_to(a, 1000), tail3(a), fill_to(b, 103333), tail3(b), fill_to(c, 777), tail3(c), fill_to(one, 200);
        N.multi++;
        run("three streams", {Item{a, want_of(a).out.size() + 1, false, nullptr}, Item{b, want_of(b).out.size() + 2, false, nullptr}, Item{c, want_of(c).out.size(), false, nullptr}}, false, 0);
        run("three short streams", {Item{c, want_of(c).out.size() + 1, false, nullptr}, Item{a, want_of(a).out.size() + 2, false, nullptr}, Item{c, want_of(c).out.size(), false, nullptr}}, false, 0);
        N.empty++;
        check("empty", Bytes());
        run("empty alone", {Item{Bytes(), 0, false, nullptr}}, false, 0);
        N.one_chunk++;
        check("one chunk", one);
        run("one chunk alone", {Item{one, want_of(one).out.size(), false, nullptr}}, false, 0);
    }
#define P(f) K2_COUNT(N, 16, f)
    P(runs); P(streams); P(taken); P(handed_error); P(handed_design); P(jc256); P(jc1024); P(blocks); P(seams); P(lit_enter); P(passthrough);
    P(merged); P(repairs); P(phase_repairs); P(bodies); P(pad_seam); P(pad_tail); P(cuts); P(cuts_taken); P(cuts_handed_ok); P(c_on); P(stops);
    P(tails); P(multi); P(empty); P(one_chunk); P(late_reset); P(no_reset); P(far_distance); P(short_slot); P(breaks);
    std::printf("ok\n");
    return 0;
}
