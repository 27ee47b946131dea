// Host check of K2t's steps (eazy_amd/csrc/ez_k2_tok.h): the same source, compiled for the CPU, run
// step by step as ez_decompress_tok.hip's tok_one runs it, the 64 lanes emulated in order, on hand-built
// streams (tests/k2t_streams.py's groups T1, T2, T3, T5 and T7 restated with the C++ builder):
//   the window stage  per window the token-start list, the next entry p and the hand-over verdict equal
//                     one in-order k2_scan walk of the stream (every padding zero a token of its own);
//   the round stage   planning only, on a flat output buffer (no ring, far16, flush or deferral): nr, dst,
//                     total, fre / ys after the search and the batch boundaries from the header's
//                     functions; the literals written, each batch's copies executed once in lane order
//                     and once in reverse lane order (a copy's 16-byte steps in order, runs by pattern):
//                     both outputs equal the oracle's Reader (oracle/eazy_oracle.c), so a batch rule that
//                     lets dependent copies into one batch shows as a byte mismatch.
//   k2_tok_check      prints the count of every class, exits 1 at the first mismatch
// The emulated LDS arrays (the staged window; the advances, exits and entries) are exactly TLayout's
// sizes, allocated apart, and the second is poisoned before every window; the window is staged from a
// batch in which junk bytes follow the stream, as the next stream's do.  The wave-level loops (win_scan,
// win_walk, win_list, round_parse, alone_token, round_place, round_literals, round_copies) are mirrored
// serially below, each under the name of the step it mirrors.  Every stream runs with both rings'
// budgets, whole and cut at each of its last 27 bytes.
#include <algorithm>
#include <map>

#include "../eazy_amd/csrc/ez_k2_tok.h"
#include "k2_check_common.h"

using namespace k2check;
using namespace ez;

namespace {

struct Counts {
    uint64_t runs, windows, taken, handed_error, handed_design, seams, residues, rare_pairs, rare_steps, exit2_stops, stepped_over,
        empty_segments, pad_windows, clamped, bodies, lengths, cuts, cuts_taken, cuts_handed_ok, invalid, walk_handed, rounds, nr63, nr64,
        alone, cut_big, cut_budget, budget_edges, reset_off_lane0, code4, code5, code6, code7, code8, room_alone, slots, batches, chain64,
        searches, below_threshold, in_literal, redirect1, redirect2, unresolved, straddle, zero_len, source_edges, short_period, deferred;
} N;

[[noreturn]] void fail(const std::string &name, const char *what) {
    std::printf("MISMATCH %s: %s\n", name.c_str(), what);
    std::exit(1);
}

// a stream builder's own precondition does not hold
[[noreturn]] void die(int line) {
    std::printf("k2_tok_check.hip:%d: a stream is not built as intended\n", line);
    std::exit(2);
}

const int32_t kLim32 = k2_lim32(0);
constexpr size_t kJunk = 64;  // bytes of "the next stream" behind the stream under check

V16 at16(const uint8_t *p) {
    V16 v;
    std::memcpy(&v, p, 16);
    return v;
}

// ---- the wave's LDS: the staged window (TLayout: inb .. tab) and tab (the advances, the exits, the entries)
struct Lds {
    static constexpr size_t inb_bytes = TLayout<4096>::tab - TLayout<4096>::inb, tab_bytes = TLayout<4096>::defs - TLayout<4096>::tab;
    static_assert(inb_bytes == TLayout<8192>::tab - TLayout<8192>::inb && tab_bytes == TLayout<8192>::defs - TLayout<8192>::tab, "");
    uint8_t *inb, *tab;
    Lds() : inb((uint8_t *)std::malloc(inb_bytes)), tab((uint8_t *)std::malloc(tab_bytes)) {}
    ~Lds() {
        std::free(inb);
        std::free(tab);
    }
    uint16_t *ex() const { return (uint16_t *)(tab + kTWin); }
    uint16_t *ent() const { return (uint16_t *)(tab + 3 * kTWin); }
};

struct Win {
    std::vector<int32_t> starts;  // stream positions
    int32_t p;
    int code;
};

// ---- the window at the chain's entry w, as tok_one's first two stages run it
Win emu_window(Lds &m, const Bytes &batch, int32_t nb, int32_t w) {
    const int32_t base = w & ~15, limr = tk_limr(nb, base);
    uint16_t *ex = m.ex(), *ent = m.ent();
    Win r{{}, 0, 0};
    N.windows++;
    // win_scan: stage (zeros past the batch), the advances, the exits, the exits two steps on
    std::memset(m.tab, 0xcc, Lds::tab_bytes);
    for (int32_t k = 0; k < kTStage; k++) m.inb[k] = (size_t)(base + k) < batch.size() ? batch[(size_t)(base + k)] : 0;
    for (int lane = 0; lane < kWave; lane++) {
        uint4 a;
        uint32_t next, ad[4];
        std::memcpy(&a, m.inb + 16 * lane, 16);
        std::memcpy(&next, m.inb + 16 * lane + 16, 4);
        tk_advances(a, next, ad);
        std::memcpy(m.tab + 16 * lane, ad, 16);
        ent[lane] = kTNoEntry;
        tk_exits(ad, 16 * lane, tk_stop(16 * lane + 16, limr), ex);
    }
    {
        static uint16_t e2[kTWin];
        for (int32_t i = 0; i < kTWin; i++) {  // (every lane reads, a barrier, every lane writes)
            const int32_t y = ex[i];
            e2[i] = (uint16_t)tk_exit2(y, limr, ex);
            if (y < limr && ex[y] != y && ex[y] < tk_stop((y | 15) + 1, limr)) N.exit2_stops++;  // the landing's chain meets a rare form in its segment
        }
        std::memcpy(ex, e2, sizeof e2);
    }
    // win_walk
    int32_t e = w - base, sl = -1;
    while (e < limr) {
        const int32_t at = e, x = ex[e];
        tk_walk_step(e, sl, x, ex, ent, true, [&](int32_t q) { return tk_rare_adv(at16(m.inb + q), base + q, nb, kLim32, 0); });
        if (x == at) {
            N.rare_steps++;
            if (ex[at] == 0xffff) N.clamped++;
        }
    }
    r.code = tk_walk_code(base, e, nb);
    if (r.code) return r;
    r.p = base + e;
    // win_list: the marking from the walk's entries, the entries of the stepped-over segments, the marking from those
    uint32_t m16[kWave];
    int32_t q2[kWave];
    bool had[kWave];
    for (int lane = 0; lane < kWave; lane++) {
        const int32_t s0 = 16 * lane, se = s0 + 16, sm = tk_stop(se, limr);
        had[lane] = ent[lane] != kTNoEntry;
        q2[lane] = tk_entry_or(ent[lane], se);
        m16[lane] = 0;
        while (q2[lane] < sm) tk_mark_step(q2[lane], m16[lane], s0, m.tab, ex);
    }
    for (int lane = 0; lane < kWave; lane++) {
        const int32_t to = q2[lane] >> 4;
        const bool open = had[lane] && q2[lane] < limr && ent[to] == kTNoEntry;
        tk_fill_entry(had[lane], q2[lane], limr, ent);
        if (open && ent[to] == q2[lane]) N.stepped_over++;
    }
    for (int lane = 0; lane < kWave; lane++) {
        const int32_t s0 = 16 * lane, se = s0 + 16, sm = tk_stop(se, limr);
        if (!had[lane]) {
            q2[lane] = tk_entry_or(ent[lane], se);
            while (q2[lane] < sm) tk_mark_step(q2[lane], m16[lane], s0, m.tab, ex);
        }
        if (s0 + 16 <= limr && s0 >= w - base && m16[lane] == 0) N.empty_segments++;
        for (uint32_t b = m16[lane]; b; b &= b - 1) r.starts.push_back(base + s0 + (int32_t)__builtin_ctz(b));
    }
    return r;
}

// ---- the same window by one in-order walk: every padding zero a token, every other form by k2_scan
Win ref_window(const Bytes &batch, int32_t nb, int32_t w) {
    const int32_t base = w & ~15, end = base + tk_limr(nb, base);
    Win r{{}, w, 0};
    while (r.p < end) {
        r.starts.push_back(r.p);
        K2Tok t;
        if (batch[(size_t)r.p] == 0) {
            r.p += 1;
        } else if (k2_scan(at16(batch.data() + r.p), r.p, nb, kLim32, 0, t) == kParseHandOver) {
            r.code = kTokPast;
            return r;
        } else {
            r.p += t.adv;
        }
    }
    r.code = r.p > nb ? kTokPast : 0;
    return r;
}

// ---- the flat output: 16 bytes at x, zeros before the stream start; a copy's bytes
struct Flat {
    Bytes b;
    V16 ld(int32_t x) const {
        uint8_t t[16];
        for (int k = 0; k < 16; k++) t[k] = x + k >= 0 ? b[(size_t)(x + k)] : 0;
        return at16(t);
    }
    void st(int32_t x, V16 v, int32_t n) { std::memcpy(b.data() + x, &v, (size_t)(n < 16 ? n : 16)); }
    void copy(int32_t dst, int32_t ys, int32_t D, int32_t L) {
        if (D > 0 && D < 16) {  // a run: its pattern every run_step_of bytes
            const V16 pv = run_pattern(shr16(ld(dst - 16), (uint32_t)(16 - D)), (uint32_t)D);
            for (int32_t k = 0; k < L; k += run_step_of(D)) st(dst + k, pv, L - k);
        } else {  // 16-byte steps in order; a zero region's zeros
            for (int32_t k = 0; k < L; k += 16) st(dst + k, D == 0 ? V16{0, 0} : ld(ys + k), L - k);
        }
    }
};

struct State {
    int32_t pos, bsl;
    int nd;
};

// ---- the rounds of a window's token list, as tok_one's third stage plans them; fw / rv: the output with
// every batch's copies in lane order / in reverse lane order
int emu_rounds(const Lds &m, const Bytes &batch, int32_t nb, int32_t base, const std::vector<int32_t> &starts, State &S, int32_t cap, int32_t budget,
               Flat &fw, Flat &rv) {
    const int32_t cnt = (int32_t)starts.size();
    for (int32_t t0 = 0; t0 < cnt;) {
        // round_parse
        bool has[kWave], tok[kWave];
        int32_t q[kWave], L[kWave], incl[kWave], dst[kWave];
        V16 h[kWave];
        K2Tok tk[kWave];
        int rr[kWave];
        uint64_t rsts = 0, toks = 0, cut = 0;
        N.rounds++;
        for (int l = 0; l < kWave; l++) {
            has[l] = t0 + l < cnt;
            q[l] = base + (has[l] ? starts[(size_t)(t0 + l)] - base : 0);
            h[l] = at16(m.inb + (q[l] - base));
            const bool other = tk_parse_fast(h[l], kLim32, tk[l]);
            rr[l] = kParseToken;
            if (has[l] && other) rr[l] = k2_scan(h[l], q[l], nb, kLim32, 0, tk[l]);
            rr[l] = has[l] ? rr[l] : kParseSkip;
            if (rr[l] == kParseHandOver) return kTokForm;
            tok[l] = rr[l] == kParseToken;
            rsts |= (uint64_t)(rr[l] == kScanReset) << l;
            toks |= (uint64_t)tok[l] << l;
        }
        if (rsts) {
            if (const int code = tk_reset_code(S.pos, rsts, toks)) return code;
            S.bsl = (int32_t)tk[__builtin_ctzll(rsts)].marg;
            if (__builtin_ctzll(rsts) != 0) N.reset_off_lane0++;
        }
        if (const int code = tk_window_code(S.bsl, toks)) return code;
        for (int l = 0, sum = 0; l < kWave; l++) {
            L[l] = tok[l] ? tk[l].L : 0;
            incl[l] = sum += L[l];
            cut |= (uint64_t)tk_cut(has[l], tok[l], L[l], incl[l], budget) << l;
        }
        const int32_t nr = tk_round_len(cut, cnt - t0);
        if (cut) {
            const int f = (int)__builtin_ctzll(cut);
            (tok[f] && L[f] > kTBig ? N.cut_big : N.cut_budget)++;
            if (!(tok[f] && L[f] > kTBig) && incl[f] == budget + 1) N.budget_edges++;
        }
        if (nr > 0 && incl[nr - 1] >= budget - 1) N.budget_edges++;
        N.nr63 += nr == 63, N.nr64 += nr == 64;
        if (nr == 0) {
            // alone_token
            const int32_t L0 = L[0], D0 = (int32_t)tk[0].D, src0 = q[0] + tk[0].j, pos = S.pos;
            const bool cp0 = tk[0].cp;
            if (const int code = tk_alone_code(pos, L0, cap, cp0, (uint32_t)D0, S.bsl)) return code;
            N.alone++;
            if (tk_defers(cp0, L0, S.nd, true)) S.nd++, N.deferred++;
            if (!cp0 || D0 == 0 || D0 >= 16) {
                const int32_t W = tk_alone_width(cp0, D0);
                for (int32_t done = 0; done < L0; done += W) {  // (every lane reads, then every lane writes)
                    V16 v[kWave];
                    for (int l = 0; l < kWave; l++)
                        if (16 * l < W && done + 16 * l < L0) v[l] = !cp0 ? at16(batch.data() + src0 + done + 16 * l) : (D0 ? fw.ld(pos - D0 + done + 16 * l) : V16{0, 0});
                    for (int l = 0; l < kWave; l++)
                        if (16 * l < W && done + 16 * l < L0) fw.st(pos + done + 16 * l, v[l], L0 - done - 16 * l);
                }
            } else {
                fw.copy(pos, pos - D0, D0, L0);
            }
            std::memcpy(rv.b.data() + pos, fw.b.data() + pos, (size_t)L0);
            S.pos += L0;
            t0 += 1;
            continue;
        }
        // round_place
        const int32_t total = incl[nr - 1], pos = S.pos;
        uint64_t far = 0;
        for (int l = 0; l < kWave; l++) {
            dst[l] = pos + incl[l] - L[l];
            far |= (uint64_t)(l < nr && tok[l] && tk_past_window(tk[l].cp, tk[l].D, S.bsl)) << l;
        }
        if (const int code = tk_room_code(pos, total, cap)) return code;
        if (const int code = tk_far_code(far)) return code;
        // round_literals
        for (int l = 0; l < nr; l++)
            if (tok[l] && !tk[l].cp) {
                std::memcpy(fw.b.data() + dst[l], batch.data() + q[l] + tk[l].j, (size_t)L[l]);
                std::memcpy(rv.b.data() + dst[l], batch.data() + q[l] + tk[l].j, (size_t)L[l]);
            }
        // round_copies: the plan
        bool in[kWave], cpy[kWave], fre[kWave], open[kWave], redir[kWave];
        int32_t D[kWave], cs[kWave], need[kWave], ys[kWave], ye[kWave], tend[kWave], tinf[kWave], nred[kWave];
        uint64_t cm = 0;
        int nopen = 0;
        for (int l = 0; l < kWave; l++) {
            in[l] = l < nr && tok[l];
            cpy[l] = in[l] && tk[l].cp;
            D[l] = (int32_t)tk[l].D;
            cs[l] = ys[l] = dst[l] - D[l];
            need[l] = ye[l] = tk_need(D[l], cs[l], L[l]);
            fre[l] = tk_free0(cpy[l], D[l], need[l], pos);
            open[l] = cpy[l] && !fre[l];
            redir[l] = tk_redir(D[l], L[l]);
            tend[l] = tk_tend(in[l], dst[l], L[l]);
            tinf[l] = tk_tinf(in[l], tk[l].cp, D[l]);
            nred[l] = 0;
            cm |= (uint64_t)cpy[l] << l;
            nopen += open[l];
            if (cpy[l] && D[l] > 0 && D[l] < 16) N.short_period++;
        }
        if (nopen == kTSearchMin - 1) N.below_threshold++;
        if (nopen >= kTSearchMin) {
            N.searches++;
            for (int it = 0; it < kTSearchSteps; it++)
                for (int l = 0; l < kWave; l++) {
                    if (!open[l]) continue;
                    int t = 0;
                    for (int st = 16; st > 0; st >>= 2) t = tk_owner_step(t, st, dst[t + st], dst[t + 2 * st], dst[t + 3 * st], ys[l]);
                    const int32_t y0 = ys[l];
                    const bool inside = ys[l] >= pos && ye[l] <= tend[t] && t < l;
                    tk_redirect(ys[l], ye[l], fre[l], open[l], pos, tend[t], tinf[t], t, l, redir[l]);
                    if (!inside && y0 >= pos) N.straddle++;
                    if (inside && tinf[t] < 0) N.in_literal++;
                    if (t > 0 && dst[t - 1] == dst[t] && inside) N.zero_len++;  // lanes without output share the holder's dst
                    if (ys[l] != y0) nred[l]++;
                    if (!open[l] && fre[l] && nred[l] == 1 && ys[l] != y0) N.redirect1++;
                    if (!open[l] && fre[l] && nred[l] == 2 && ys[l] != y0) N.redirect2++;
                }
            for (int l = 0; l < kWave; l++)
                if (open[l]) ys[l] = cs[l], N.unresolved++;
        }
        // round_copies: the batches
        int nbatch = 0;
        while (cm) {
            const int a = (int)__builtin_ctzll(cm);
            const int32_t oa = dst[a];
            uint64_t brk = 0, exm = 0;
            for (int l = 0; l < kWave; l++) brk |= (uint64_t)tk_breaks((cm >> l) & 1, fre[l], l, a, need[l], oa) << l;
            const int bnd = brk ? (int)__builtin_ctzll(brk) : kWave;
            for (int l = 0; l < kWave; l++) exm |= (uint64_t)tk_runs((cm >> l) & 1, fre[l], l, bnd) << l;
            for (int l = 0; l < kWave; l++)
                if ((exm >> l) & 1) fw.copy(dst[l], ys[l], D[l], L[l]);
            for (int l = kWave - 1; l >= 0; l--)
                if ((exm >> l) & 1) rv.copy(dst[l], ys[l], D[l], L[l]);
            cm &= ~exm;
            nbatch++;
        }
        N.batches += (uint64_t)nbatch;
        if (nbatch == 64) N.chain64++;
        S.pos += total;
        t0 += nr;
    }
    return 0;
}

// the oracle's Reader on a stream: its error and its output
struct Want {
    int err;
    Bytes out;
};
Want reader(const Bytes &s) {
    int64_t olen = 0;
    const int err = oracle(s.data(), s.size(), 0, olen);
    return Want{err, Bytes(g_out.begin(), g_out.begin() + olen)};
}

// ---- one stream in a slot of cap bytes with a ring's budget, as tok_one: its hand-over code (0: taken)
int run_one(const std::string &name, const Bytes &s, int32_t cap, int32_t budget, const Want &want) {
    static Lds m;
    static Flat fw, rv;
    Bytes batch = s;
    for (size_t k = 0; k < kJunk; k++) batch.push_back((uint8_t)(0x81 + 7 * k));  // (the next stream's bytes: no zeros)
    N.runs++;
    if (const int code = tk_args_code((int64_t)batch.size(), (int64_t)s.size(), cap)) return code;
    batch.insert(batch.end(), kTStage + 32, 0);  // (beyond the batch: never read as bytes of it)
    batch.resize(batch.size());
    const int32_t nb = (int32_t)s.size();
    fw.b.assign((size_t)cap + 64, 0xa5);
    rv.b.assign((size_t)cap + 64, 0xa5);
    State S{0, -1, 0};
    // (the kernel's staging reads zeros past the batch, the in-order walk the same bytes)
    Bytes staged(batch.begin(), batch.begin() + (long)(s.size() + kJunk));
    for (int32_t w = 0; w < nb;) {
        const Win got = emu_window(m, staged, nb, w), ref = ref_window(batch, nb, w);
        if (got.code != ref.code) fail(name, got.code ? "the walk hands over, the in-order walk does not" : "the in-order walk hands over, the walk does not");
        if (got.code) {
            N.walk_handed++;
            return got.code;
        }
        if (got.starts != ref.starts) fail(name, "a window's token starts differ from the in-order walk's");
        if (got.p != ref.p) fail(name, "a window's next entry differs from the in-order walk's");
        if (const int code = emu_rounds(m, batch, nb, w & ~15, got.starts, S, cap, budget, fw, rv)) return code;
        w = got.p;
    }
    if (want.err != 0) fail(name, "taken, but the Reader reports an error");
    if ((size_t)S.pos != want.out.size()) fail(name, "taken, but not the Reader's size");
    if (!std::equal(want.out.begin(), want.out.end(), fw.b.begin())) fail(name, "bytes differ from the Reader's (batches in lane order)");
    if (!std::equal(want.out.begin(), want.out.end(), rv.b.begin())) fail(name, "bytes differ from the Reader's (batches in reverse lane order)");
    return 0;
}

const int32_t kBudgets[2] = {TLayout<4096>::budget, TLayout<8192>::budget};

// the stream whole and cut at each of its last 27 bytes, with both budgets.  expect: the code it must
// hand over with (0: taken; -1: the Reader's verdict decides); design: handed over though the Reader accepts it
void check(const std::string &name, const Bytes &s, int expect = -1, bool design = false, int64_t slot = -1) {
    const Want want = reader(s);
    const int32_t cap = (int32_t)(slot >= 0 ? slot : std::max<size_t>(want.out.size() + (want.err ? 80000 : 5), 16));
    for (int32_t budget : kBudgets) {
        const int code = run_one(name, s, cap, budget, want);
        if (expect >= 0 && (code & 0xff) != expect) fail(name, "not the expected hand-over code");
        if (code == 0) N.taken++;
        else if (want.err != 0) N.handed_error++;
        else if (design) N.handed_design++;
        else fail(name, "handed over, but the Reader accepts it and no design rule hands it over");
        if (design && code == 0) fail(name, "taken, but built to be handed over");
        const int c = code & 0xff;
        N.code4 += c == kTokReset, N.code5 += c == kTokNoWindow, N.code6 += code == kTokAlone, N.code7 += c == kTokRoom, N.code8 += c == kTokFar;
        N.room_alone += code == (kTokAlone | kTokRoomFlag);
    }
    for (size_t cut = 1; cut <= 27 && cut <= s.size(); cut++) {
        const Bytes t(s.begin(), s.end() - (long)cut);
        const Want wt = reader(t);
        const std::string nm = name + " cut " + std::to_string(cut);
        for (int32_t budget : kBudgets) {
            N.cuts++;
            const int code = run_one(nm, t, cap, budget, wt);
            if (code == 0) N.cuts_taken++;
            else if (wt.err == 0) N.cuts_handed_ok++;  // (a cut the Reader reads to a clean end)
        }
    }
}

// ---- a stream under construction: its bytes and its output position
struct SB {
    Bytes c;
    int64_t pos = 0;
    explicit SB(bool header = true, int bsl = 0x14) {
        if (header) hdr(c, bsl);
    }
    SB &lit(int64_t n) {
        lit_rnd(c, n);
        pos += n;
        return *this;
    }
    SB &cpy(int64_t d, int64_t n, bool lng = false) {
        (lng ? cpy_long : k2check::cpy)(c, d, n);
        pos += n;
        return *this;
    }
    SB &src(int64_t at, int64_t n, bool lng = false) { return cpy(pos - at, n, lng); }  // a copy whose source starts at output position at
    SB &zeros(size_t n) {
        c.insert(c.end(), n, 0);
        return *this;
    }
    SB &brk() {
        meta(c, 3 << 3, "", 0);
        return *this;
    }
    SB &raw(const Bytes &b) {  // (pos is not kept: the window-stage streams do not need it)
        put(c, b);
        return *this;
    }
    // short literals and copies up to exactly input offset target
    SB &to(size_t target) {
        if (c.size() > target) die(__LINE__);
        while (c.size() < target) {
            const size_t left = target - c.size();
            if (left == 1) zeros(1);
            else if (left <= 100) lit((int64_t)left - 1);
            else if (rnd() % 3 == 0) cpy(1 + (int64_t)(rnd() % 200), 4 + (int64_t)(rnd() % 60));
            else lit(1 + (int64_t)(rnd() % 60));
        }
        return *this;
    }
    // (base, end) of the scan window that holds the next token's start
    std::pair<size_t, size_t> window() const {
        Bytes z = c;
        z.insert(z.end(), 32, 0);
        std::vector<size_t> pts;
        for (size_t p = 0; p < c.size();) {
            K2Tok t;
            pts.push_back(p);
            if (z[p] == 0) p += 1;
            else if (k2_scan(at16(z.data() + p), (int32_t)p, (int32_t)c.size(), kLim32, 0, t) == kParseHandOver) die(__LINE__);
            else p += (size_t)t.adv;
        }
        pts.push_back(c.size());
        for (size_t w = 0;;) {
            const size_t base = w & ~(size_t)15;
            auto it = std::lower_bound(pts.begin(), pts.end(), base + kTWin);
            if (it == pts.end()) return {base, base + kTWin};
            w = *it;
        }
    }
    // literals up to the end of the current window: the next token opens a window
    SB &new_window() {
        const size_t end = window().second;
        return to(end >= c.size() + 2 ? end : end + kTWin);
    }
    SB &trailer() { return lit(4).cpy(3, 12); }
};

SB first(const Form &f) {
    SB s;
    if (f.big_first) s.lit(70000);
    return s;
}

// ---------------------------------------------------------------- the window stage's streams
void window_streams(const std::vector<Form> &fs) {
    for (const Form &f : fs) {
        // its first byte d = 0 .. min(its length, 16) bytes before the end of the first window and of a drifted second one
        for (size_t d = 0; d <= std::min<size_t>(f.b.size(), 16); d++) {
            SB s = first(f).lit(600);
            s.to(s.window().second - d).raw(f.b).trailer();
            N.seams++;
            check(std::string("seam first ") + f.name + " -" + std::to_string(d), s.c);
            SB t = first(f).lit(600);
            const size_t end = t.window().second;
            t.to(end - 24).lit(200);  // straddles the window's end: the next window starts past it
            const auto w2 = t.window();
            const size_t e = end - 24 + 2 + 200 - w2.first;  // the chain's entry into it, past its base
            if (w2.first <= end || w2.second % 1024 == 0 || e < 1 || e > 15) die(__LINE__);
            t.to(w2.second - d).raw(f.b).trailer();
            N.seams++;
            check(std::string("seam drift ") + f.name + " -" + std::to_string(d), t.c);
        }
        // at each residue of a lane segment, short tokens before it
        for (size_t r = 0; r < 16; r++) {
            SB s = first(f).lit(600);
            s.to((s.c.size() + 40) / 16 * 16 + 16 + r).raw(f.b).trailer();
            N.residues++;
            check(std::string("residue ") + f.name + " " + std::to_string(r), s.c);
        }
    }
    // two rare forms back to back
    for (const Form &a : fs)
        for (const Form &b : fs) {
            const auto rare = [](const Form &f) { return !f.big_first && f.b.size() < 60000 && f.b[0] != 0 && std::string(f.name) != "lit_len0" && std::string(f.name).rfind("cpy_plain", 0) && std::string(f.name).rfind("cpy_off", 0); };
            if (!rare(a) || !rare(b)) continue;
            SB s;
            s.lit(700).raw(a.b).raw(b.b).trailer();
            N.rare_pairs++;
            check(std::string("pair ") + a.name + " + " + b.name, s.c);
        }
    // a first exit that lands in a segment whose chain meets a rare form before leaving it, at every offset of the landing
    for (size_t r = 0; r < 14; r++) {
        SB s;
        s.lit(300);
        const size_t a = (s.c.size() + 40) / 16 * 16 + 32;
        s.to(a - 6).lit(5 + (int64_t)r);  // lands at a + r
        s.lit(1).lit(200).trailer();       // a + r + 2: Len1, a rare form, in the landing's segment
        check("landing before a rare form " + std::to_string(r), s.c);
    }
    // long literal bodies: whole segments without a chain position; bodies that parse as tokens are never marked
    for (const Bytes &fill : {Bytes{0x00}, Bytes{0x80, 0x80}, Bytes{0x7e}, Bytes{0xfc}, Bytes{0xfd}, Bytes{0xfe}, Bytes{0xff}, Bytes{0x05, 0x86}}) {
        SB s;
        s.lit(40);
        tag(s.c, 0x00, 3000);
        for (int64_t k = 0; k < 3000; k++) s.c.push_back(fill[(size_t)k % fill.size()]);
        s.pos += 3000;
        s.cpy(100, 20).cpy(2999, 50).cpy(1, 30).lit(1).cpy(1500, 300).trailer();
        N.bodies++;
        check("body of " + std::to_string(fill[0]), s.c);
    }
    // a literal that advances 65,536 + 20 bytes from the middle of a window, its body full of literal tags: the exit clamp
    for (size_t at : {500, 511, 512}) {
        SB s;
        s.lit(300).to(at);
        tag(s.c, 0x00, 65553);
        for (int64_t k = 0; k < 65553; k++) s.c.push_back(k % 124 == 17 ? 0x7b : (uint8_t)rnd());
        check("advance 65556 at " + std::to_string(at), s.trailer().c);
    }
    // a window of 1,024 padding zeros; padding runs across segment and window seams
    {
        SB s;
        s.lit(500).new_window().zeros(1024).lit(30).cpy(17, 40).trailer();
        N.pad_windows++;
        check("window of zeros", s.c);
        for (size_t n : {1, 15, 16, 17, 40})
            for (size_t d : {(size_t)1, (n + 1) / 2, n}) {
                SB t;
                t.lit(500);
                t.to(t.window().second - d).zeros(n).trailer();
                check("pad " + std::to_string(n) + " seam -" + std::to_string(d), t.c);
            }
        SB z(false);
        z.zeros(100);
        hdr(z.c);
        N.pad_windows++;
        check("100 zeros before the header", z.lit(50).cpy(20, 30).trailer().c);
    }
    // lengths around a window, one under 16, one no multiple of 16
    for (size_t nb : {1023, 1024, 1025, 12, 1500}) {
        SB s;
        s.to(nb);
        N.lengths++;
        check("length " + std::to_string(nb), s.c);
    }
    // the forms k2_scan hands over, in the middle of a window: the walk's verdict, kTokPast
    const std::vector<std::pair<const char *, Bytes>> bad = {
        {"tag 127", {0x7f, 1, 2, 3, 4, 5}},
        {"offset byte 255", {0x85, 0xff, 0xff, 1, 2}},
        {"4-byte length 2^30", {0x7e, 0, 0, 0, 0x40, 1}},
        {"4-byte offset 2^30", {0x85, 0xfe, 0, 0, 0, 0x40}},
        {"unsupported meta", {0x80, (5 << 3) | 0, 7}},
        {"wide meta", {0x80, (3 << 3) | 6, 1, 2, 3}},
    };
    for (const auto &b : bad) {
        SB s;
        s.lit(300).to(700).raw(b.second).trailer();
        N.invalid++;
        check(std::string("invalid: ") + b.first, s.c, kTokPast);
    }
}

// ---------------------------------------------------------------- the round stage's streams
void round_streams() {
    // windows of exactly 63, 64 and 65 tokens (1-byte literals)
    for (int n : {63, 64, 65}) {
        SB s;
        s.lit(500).new_window();
        for (int k = 0; k < n - 1; k++) s.lit(1);
        s.lit((int64_t)(s.window().second - s.c.size()) + 50);
        check("window of " + std::to_string(n) + " tokens", s.trailer().c);
    }
    // tokens of 511, 512 and 513 bytes: 513 is moved alone
    for (int64_t L : {kTBig - 1, kTBig, kTBig + 1}) {
        check("lit " + std::to_string(L), SB().lit(100).lit(L).trailer().c);
        check("cpy " + std::to_string(L), SB().lit(700).cpy(600, L).trailer().c);
        check("cpy overlap " + std::to_string(L), SB().lit(700).cpy(40, L).trailer().c);
        check("run " + std::to_string(L), SB().lit(100).cpy(3, L).trailer().c);
        check("zero region " + std::to_string(L), SB().lit(100).cpy(0, L).trailer().c);
    }
    check("lit 16384 (deferred)", SB().lit(100).lit(16384).cpy(16384 + 50, 30).cpy(20, 600).trailer().c);
    // rounds whose running output reaches budget - 1, budget and budget + 1; a 512-byte token that ends on the budget
    for (int32_t budget : kBudgets) {
        const int n512 = (budget - 448) / 512;
        for (int delta : {-1, 0, 1}) {
            SB s;
            s.lit(650).new_window();
            for (int k = 0; k < n512; k++) s.cpy(520 + 13 * k, 512);
            s.lit(100).cpy(555, 348 + delta);
            for (int k = 0; k < 10; k++) s.lit(2).cpy(700 + k, 30);
            check("budget " + std::to_string(budget) + " " + std::to_string(delta), s.trailer().c);
        }
        SB s;
        s.lit(650).new_window().lit(100).cpy(555, 348);
        for (int k = 0; k < n512; k++) s.cpy(520 + 13 * k, 512);
        check("512 lands on budget " + std::to_string(budget), s.lit(5).cpy(530, 512).trailer().c);
    }
    // MetaReset on another lane than 0; two resets; a token before any reset; distances beyond the window
    {
        SB s(false);
        magic(s.c);
        s.zeros(5);
        rst(s.c);
        check("magic padding reset", s.lit(50).cpy(20, 30).trailer().c);
        SB two;
        rst(two.c, 0x12);
        check("two resets", two.lit(50).cpy(20, 30).trailer().c, kTokReset, true);
        SB late;
        late.lit(40);
        rst(late.c);
        check("reset after output", late.lit(40).trailer().c, kTokReset, true);
        SB none(false);
        magic(none.c);
        check("no reset", none.lit(40).trailer().c, kTokNoWindow);
        check("far distance in a round", SB(true, 10).lit(400).lit(400).lit(400).cpy(1024, 20).lit(3).cpy(1025, 20).trailer().c, kTokFar);
        check("far distance alone", SB(true, 10).lit(400).lit(400).lit(400).cpy(1024, 600).lit(3).cpy(1025, 600).trailer().c, kTokAlone);
    }
    // a slot exactly enough and one byte short, at a token of a round and at a token moved alone
    for (int64_t L : {40, 512, 513, 2000})
        for (bool cp : {true, false}) {
            SB s;
            s.lit(700).lit(5).cpy(100, 30);
            if (cp) s.cpy(600, L);
            else s.lit(L);
            const std::string nm = std::string("slot ") + (cp ? "cpy " : "lit ") + std::to_string(L);
            N.slots++;
            check(nm + " exact", s.c, 0, false, s.pos);
            check(nm + " short", s.c, L > kTBig ? kTokAlone : kTokRoom, true, s.pos - 1);
        }
    // a copy source ending at, and past, an earlier copy's first byte (the batch rule need > oa)
    for (int past : {0, 1, 2, 15, 16, 17})
        for (int64_t L : {5, 16, 20, 33}) {
            SB s;
            s.lit(700).new_window();
            const int64_t oa = s.pos;
            s.cpy(600, 40).lit(30).src(oa - L + past, L);
            N.source_edges++;
            check("source ends " + std::to_string(past) + " past L" + std::to_string(L), s.lit(3).cpy(50, 20).trailer().c);
        }
    for (int64_t D : {15, 16, 17})
        for (int64_t L : {D + 1, (int64_t)40, (int64_t)300})
            check("D" + std::to_string(D) + " L" + std::to_string(L), SB().lit(700).new_window().cpy(600, 30).cpy(D, L).lit(2).cpy(D, L).trailer().c);
    // 64 copies in one round, each reading the one before: 64 batches
    for (int64_t L : {1, 16, 20}) {
        SB s;
        s.lit(700).new_window().lit(600);  // (moved alone: the copies start a round)
        for (int k = 0; k < 64; k++) s.cpy(L, L);
        check("chain 64 L" + std::to_string(L), s.trailer().c);
    }
    {
        SB s;
        s.lit(700).new_window().lit(600);
        for (int k = 0; k < 64; k++) s.cpy(24 + (k % 3), 20 + (k % 5));
        check("chain 64 mixed", s.trailer().c);
    }
    // 15 and 16 copies reading the round's own output: the search's threshold
    for (int n : {15, 16}) {
        SB s;
        s.lit(700).new_window();
        const int64_t a = s.pos;
        s.lit(60);
        for (int k = 0; k < n; k++) s.src(a + 2 + k, 20);
        check(std::to_string(n) + " copies of the round's output", s.trailer().c);
    }
    // redirects once, twice and three deep (the third stays unresolved), in a round that searches
    {
        SB s;
        s.lit(700).new_window();
        const int64_t before = s.pos - 300, a = s.pos;
        s.lit(60);
        for (int k = 0; k < 16; k++) s.src(a + 2 + k, 20);
        const int64_t c1 = s.pos;
        s.src(before, 40);  // final at the round's start
        const int64_t c2 = s.pos;
        s.src(c1 + 3, 30);  // once: into c1's source, before the round
        const int64_t c3 = s.pos;
        s.src(c2 + 2, 20);  // twice
        const int64_t c4 = s.pos;
        s.src(c3 + 1, 16);  // three deep: unresolved
        s.src(c4, 16);
        check("redirects one, two and three deep", s.trailer().c);
    }
    // sources inside a literal of the round, inside a copy, straddling two tokens; zero-length tokens between tokens that share a dst
    for (int gap = 0; gap < 3; gap++) {
        SB s;
        s.lit(700).new_window();
        for (int k = 0; k < 7; k++) {
            const int64_t a = s.pos;
            s.lit(40);
            if (gap == 1) s.zeros(1 + (size_t)k % 3);
            if (gap == 2) s.brk();
            const int64_t b = s.pos;
            s.src(a + 5, 20);
            const int64_t c = s.pos;
            s.src(b + 2, 16);
            const int64_t d = s.pos;
            s.src(c, 16).src(a + 30, 20).src(d - 8, 24);
            if (gap == 1) s.zeros(2);
            s.src(b + 1, 19, true);
        }
        check(std::string("own output ") + (gap == 0 ? "plain" : gap == 1 ? "pad" : "brk"), s.trailer().c);
    }
}

}  // namespace

int main() {
    g_out.resize(64 << 20);
    window_streams(forms());
    round_streams();
#define P(f) K2_COUNT(N, 16, f)
    P(runs); P(windows); P(taken); P(handed_error); P(handed_design); P(seams); P(residues); P(rare_pairs); P(rare_steps); P(exit2_stops);
    P(stepped_over); P(empty_segments); P(pad_windows); P(clamped); P(bodies); P(lengths); P(cuts); P(cuts_taken); P(cuts_handed_ok); P(invalid);
    P(walk_handed); P(rounds); P(nr63); P(nr64); P(alone); P(cut_big); P(cut_budget); P(budget_edges); P(reset_off_lane0); P(code4); P(code5);
    P(code6); P(code7); P(code8); P(room_alone); P(slots); P(batches); P(chain64); P(searches); P(below_threshold); P(in_literal); P(redirect1);
    P(redirect2); P(unresolved); P(straddle); P(zero_len); P(source_edges); P(short_period); P(deferred);
    std::printf("ok\n");
    return 0;
}
