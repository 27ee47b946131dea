// ez_k2_tok.h — what a lane of K2t computes (ez_decompress_tok.hip: token-parallel decode, one wave per
// stream), its constants and its LDS layout.
//
// The functions are arithmetic on a lane's own values and on arrays it is handed (the staged window,
// the advances, the exits ex, the entries ent: LDS in the kernel, host arrays in tools/k2_tok_check.hip,
// which runs the same source over emulated lanes against the oracle).  Staging, barriers, ballots,
// lane exchanges, atomics, the ring and the stores are the kernel's.
//   window stage   tk_advances (swar_adv), tk_exits, tk_exit2, tk_walk_step (tk_rare_adv), tk_walk_code, tk_entry_or,
//                  tk_mark_step, tk_fill_entry;
//   round stage    tk_parse_fast, tk_cut, tk_round_len, tk_need, tk_free0, tk_owner_step, tk_redirect,
//                  tk_breaks, tk_runs, tk_slow, run_step_of, tk_alone_width, tk_defers;
//   hand-overs     tk_args_code .. tk_far_code: each check returns its code (TokCode), 0 to go on.
#pragma once

#include "ez_internal.h"
#include "ez_k2_parse.h"
#include "ez_k2_ring.h"
#include "ez_wave.h"

namespace ez {

constexpr int32_t kTWin = 1024;                 // input positions scanned per window (16 per lane)
constexpr int32_t kTStage = kTWin + 96;         // staged input bytes: a header at the window's end reads 16 more
constexpr int32_t kTBig = 512;                  // tokens longer than this are moved alone by the whole wave
constexpr int32_t kTOver = 1 << 30;             // tk_rare_adv: a form to hand over (past any stream)
constexpr int32_t kTNoEntry = 0xffff;           // ent: the chain has not entered the segment

template <int32_t R>
struct TLayout {
    static constexpr int32_t ring = 16;          // [16 guard][R][16 mirror][16 guard]
    static constexpr int32_t inb = R + 48;       // the staged input window
    // tab: the scan's advances (kTWin bytes; per-lane write trash during the rounds), the segment
    // exits (u16 x kTWin; then the token list), the segment entries (u16 x 64)
    static constexpr int32_t tab = inb + kTStage;
    static constexpr int32_t defs = tab + 3 * kTWin + 2 * kWave;  // the stream's deferred literals (3 x int32 each)
    static constexpr int32_t bytes = defs + 12 * kDefSlots;
    // output bytes of one round at most: the round's writes never reach a ring slot it reads, and
    // a source farther back than the ring is already in HBM (unflushed output stays < 1 KiB)
    static constexpr int32_t budget = R - 1024 - 64;
    static_assert(budget >= kTBig, "a round must hold any token that is not moved alone");
    static_assert(kDeferMin > R, "a deferred literal refills the whole ring");
};

// Why a stream is handed to the exact decoder (debug builds store 100 + code as its status).
// kTokRoomFlag: the output needs more than the slot (the caller that sizes the slot itself is told)
enum TokCode : int {
    kTokArgs = 1,      // argument bounds
    kTokPast = 2,      // the last token runs past the input, or a form the full parse hands over (walk)
    kTokForm = 3,      // a form the full parse hands over (round)
    kTokReset = 4,     // a MetaReset after output, two of them, or a token before it in the round
    kTokNoWindow = 5,  // a token before any MetaReset
    kTokAlone = 6,     // a token moved alone: room, or a distance beyond the window
    kTokRoom = 7,      // a round: room
    kTokFar = 8,       // a round: a distance beyond the window
    kTokRoomFlag = 0x100,
};

// ---------------------------------------------------------------- the window stage

EZ_HD uint32_t fanout(uint32_t f) { return f | (f - (f >> 7)); }  // bit 7 of a byte -> 0xff

// Input bytes a token starting at each of 4 positions takes: X = bytes x .. x+3, Y = bytes
// x+1 .. x+4.  The common forms (reader.go:346-392, 422-472): a literal with a 1-byte tag
// (length < 124; a zero byte is padding, one byte), a copy with a 1-byte tag and a plain, Off1
// or Off2 offset.  0 for the others (Len1/Len2/Len4 tags, metas, Off4 and OffLong offsets).
EZ_HD uint32_t swar_adv(uint32_t X, uint32_t Y) {
    const uint32_t X7 = X & 0x7f7f7f7fu, Y7 = Y & 0x7f7f7f7fu;
    const uint32_t isc = X & 0x80808080u;                         // a copy's (or meta's) tag
    const uint32_t lit = X7 + 0x01010101u;                         // 1 + length
    const uint32_t ge252 = (Y7 + 0x04040404u) & Y & 0x80808080u;  // offset byte >= 252
    const uint32_t ge254 = (Y7 + 0x02020202u) & Y & 0x80808080u;  // >= 254: Off4, OffLong
    const uint32_t cpy = 0x02020202u + (((Y & 0x03030303u) + 0x01010101u) & fanout(ge252));
    const uint32_t mc = fanout(isc);
    const uint32_t adv = (cpy & mc) | (lit & ~mc);
    const uint32_t lwide = (X7 + 0x04040404u) & 0x80808080u;      // length byte >= 124
    const uint32_t nz = (X7 + 0x7f7f7f7fu) & 0x80808080u;         // low 7 bits nonzero (else 0x80: meta)
    const uint32_t rare = lwide | (isc & ~nz) | (isc & ge254);
    return adv & ~fanout(rare);
}

// positions walked in the window at base: up to the window's end or the stream's
EZ_HD int32_t tk_limr(int32_t nb, int32_t base) { return (nb < base + kTWin ? nb : base + kTWin) - base; }
// where a chain through the segment ending at se stops: the segment's end or the window's
EZ_HD int32_t tk_stop(int32_t se, int32_t limr) { return se < limr ? se : limr; }

// a lane's four advance words (a byte per position of its segment) from the segment's 16 staged
// bytes a and the 4 bytes after them
EZ_HD void tk_advances(uint4 a, uint32_t next, uint32_t ad[4]) {
    ad[0] = swar_adv(a.x, k2_alignbyte1(a.y, a.x));
    ad[1] = swar_adv(a.y, k2_alignbyte1(a.z, a.y));
    ad[2] = swar_adv(a.z, k2_alignbyte1(a.w, a.z));
    ad[3] = swar_adv(a.w, k2_alignbyte1(next, a.w));
}

// Segment exits, backwards through the lane's 16 positions [s0, s0 + 16): ex[p] = the first
// position at or past sx (the segment's end or the window's) that a chain through p reaches, or
// the first rare form on the way (p itself when it is one); offsets from the window's base
EZ_HD void tk_exits(const uint32_t ad[4], int32_t s0, int32_t sx, uint16_t *ex) {
#pragma unroll
    for (int j = 15; j >= 0; j--) {
        const int32_t a = (int32_t)((ad[j >> 2] >> (8 * (j & 3))) & 0xff);
        const int32_t pj = s0 + j, n = pj + a;
        const int32_t in_seg = ex[n < sx ? n : pj];  // (written already when n < sx)
        ex[pj] = (uint16_t)(a == 0 ? pj : (n >= sx ? n : in_seg));
    }
}

// The exit two steps on of an exit y: the exit of y when y lies in the window and the chain through
// y leaves y's segment (no rare form on the way: it stops at the landing), else y
EZ_HD int32_t tk_exit2(int32_t y, int32_t limr, const uint16_t *ex) {
    const int32_t z = y < limr ? (int32_t)ex[y] : y;
    return y < limr && z >= (y | 15) + 1 ? z : y;
}

// the advance of a rare form at stream position p (h: its 16 bytes): the full parse; kTOver when the
// stream goes to the exact decoder
EZ_HD int32_t tk_rare_adv(V16 h, int32_t p, int32_t nb, int32_t lim32, int64_t limit) {
    K2Tok t;
    return k2_scan(h, p, nb, lim32, limit, t) == kParseHandOver ? kTOver : t.adv;
}

// One step of the walk at window offset e, whose stored exit is x = ex[e]; sl: the segment of the
// step before (-1 at first).  A segment's first chain position is recorded as its entry; a rare form
// (x == e) takes rare(e), tk_rare_adv of the staged bytes, and its exit is stored back into ex for
// the marking (clamped: ex holds 16 bits); wr: this lane stores (one lane of the wave).  A form to
// hand over (kTOver) leaves e past any stream: the walk ends and tk_walk_code returns its code
template <class Rare>
EZ_HD void tk_walk_step(int32_t &e, int32_t &sl, int32_t x, uint16_t *ex, uint16_t *ent, bool wr, Rare rare) {
    const int32_t sg = e >> 4;
    if (sg != sl) {
        if (wr) ent[sg] = (uint16_t)e;
        sl = sg;
    }
    if (x == e) {
        x = e + rare(e);
        if (wr) ex[e] = (uint16_t)(x < 0xffff ? x : 0xffff);
    }
    e = x;
}
// after the walk, which left the window at offset e: the last token runs past the input, or a form to hand over
EZ_HD int tk_walk_code(int32_t base, int32_t e, int32_t nb) { return base + e > nb ? kTokPast : 0; }

// a segment's entry as the marking's first position: none = the segment's end (nothing to mark)
EZ_HD int32_t tk_entry_or(int32_t entry, int32_t se) { return entry != kTNoEntry ? entry : se; }

// One marking step in the segment at s0: q is a token start; on by its advance (a rare form's from
// the exit the walk resolved)
EZ_HD void tk_mark_step(int32_t &q, uint32_t &m16, int32_t s0, const uint8_t *adv, const uint16_t *ex) {
    m16 |= 1u << (q - s0);
    int32_t a = (int32_t)adv[q];
    if (a == 0) a = (int32_t)ex[q] - q;
    q += a;
}

// The segments the walk stepped over: a marked segment's exit q (had: the segment had an entry) is the
// entry of the segment it lands in when that one has none yet (the chain's exits lie in distinct segments)
EZ_HD void tk_fill_entry(bool had, int32_t q, int32_t limr, uint16_t *ent) {
    if (had && q < limr && ent[q >> 4] == kTNoEntry) ent[q >> 4] = (uint16_t)q;
}

// ---------------------------------------------------------------- the round stage

EZ_HD int tk_args_code(int64_t in_total, int64_t nb, int64_t cap) {
    return in_total < 16 || nb >= (1ll << 30) || cap >= (1ll << 30) || cap < 16 ? kTokArgs : 0;
}

// The common forms branch-free (fast_tok) into tk; true: another form (padding, metas, long tags and
// offsets) or a length over the limit, which take the full parse (k2_scan)
EZ_HD bool tk_parse_fast(V16 h, int32_t lim32, K2Tok &tk) {
    tk.j = 1;
    tk.marg = 0;
    int32_t fadv;
    const int32_t ft = fast_tok(h.lo, tk.L, fadv, tk.D, tk.cp);
    tk.D = tk.cp ? tk.D : 0;
    return ft < 0 || tk.L > lim32;
}

// a Break meta's first two bytes (0x80, MetaBreak | MetaLen0)
EZ_HD bool tk_is_break(V16 h) { return ((uint32_t)h.lo & 0xffffu) == (0x80u | ((kMetaBreak | kMetaLen0) << 8)); }

// MetaReset (rsts: the round's lanes that parsed one, not 0; toks: those with a token): only before
// any output, once, and before the round's tokens
EZ_HD int tk_reset_code(int32_t pos, uint64_t rsts, uint64_t toks) {
    const int f = (int)__builtin_ctzll(rsts);
    return pos != 0 || __builtin_popcountll(rsts) > 1 || (toks & ((1ull << f) - 1)) ? kTokReset : 0;
}
EZ_HD int tk_window_code(int32_t bsl, uint64_t toks) { return bsl < 0 && toks ? kTokNoWindow : 0; }

// the round is cut before this lane: a token moved alone, or the running output incl past the budget
EZ_HD bool tk_cut(bool has, bool tok, int32_t L, int32_t incl, int32_t budget) { return has && ((tok && L > kTBig) || incl > budget); }
// tokens of the round: up to the first cut lane, of the left tokens of the list (0: lane 0's token alone)
EZ_HD int32_t tk_round_len(uint64_t cut, int32_t left) { return cut ? (int32_t)__builtin_ctzll(cut) : (left < kWave ? left : kWave); }

EZ_HD bool tk_no_room(int32_t pos, int32_t n, int32_t cap) { return (uint32_t)pos + (uint32_t)n > (uint32_t)cap; }
EZ_HD bool tk_past_window(bool cp, uint32_t D, int32_t bsl) { return cp && bsl < 30 && D > (1u << bsl); }
EZ_HD int tk_alone_code(int32_t pos, int32_t L, int32_t cap, bool cp, uint32_t D, int32_t bsl) {
    if (tk_no_room(pos, L, cap)) return kTokAlone | kTokRoomFlag;
    return tk_past_window(cp, D, bsl) ? kTokAlone : 0;
}
EZ_HD int tk_room_code(int32_t pos, int32_t total, int32_t cap) { return tk_no_room(pos, total, cap) ? kTokRoom | kTokRoomFlag : 0; }
EZ_HD int tk_far_code(uint64_t far) { return far ? kTokFar : 0; }  // far: the round's lanes with tk_past_window

// a literal moved alone is left to kd_copy (nd: the stream's deferred literals so far)
EZ_HD bool tk_defers(bool cp, int32_t L, int nd, bool have_list) { return !cp && L >= kDeferMin && nd < kDefSlots && have_list; }
// the alone path's pass width: a copy's reads stay below the bytes its pass writes
EZ_HD int32_t tk_alone_width(bool cp, int32_t D) {
    return !cp || D == 0 ? 16 * kWave : ((D & ~15) < 16 * kWave ? (D & ~15) : 16 * kWave);
}
// bytes a run of period per (1..15) advances per 16-byte pattern store
EZ_HD int32_t run_step_of(int32_t per) { return per * (16 / per); }

// a copy's source must be final up to need (exclusive) before it runs: its first min(D, L) bytes
// (the rest it reads from itself); a zero region needs nothing
EZ_HD int32_t tk_need(int32_t D, int32_t cs, int32_t L) { return D == 0 ? -0x7fffffff : cs + (D < L ? D : L); }
// final at the round's start: a zero region, a source before the round
EZ_HD bool tk_free0(bool cpy, int32_t D, int32_t need, int32_t pos) { return cpy && (D == 0 || need <= pos); }
// sources from here on are in the ring during the round
EZ_HD int32_t tk_ringlo(int32_t pos, int32_t total, int32_t R) { return pos + total - R + 16; }

// The redirect search.  Only in rounds with >= kTSearchMin copies reading the round's own output:
// there the searches pay (C4s: 26 -> 22 batches per round, K2 101 -> 94 ms); on C2's logs (10 such
// copies per round on average, 4.1 -> 3.0 batches) they cost more than the batches they save
// (4.44 -> 4.55 ms), and 2 % of its rounds reach 16.  kTSearchSteps: two steps resolve 72 % of what
// any number would on C2's logs (a simulation of the rounds; each step a 4-way search, three
// dependent LDS round trips)
constexpr int kTSearchMin = 16, kTSearchSteps = 2;
// what the search reads of the token holding a position: its output end, and -1 literal, D > 0 a
// copy, 0 neither (in: a token of the round)
EZ_HD int32_t tk_tend(bool in, int32_t dst, int32_t L) { return in ? dst + L : 0; }
EZ_HD int32_t tk_tinf(bool in, bool cp, int32_t D) { return !in ? 0 : (!cp ? -1 : D); }
// a copy that may read another copy's source instead: not overlapping itself, 16-byte reads
EZ_HD bool tk_redir(int32_t D, int32_t L) { return D >= 16 && D >= L; }
// The token holding position y: the last lane whose output starts at or before it (dst does not
// decrease over the lanes; a lane with no output shares its dst with the next one).  One of three
// 4-way steps (st = 16, 4, 1) from t = 0: d1, d2, d3 = dst of lanes t + st, t + 2 st, t + 3 st
EZ_HD int tk_owner_step(int t, int st, int32_t d1, int32_t d2, int32_t d3, int32_t y) {
    return t + (d1 <= y ? st : 0) + (d2 <= y ? st : 0) + (d3 <= y ? st : 0);
}
// One step of the search for an open copy with source [ys, ye), t the lane holding ys, te and ti
// that token's tk_tend and tk_tinf: a source that straddles tokens or the round's start is left to
// the batches; inside a literal of the round it is final (fre); inside an earlier copy it becomes
// that copy's source (the same bytes), final when that lies before the round, else open for another step
EZ_HD void tk_redirect(int32_t &ys, int32_t &ye, bool &fre, bool &open, int32_t pos, int32_t te, int32_t ti, int t, int lane, bool redir) {
    if (ys < pos || ye > te || t >= lane) {
        open = false;
    } else if (ti < 0) {
        fre = true;
        open = false;
    } else if (ti > 0 && redir) {
        ys -= ti;
        ye -= ti;
        if (ye <= pos) {
            fre = true;
            open = false;
        }
    } else {
        open = false;
    }
}

// The batch led by lane a (the first pending copy, output at oa) ends before the first pending copy
// after it whose source is not final and reaches past oa
EZ_HD bool tk_breaks(bool pend, bool fre, int lane, int a, int32_t need, int32_t oa) { return pend && !fre && lane > a && need > oa; }
// the copy runs in the batch that ends before lane bnd
EZ_HD bool tk_runs(bool pend, bool fre, int lane, int bnd) { return pend && (fre || lane < bnd); }
// not the common copy (D >= 16, source in the ring, after the stream start): runs and zero regions,
// sources before the start or past the ring
EZ_HD bool tk_slow(bool ex, int32_t D, int32_t ys, int32_t ringlo) { return ex && (D < 16 || ys < 0 || ys < ringlo); }

}  // namespace ez
