// ez_decompress_tok.hip — K2t: token-parallel batch decompression, one wave per
// stream, every lane busy on the stream's tokens.
//
// Restates Reader.Read to EOF for NewReaderBytes (reader.go:116-216 read,
// readTag :218-270, continueMetaTag :272-325, Decoder :346-514) for the common
// case through k2_scan (ez_k2_parse.h); anything else hands the stream to the
// exact decoder (ez_decompress.hip), as K2r and K2w do.
//
// Why.  Reader.read walks its tokens one after another; a lane per stream (K2r)
// keeps that chain on one lane and leaves the chip one wave per SIMD at C1, and a
// wave per stream that walks the tokens on the scalar unit and moves each one
// with the whole wave (K2w) pays a scalar parse and a wave-wide step per token.
// Here the walk is split into what is parallel and what is not:
//
//  1. scan: the stream's compressed input is staged 1 KiB at a time (a window)
//     and every lane computes, for each of its 16 input positions, how many input
//     bytes a token starting there would take (SWAR over 4 positions a word; the
//     common forms only, 0 for the others);
//  2. walk: each lane follows the chain through its own 16 positions from every
//     entry offset (backwards, so each position's exit from the lane's segment
//     is one lookup: ex[p]); the scalar unit then crosses the window segment to
//     segment through those exits (64 steps per window, the rare forms parsed in
//     full when the walk reaches them), and every lane marks the real token starts
//     of its segment from the entry the walk gave it;
//  3. tokens: the starts are compacted into a list; each round gives 64 tokens
//     one lane each: the full parse (k2_scan), a wave prefix sum of the output
//     lengths (every token's output position at once), every literal written at
//     once, and the copies in batches: a batch runs every copy up to the first one
//     whose source reaches past the batch's first output byte (copies of log lines
//     mostly read output decoded a few hundred bytes earlier: ~26 batches for the
//     ~210 copies of a C1 stream).
//
// Output goes through an LDS ring of R bytes (R = 4 KiB or 8 KiB) and leaves it
// 1 KiB at a time; copies reaching past the ring read the output already in HBM.
// A token longer than kTBig bytes is moved alone by the whole wave, HBM to HBM.
#include "ez_format.h"
#include "ez_internal.h"
#include "ez_wave.h"
#include "ez_bytes.h"
#include "ez_k2_parse.h"
#include "ez_k2_ring.h"
#include "ez_k2_tok.h"

namespace ez {
namespace {

// timing builds only (wrong bytes; each bit skips a step at its call in tok_one): 256 no copy
// batches, 512 no literal pass, 1024 no rounds, 2048 no walk; 4096: a debug build, see HANDOVER
#ifndef EZ_EXP
#define EZ_EXP 0
#endif

__device__ __forceinline__ V16 lds16(const uint8_t *p) { return V16{*(const u64_ua *)p, *(const u64_ua *)(p + 8)}; }

// the bytes of v before position x + k (k < 16) that lie before the stream start read 0
__device__ __forceinline__ V16 zero_before_start(V16 v, int32_t x) {
    if (x >= 0) return v;
    const uint32_t nz = (uint32_t)(-x);
    return shl16(shr16(v, nz), nz);
}

typedef uint32_t __attribute__((aligned(1))) u32_ua;
typedef uint16_t __attribute__((aligned(1))) u16_ua;

// the first n bytes (1..16) of v at d, without branches: five stores, the absent ones to trash
__device__ __forceinline__ void put_exact(uint8_t *d, V16 v, uint32_t n, uint8_t *trash) {
    const bool b8 = n >= 8;
    *(u64_ua *)(b8 ? d : trash) = v.lo;
    *(u64_ua *)(n == 16 ? d + 8 : trash) = v.hi;
    uint64_t x = b8 ? v.hi : v.lo;
    uint8_t *t = d + (n & 8);
    *(u32_ua *)((n & 4) ? t : trash) = (uint32_t)x;
    x = (n & 4) ? x >> 32 : x;
    t += n & 4;
    *(u16_ua *)((n & 2) ? t : trash) = (uint16_t)x;
    x = (n & 2) ? x >> 16 : x;
    t += n & 2;
    *(uint8_t *)((n & 1) ? t : trash) = (uint8_t)x;
}
// n bytes (1..16) of position p into the ring, exact; the mirror / wrapped copy only when needed
template <int32_t R>
__device__ __forceinline__ void rput_fast(uint8_t *ring, int32_t p, V16 v, uint32_t n, uint8_t *trash) {
    const int32_t r = p & (R - 1);
    put_exact(ring + r, v, n, trash);
    const bool mir = r < 16 || r + (int32_t)n > R;
    if (__ballot(mir)) {
        if (mir) put_n(ring + (r < 16 ? r + R : r - R), v, n);
    }
}

// tk_rare_adv of the staged bytes h (the same on every lane), out of line: the full parse stays out
// of the walk's loop
__device__ __attribute__((noinline)) int32_t rare_adv(const uint8_t *h, int32_t p, int32_t nb, int32_t lim32, int64_t limit) {
    return __builtin_amdgcn_readfirstlane(tk_rare_adv(lds16(h), p, nb, lim32, limit));
}

// what the steps share of a stream: the wave's LDS arrays, the stream's input and its slot
struct TokCtx {
    const DecompressArgs &A;
    uint64_t s;
    int lane;
    uint8_t *ring, *inb, *tab;
    uint8_t *trash;   // the lane's 16 bytes of tab (the advances are dead during the rounds)
    int32_t *defs;    // the stream's deferred literals
    const uint8_t *b, *in_end;
    uint8_t *out;
    int32_t nb, cap, lim32;
    int64_t limit;
    // of the window: the segment exits, then the token list (tp) in their place; the segment entries
    __device__ __forceinline__ uint16_t *ex() const { return (uint16_t *)(tab + kTWin); }
    __device__ __forceinline__ uint16_t *ent() const { return (uint16_t *)(tab + 3 * kTWin); }
};
// the decoder's state: the output position, the position below which the output is in HBM, log2 of
// the window (-1: no MetaReset yet), the stream's deferred literals (kd_copy moves them after the decoders)
struct TokState {
    int32_t pos, fl, bsl;
    int nd;
};

// ---- scan: stage the window [base, base + kTStage) (bytes past the batch read 0); the advance of
// every position of the lane's segment; the segment exits, then in place the exits two steps on
__device__ __forceinline__ void win_scan(const TokCtx &C, int32_t base, int32_t limr) {
    const int lane = C.lane;
    for (int32_t k = 16 * lane; k < kTStage; k += 16 * kWave) {
        const V16 v = ld_in(C.b + base + k, C.A.in, C.in_end);
        *(u64_ua *)(C.inb + k) = v.lo;
        *(u64_ua *)(C.inb + k + 8) = v.hi;
    }
    __syncthreads();
    uint32_t ad[4];
    tk_advances(*(const uint4 *)(C.inb + 16 * lane), *(const uint32_t *)(C.inb + 16 * lane + 16), ad);
    *(uint4 *)(C.tab + 16 * lane) = make_uint4(ad[0], ad[1], ad[2], ad[3]);
    uint16_t *ex = C.ex();
    const int32_t s0 = 16 * lane;
    C.ent()[lane] = kTNoEntry;
    tk_exits(ad, s0, tk_stop(s0 + 16, limr), ex);
    __syncthreads();
    // exits two steps on: the walk then crosses two segments per LDS round trip; the entries of the
    // segments it steps over are filled in by the marking (each is the exit of the segment before it)
    uint32_t e2[8];
    const uint4 r0 = *(const uint4 *)(ex + s0), r1 = *(const uint4 *)(ex + s0 + 8);
    const uint32_t e1[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
#pragma unroll
    for (int t = 0; t < 8; t++)
        e2[t] = (uint32_t)tk_exit2((int32_t)(e1[t] & 0xffffu), limr, ex) | ((uint32_t)tk_exit2((int32_t)(e1[t] >> 16), limr, ex) << 16);
    __syncthreads();  // (every lane has read the exits it needs)
    *(uint4 *)(ex + s0) = make_uint4(e2[0], e2[1], e2[2], e2[3]);
    *(uint4 *)(ex + s0 + 8) = make_uint4(e2[4], e2[5], e2[6], e2[7]);
    __syncthreads();
}

// ---- walk (uniform) from the entry e segment to segment through the exits, resolving the rare forms
// on the way; each segment's first chain position is its entry.  e: where the chain leaves the window
__device__ __forceinline__ int win_walk(const TokCtx &C, int32_t base, int32_t limr, int32_t &e) {
    uint16_t *ex = C.ex();
    int32_t sl = -1;
    while (e < limr) {  // (e, x, sl uniform)
        const int32_t x = __builtin_amdgcn_readfirstlane((int32_t)ex[e]);
        tk_walk_step(e, sl, x, ex, C.ent(), C.lane == 0, [&](int32_t at) {
            return __builtin_amdgcn_readfirstlane(rare_adv(C.inb + at, base + at, C.nb, C.lim32, C.limit));
        });
    }
    return tk_walk_code(base, e, C.nb);
}

// the marking of the lane's segment from q on, for the lanes that are on
__device__ __forceinline__ void mark_segment(bool on, int32_t &q, uint32_t &m16, int32_t s0, int32_t sm, const uint8_t *adv, const uint16_t *ex) {
    while (__ballot(on && q < sm)) {
        if (on && q < sm) tk_mark_step(q, m16, s0, adv, ex);
    }
}

// ---- every lane marks the chain's token starts in its segment, from the entry the walk gave it (then
// the segments the walk stepped over, from the entries the first pass gives them); the starts become
// the token list in input order, in the exits' place.  Returns the tokens of the window
__device__ __forceinline__ int32_t win_list(const TokCtx &C, int32_t limr) {
    const int lane = C.lane;
    uint16_t *ex = C.ex(), *ent = C.ent(), *tp = ex;
    const int32_t s0 = 16 * lane, se = s0 + 16, sm = tk_stop(se, limr);
    __syncthreads();
    int32_t q2 = (int32_t)ent[lane];
    const bool had = q2 != kTNoEntry;
    q2 = tk_entry_or(q2, se);
    uint32_t m16 = 0;
    mark_segment(true, q2, m16, s0, sm, C.tab, ex);
    __syncthreads();
    tk_fill_entry(had, q2, limr, ent);
    __syncthreads();
    if (!had) q2 = tk_entry_or((int32_t)ent[lane], se);
    mark_segment(!had, q2, m16, s0, sm, C.tab, ex);
    // a wave prefix sum of the counts, then each lane's starts
    const int32_t mc = __builtin_popcount(m16);
    int32_t ic = mc;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const int32_t v = __shfl_up(ic, d, kWave);
        if (lane >= d) ic += v;
    }
    const int32_t cnt = __builtin_amdgcn_readlane(ic, kWave - 1);
    __syncthreads();  // (the exits are read; the list overwrites them)
    int32_t at = ic - mc;
    while (__ballot(m16 != 0)) {
        if (m16 != 0) {
            tp[at++] = (uint16_t)(s0 + (int32_t)__builtin_ctz(m16));
            m16 &= m16 - 1;
        }
    }
    __syncthreads();
    return cnt;
}

// a round: up to 64 tokens of the list, one per lane
struct TokRound {
    V16 h;          // the token's 16 header bytes
    K2Tok tk;
    int32_t q;      // its input position
    int rr;         // its parse (kParseSkip on a lane without one)
    bool has, tok;  // a list entry; a token (not padding or a meta)
    int32_t L, incl;  // its output bytes; the running sum over the lanes
    int32_t nr;     // tokens of the round: up to the first one moved alone, within the output budget (0: lane 0's alone)
};

// ---- the round's parse (the full parse where fast_tok does not know the form), the MetaReset, the
// prefix sum of the output lengths and the cut
template <int32_t R>
__device__ __forceinline__ int round_parse(const TokCtx &C, TokState &S, int32_t base, int32_t t0, int32_t cnt, TokRound &r) {
    const int lane = C.lane;
    r.has = t0 + lane < cnt;
    r.q = base + (r.has ? (int32_t)C.ex()[t0 + lane] : 0);
    r.h = lds16(C.inb + (r.q - base));
    const bool other = tk_parse_fast(r.h, C.lim32, r.tk);
    const bool full = r.has && other;
    int rr = kParseToken;
    if (__ballot(full)) {
        if (full) rr = k2_scan(r.h, r.q, C.nb, C.lim32, C.limit, r.tk);
    }
    rr = r.has ? rr : kParseSkip;
    r.rr = rr;
    if (__ballot(rr == kParseHandOver)) return kTokForm;
    r.tok = rr == kParseToken;
    const uint64_t rsts = __ballot(rr == kScanReset), toks = __ballot(r.tok);
    if (rsts) {
        if (const int code = tk_reset_code(S.pos, rsts, toks)) return code;
        S.bsl = __builtin_amdgcn_readlane((int)r.tk.marg, (int)__builtin_ctzll(rsts));
    }
    if (const int code = tk_window_code(S.bsl, toks)) return code;
    r.L = r.tok ? r.tk.L : 0;
    int32_t incl = r.L;
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const int32_t v = __shfl_up(incl, d, kWave);
        if (lane >= d) incl += v;
    }
    r.incl = incl;
    r.nr = tk_round_len(__ballot(tk_cut(r.has, r.tok, r.L, incl, TLayout<R>::budget)), cnt - t0);
    return 0;
}

// ---- lane 0's token alone (longer than kTBig): HBM to HBM by the whole wave
template <int32_t R>
__device__ __forceinline__ int alone_token(const TokCtx &C, TokState &S, const TokRound &r) {
    const int lane = C.lane;
    uint8_t *ring = C.ring, *out = C.out;
    const int32_t pos = S.pos;
    const int32_t L0 = __builtin_amdgcn_readlane(r.L, 0), D0 = __builtin_amdgcn_readlane((int)r.tk.D, 0);
    const bool cp0 = __builtin_amdgcn_readlane((int)r.tk.cp, 0) != 0;
    const int32_t src0 = __builtin_amdgcn_readlane(r.q + r.tk.j, 0);
    if (const int code = tk_alone_code(pos, L0, C.cap, cp0, (uint32_t)D0, S.bsl)) return code;
    flush_exact<R>(ring, out, S.fl, pos, lane);  // everything before it to HBM
    __builtin_amdgcn_s_waitcnt(0);               // (stores done before the copy reads them back)
    if (tk_defers(cp0, L0, S.nd, C.A.defer != nullptr)) {
        // a long literal: recorded for kd_copy (the chip moves it after the decoders); the ring gets
        // its last bytes from the input
        defer_record(C.A, C.s, C.defs, S.nd, pos, src0, L0, lane);
        S.nd++;
        for (int32_t x = L0 - R + 16 * lane; x < L0; x += 16 * kWave)  // (L0 > R)
            rput<R>(ring, pos + x, ld_in(C.b + src0 + x, C.A.in, C.in_end), (uint32_t)(L0 - x < 16 ? L0 - x : 16));
        S.pos = S.fl = pos + L0;
        __syncthreads();
        return 0;
    }
    if (!cp0 || D0 == 0 || D0 >= 16) {
        const int32_t W = tk_alone_width(cp0, D0);
        for (int32_t done = 0; done < L0; done += W) {
            const int32_t k = done + 16 * lane;
            if (16 * lane < W && k < L0) {
                V16 v{0, 0};
                if (!cp0) v = ld_in(C.b + src0 + k, C.A.in, C.in_end);
                else if (D0 != 0) v = far16(out, C.cap, C.b, pos - D0 + k, S.nd, C.defs);  // before the stream: 0
                if (k + 16 <= L0) st16v(out + pos + k, v);
                else put_small(out + pos + k, v, (uint32_t)(L0 - k));
            }
            __builtin_amdgcn_s_waitcnt(0);
        }
    } else {  // a short-period run: its 16-byte pattern every step bytes
        const V16 v = zero_before_start(rld<R>(ring, pos - 16), pos - 16);
        const V16 pv = run_pattern(shr16(v, (uint32_t)(16 - D0)), (uint32_t)D0);
        const int32_t stp = run_step_of(D0);
        for (int32_t k = stp * lane; k < L0; k += stp * kWave) {
            if (k + 16 <= L0) st16v(out + pos + k, pv);
            else put_small(out + pos + k, pv, (uint32_t)(L0 - k));
        }
        __builtin_amdgcn_s_waitcnt(0);
    }
    // the ring gets the token's last bytes back (what later copies may read from it)
    const int32_t np = pos + L0;
    const int32_t lo = np - R > pos ? np - R : pos;
    for (int32_t x = lo + 16 * lane; x < np; x += 16 * kWave)
        rput<R>(ring, x, ld_clamped16(out + x, out, out + C.cap), (uint32_t)(np - x < 16 ? np - x : 16));
    S.pos = S.fl = np;
    __syncthreads();
    return 0;
}

// ---- the round's place in the output: the slot's room, every distance within the window, and the
// output positions of its Break metas (0x80, MetaBreak | MetaLen0) for a Reader handle's Reads (which
// stop there with ErrBreak, reader.go:312-313).  dst: the lane's output position; total: the round's bytes
__device__ __forceinline__ int round_place(const TokCtx &C, const TokState &S, const TokRound &r, int32_t dst, int32_t total) {
    const bool brk = r.has && C.lane < r.nr && r.rr == kParseSkip && tk_is_break(r.h);
    if (C.A.breaks && __ballot(brk)) {
        if (brk) {
            const uint64_t at = atomicAdd((unsigned long long *)C.A.breaks, 1ull);
            if (at < C.A.breaks_cap) C.A.breaks[1 + at] = (uint64_t)dst;
        }
    }
    if (const int code = tk_room_code(S.pos, total, C.cap)) return code;
    return tk_far_code(__ballot(C.lane < r.nr && r.tok && tk_past_window(r.tk.cp, r.tk.D, S.bsl)));
}

// ---- literals: all at once (their bytes from the staged window, or HBM past it)
template <int32_t R>
__device__ __forceinline__ void round_literals(const TokCtx &C, const TokRound &r, int32_t base, int32_t dst) {
    const bool lit = C.lane < r.nr && r.tok && !r.tk.cp;
    const int32_t src = r.q + r.tk.j, L = r.L;
    for (int32_t k = 0; __ballot(lit && 16 * k < L); k++) {
        if (lit && 16 * k < L) {
            const int32_t x = src + 16 * k;
            const bool staged = x + 16 <= base + kTStage;
            V16 v = lds16(C.inb + (staged ? x - base : 0));
            if (__ballot(!staged)) {
                if (!staged) v = ld_in(C.b + x, C.A.in, C.in_end);
            }
            rput_fast<R>(C.ring, dst + 16 * k, v, (uint32_t)(L - 16 * k < 16 ? L - 16 * k : 16), C.trash);
        }
    }
}

// ---- copies, in batches: every copy up to the first one whose source reaches past the batch's
// first output byte (its sources are final; the writes never overlap)
template <int32_t R>
__device__ __forceinline__ void round_copies(const TokCtx &C, const TokState &S, const TokRound &r, int32_t dst, int32_t total) {
    const int lane = C.lane;
    uint8_t *ring = C.ring;
    const int32_t pos = S.pos, L = r.L;
    const bool in = lane < r.nr && r.tok;
    const bool cpy = in && r.tk.cp;
    const int32_t D = (int32_t)r.tk.D;
    const int32_t cs = dst - D;
    const int32_t need = tk_need(D, cs, L);
    const int32_t ringlo = tk_ringlo(pos, total, R);
    uint64_t cm = __ballot(cpy);
    // ---- sources final at the round's start (every copy marked fre may run in any batch): zero
    // regions, sources before the round; with the search (ez_k2_tok.h: tk_redirect) also sources
    // inside one literal of the round (all written before), and a copy (tk_redir) whose source lies
    // inside an earlier copy of the round reads that copy's source instead, repeated while it lands
    // in a copy
    int32_t ys = cs;  // the copy's (redirected) source
    bool fre = tk_free0(cpy, D, need, pos);
    if (__builtin_popcountll(__ballot(cpy && !fre)) >= kTSearchMin) {
        const int32_t tend = tk_tend(in, dst, L), tinf = tk_tinf(in, r.tk.cp, D);
        int32_t ye = need;
        bool open = cpy && !fre;
        const bool redir = tk_redir(D, L);
        for (int it = 0; it < kTSearchSteps && __ballot(open); it++) {
            const int32_t y = open ? ys : pos;
            int t = 0;
#pragma unroll
            for (int st = 16; st > 0; st >>= 2) {
                const int32_t d1 = __builtin_amdgcn_ds_bpermute(4 * (t + st), dst);
                const int32_t d2 = __builtin_amdgcn_ds_bpermute(4 * (t + 2 * st), dst);
                const int32_t d3 = __builtin_amdgcn_ds_bpermute(4 * (t + 3 * st), dst);
                t = tk_owner_step(t, st, d1, d2, d3, y);
            }
            const int32_t te = __builtin_amdgcn_ds_bpermute(4 * t, tend);
            const int32_t ti = __builtin_amdgcn_ds_bpermute(4 * t, tinf);
            if (open) tk_redirect(ys, ye, fre, open, pos, te, ti, t, lane, redir);
        }
        if (open) ys = cs;  // unresolved: the batches' rule, on the copy's own source
    }
    // a copy reading output flushed to HBM: the flush stores complete first (same CU: its
    // L1 then serves the bytes stored)
    if (__ballot(cpy && D >= 16 && ys < ringlo)) __builtin_amdgcn_s_waitcnt(0);
    while (cm) {
        const int a = (int)__builtin_ctzll(cm);
        const int32_t oa = __builtin_amdgcn_readlane(dst, a);
        const bool pend = (cm >> lane) & 1;
        const uint64_t brk = __ballot(tk_breaks(pend, fre, lane, a, need, oa));
        const int bnd = brk ? (int)__builtin_ctzll(brk) : kWave;
        const bool ex = tk_runs(pend, fre, lane, bnd);
        // the common copy: 16-byte ring reads and exact writes; the others (tk_slow) below
        const bool slow = tk_slow(ex, D, ys, ringlo);
        if (__ballot(slow)) {
            V16 pv{0, 0};
            int32_t stp = 16;
            if (slow && D > 0 && D < 16) {
                const V16 v = zero_before_start(rld<R>(ring, dst - 16), dst - 16);
                pv = run_pattern(shr16(v, (uint32_t)(16 - D)), (uint32_t)D);
                stp = run_step_of(D);
            }
            for (int32_t k = 0; __ballot(slow && stp * k < L); k++) {
                const int32_t o = stp * k;
                if (slow && o < L) {
                    V16 v = pv;  // a run's pattern; a zero region's zeros
                    if (D >= 16) {
                        const int32_t x = ys + o;
                        if (x >= ringlo) v = zero_before_start(rld<R>(ring, x), x);
                        else v = far16(C.out, C.cap, C.b, x, S.nd, C.defs);  // flushed already (or deferred)
                    }
                    rput<R>(ring, dst + o, v, (uint32_t)(L - o < 16 ? L - o : 16));
                }
            }
        }
        const bool fast = ex && !slow;
        for (int32_t k = 0; __ballot(fast && 16 * k < L); k++) {
            if (fast && 16 * k < L)
                rput_fast<R>(ring, dst + 16 * k, rld<R>(ring, ys + 16 * k), (uint32_t)(L - 16 * k < 16 ? L - 16 * k : 16), C.trash);
        }
        cm &= ~__ballot(ex);
    }
}

// ---- the round's output is final: whole 1 KiB chunks leave the ring
template <int32_t R>
__device__ __forceinline__ void round_done(const TokCtx &C, TokState &S, int32_t total) {
    S.pos += total;
    while (S.pos >= S.fl + 16 * kWave) {
        st16v(C.out + S.fl + 16 * C.lane, rld<R>(C.ring, S.fl + 16 * C.lane));
        S.fl += 16 * kWave;
    }
}

// hand the stream over; debug builds (EZ_EXP & 4096) record where (status 100 + code, out_size = pos).
// A hand-over because the output needs more than the slot (kTokRoomFlag) is marked for a caller that
// sizes the slot itself (a Reader handle's whole-stream decode retries with a larger one, and the exact
// decoder does not re-decode the stream just to find the slot too small)
#if (EZ_EXP & 4096)
#define HANDOVER_DEBUG(code)                                         \
    if (lane == 0) {                                                 \
        A.out_size[s] = (uint64_t)S.pos | ((uint64_t)w << 32);       \
        if (A.status) A.status[s] = 100 + ((code) & 0xff);           \
    }
#else
#define HANDOVER_DEBUG(code)
#endif
#define HANDOVER(code)                                                                        \
    do {                                                                                      \
        const int code_ = (code);                                                             \
        if (code_) {                                                                          \
            if ((code_ & kTokRoomFlag) && A.end_state && lane == 0) A.end_state[0] = -2;      \
            HANDOVER_DEBUG(code_)                                                             \
            return false;                                                                     \
        }                                                                                     \
    } while (0)

// stream s by the whole wave; false = hand it over to the exact decoder
template <int32_t R>
__device__ bool tok_one(const DecompressArgs &A, const uint64_t s, uint8_t *smem, const int lane) {
    using Lay = TLayout<R>;
    const uint8_t *in_end = A.in + A.in_off[A.count];
    const int64_t nb64 = (int64_t)(A.in_off[s + 1] - A.in_off[s]), cap64 = (int64_t)(A.out_off[s + 1] - A.out_off[s]);
    TokState S{0, 0, -1, 0};
    int32_t w = 0;  // the chain's entry into the next window
    HANDOVER(tk_args_code(in_end - A.in, nb64, cap64));
    const TokCtx C{A, s, lane, smem + Lay::ring, smem + Lay::inb, smem + Lay::tab, smem + Lay::tab + 16 * lane, (int32_t *)(smem + Lay::defs),
                   A.in + A.in_off[s], in_end, A.out + A.out_off[s], (int32_t)nb64, (int32_t)cap64, k2_lim32(A.block_size_limit), A.block_size_limit};
    while (w < C.nb) {
        const int32_t base = w & ~15, limr = tk_limr(C.nb, base);
        // 1. scan
        win_scan(C, base, limr);
        // 2. walk, and the token starts it gives
        int32_t e = limr;
        if (!(EZ_EXP & 2048)) {
            e = w - base;
            HANDOVER(win_walk(C, base, limr, e));
        }
        const int32_t cnt = win_list(C, limr);
        // 3. tokens: rounds of up to 64, one per lane
        for (int32_t t0 = 0; !(EZ_EXP & 1024) && t0 < cnt;) {
            TokRound r;
            HANDOVER(round_parse<R>(C, S, base, t0, cnt, r));
            if (r.nr == 0) {
                HANDOVER(alone_token<R>(C, S, r));
                t0 += 1;
                continue;
            }
            const int32_t total = __builtin_amdgcn_readlane(r.incl, r.nr - 1), dst = S.pos + r.incl - r.L;
            HANDOVER(round_place(C, S, r, dst, total));
            if (!(EZ_EXP & 512)) round_literals<R>(C, r, base, dst);
            if (!(EZ_EXP & 256)) round_copies<R>(C, S, r, dst, total);
            round_done<R>(C, S, total);
            t0 += r.nr;
        }
        w = base + e;
        __syncthreads();
    }
    flush_exact<R>(C.ring, C.out, S.fl, S.pos, lane);  // the last partial chunk
    if (lane == 0) {
        A.out_size[s] = (uint64_t)S.pos;
        if (A.status) A.status[s] = EZ_OK;
        if (A.end_state) {  // (one MetaReset, before any output: r.pos is the output since the start)
            A.end_state[0] = S.bsl < 0 ? 0 : (int64_t)1 << S.bsl;
            A.end_state[1] = S.pos;
        }
    }
    return true;
}

template <int32_t R>
__global__ __launch_bounds__(64) void k2_tok(DecompressArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int lane = (int)threadIdx.x;
    for (uint64_t s = blockIdx.x; s < A.count; s += gridDim.x)
        if (!tok_one<R>(A, s, smem, lane) && lane == 0) {
            slow_append(A, s);
        }
}

// every deferred literal's bytes (K2t's, and K2w's where that one is forced), 64 KiB pieces per block step
__global__ __launch_bounds__(256) void kd_copy(DecompressArgs A, uint64_t kp) {
    const uint64_t nl = A.defer[0] < A.defer_cap ? A.defer[0] : A.defer_cap;
    const DeferLit *rec = (const DeferLit *)(A.defer + 4);
    const uint8_t *lo = A.in, *hi = A.in + A.in_off[A.count];
    for (uint64_t q = blockIdx.x; q < nl * kp; q += gridDim.x) {
        const DeferLit L = rec[q / kp];
        // kp is a hint (the caller's largest slot): a longer literal's block takes every kp-th piece
        for (uint64_t b = (q % kp) * 65536; b < L.len; b += kp * 65536) {
            const uint64_t e = b + 65536 < L.len ? b + 65536 : L.len;
            for (uint64_t k = b + 16 * threadIdx.x; k < e; k += 16 * 256) {
                const V16 v = ld_in(A.in + L.src + k, lo, hi);
                if (k + 16 <= e) st16v(A.out + L.dst + k, v);
                else put_small(A.out + L.dst + k, v, (uint32_t)(e - k));
            }
        }
    }
}

}  // namespace

// R: an 8 KiB ring keeps more copies in LDS, a 4 KiB one fits more waves per CU (TLayout<4096>
// ~8.6 KiB, <8192> ~12.7 KiB of LDS).  A batch with more streams than the chip holds runs in
// rounds of resident waves, the last one partly empty, so R = 4096 is taken whenever it needs
// fewer such rounds (C2, 4,096 x 256 KiB: 3,072 resident waves at 8 KiB, all 4,096 at 4 KiB:
// K2 7.06 -> 4.93 ms), and always when the whole stream fits it.
static uint64_t resident_waves(const void *kernel, size_t lds) {
    int dev = 0, ncu = 0, per = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, kernel, 64, lds) != hipSuccess || per <= 0 || ncu <= 0)
        return 1;
    return (uint64_t)per * (uint64_t)ncu;
}
hipError_t launch_decompress_tok(const DecompressArgs &a, hipStream_t st) {
    const uint64_t grid = a.count < (1u << 30) ? a.count : (1u << 30);
    static const int force_r = knob("EZ_K2T_R", 0);  // A/B (experiment builds): 4096 / 8192
    static const uint64_t res4 = resident_waves((const void *)k2_tok<4096>, TLayout<4096>::bytes);
    static const uint64_t res8 = resident_waves((const void *)k2_tok<8192>, TLayout<8192>::bytes);
    const bool fits = a.max_out != 0 && a.max_out <= 4096;  // the whole stream fits the ring
    const bool fewer_rounds = (grid + res4 - 1) / res4 < (grid + res8 - 1) / res8;
    if (force_r == 4096 || (force_r == 0 && (fits || fewer_rounds))) {
        hipLaunchKernelGGL(k2_tok<4096>, dim3((unsigned)grid), dim3(64), TLayout<4096>::bytes, st, a);
    } else {
        hipLaunchKernelGGL(k2_tok<8192>, dim3((unsigned)grid), dim3(64), TLayout<8192>::bytes, st, a);
    }
    return hipGetLastError();
}

hipError_t launch_defer_copy(const DecompressArgs &a, hipStream_t st) {
    // pieces per record: the largest output slot bounds a literal (max_out 0: unknown, take 1 GiB)
    const uint64_t mo = a.max_out ? a.max_out : (1ull << 30);
    hipLaunchKernelGGL(kd_copy, dim3(2048), dim3(256), 0, st, a, (mo + 65535) / 65536);
    return hipGetLastError();
}

}  // namespace ez
