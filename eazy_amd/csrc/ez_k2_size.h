// ez_k2_size.h — the per-lane steps of K2z, the batch decoded-size query (ez_decompress_size.hip):
// a stream's output length from its token headers alone.
//
// A wave takes a stream in blocks of 64 chunks of C input bytes, a chunk per lane, staged so that
// every step reads the staged bytes only: a super-block, which starts at the true chain's position
// (K2z's wave route, K2g), or a part on a fixed grid (K2z's parts route, ez_k2_parts.h).  The token
// chain (every token starts where the previous one ends, readTag reader.go:218-270) is cut as K2j
// cuts it (ez_decompress_jump.hip); kz_walk (ez_k2_walk.h) drives the first four steps over the wave:
//   kz_spec    a lane parses speculatively from up to one chunk before its own and records the
//              positions it visits inside its chunk (a bitmap) and where it leaves it;
//   kz_entry   its assumed entry: the predecessor's speculative exit, or the true position;
//   kz_verify  from its entry it walks until it meets a recorded position (its exit is then the
//              speculative one) or leaves the chunk; an entry at or past the chunk's end (a token that
//              spans the chunk) passes through;
//   kz_fix     one round of the repair where a lane's assumed entry was not its predecessor's exit;
//   kz_sum     it walks its true chain once with the full k2_scan (ez_k2_parse.h) and sums the output
//              bytes, the longest distance and the flags the stream's checks need;
//   kz_end_ok  the checks at the stream's end (kj_scan's, without a slot).
// All of them are functions over a byte pointer, so the host checks run the same source over 64
// emulated lanes (tools/k2_check_common.h: emu_walk, the mirror of kz_walk).  Positions are stream
// offsets in uint32_t: a stream is shorter than 2^31 bytes (longer ones are handed over before any
// step) and a step takes less than 2^31, so no sum wraps.
#pragma once

#include "ez_k2_parse.h"

namespace ez {

constexpr int kZLanes = 64;                // chunks of a super-block, one per lane
constexpr int kZFixRounds = 64;            // re-walks of a super-block at most (a lane each: 63 suffice)
enum : uint32_t { kZBad = 1, kZReset = 2, kZResetLate = 4 };  // KzSum.fl; bits 8-15: the chunk's last MetaReset

// the staged bytes: p[0] is the stream's byte `base`; zeros past the stream's end
struct KzWin {
    const uint8_t *p;
    uint32_t base;
};
// staged bytes of a super-block of chunk size c: its chunks plus the 16 bytes a header at its end reads
constexpr uint32_t kz_stage_bytes(uint32_t c) { return kZLanes * c + 16; }

EZ_HD V16 kz_at(const KzWin &w, uint32_t y) {
    typedef uint64_t __attribute__((aligned(1))) u64u;
    const uint8_t *q = w.p + (y - w.base);
    return V16{*(const u64u *)q, *(const u64u *)(q + 8)};
}

// a padding run stops at the stream's end (readTag skips the zeros up to there, reader.go:221-224):
// the staged bytes past it are zeros too
EZ_HD uint32_t kz_clamp_pad(uint32_t t0, uint32_t q, uint32_t nb) { return t0 == 0 && q > nb ? nb : q; }

// the position after the token (padding run, meta) at p < nb, by jadv_fast: no checks
EZ_HD uint32_t kz_next(const KzWin &w, uint32_t p, uint32_t nb) {
    const V16 h = kz_at(w, p);
    return kz_clamp_pad((uint32_t)h.lo & 0xff, p + (uint32_t)jadv_fast(h), nb);
}

// lane's chunk of the super-block at sb: [c0, ce), empty for a chunk past the stream's end
template <int C>
EZ_HD void kz_chunk(uint32_t sb, int lane, uint32_t nb, uint32_t &c0, uint32_t &ce) {
    c0 = sb + (uint32_t)lane * C;
    ce = c0 + C < nb ? c0 + C : nb;
}

// The speculative walk of lane's chunk of the block at ps.  known: e is the true chain's position, at
// or past ps: the lane whose chunk holds e starts there (no warm-up: it is on the true chain), the
// lanes before it visit nothing.  A super-block starts at the true position: known, e = ps, and lane 0
// holds it.  Every other lane warms up over the chunk before its own (inside the staged bytes), so
// that its chain has usually met the true one by its chunk's start; lane 0 of a part over the staged
// chunk before the part (from 0 in the stream's first part, which is the true entry).  bm[0 .. C/32):
// the positions visited in the chunk; first: the first of them (the walk's exit if none); returns
// where the walk leaves the chunk.
template <int C>
EZ_HD uint32_t kz_spec(const KzWin &w, uint32_t ps, int lane, uint32_t nb, bool known, uint32_t e, uint32_t *bm, uint32_t &first) {
    uint32_t c0, ce;
    kz_chunk<C>(ps, lane, nb, c0, ce);
    for (int k = 0; k < C / 32; k++) bm[k] = 0;
    first = c0;
    if (c0 >= nb) return c0;
    if (known && e >= ce) {  // (the true chain enters after this chunk)
        first = e;
        return e;
    }
    uint32_t p = known && e >= c0 ? e : (c0 >= (uint32_t)C ? c0 - (uint32_t)C : 0u);
    while (p < c0) p = kz_next(w, p, nb);
    first = p;
    while (p < ce) {
        bm[(p - c0) >> 5] |= 1u << ((p - c0) & 31);
        p = kz_next(w, p, nb);
    }
    return p;
}

// lane's assumed entry after kz_spec: the predecessor's speculative exit; lane 0 (and, with a known
// entry e, every lane up to the one that holds e) its own first position
EZ_HD uint32_t kz_entry(int lane, uint32_t ps, uint32_t c, bool known, uint32_t e, uint32_t first, uint32_t prev_exit) {
    if (lane == 0) return known ? e : first;
    if (known && e >= ps + (uint32_t)lane * c) return e;  // (the chunks before the holder's, and the holder's)
    return prev_exit;
}

// The chunk's exit for the entry a (a >= c0: a predecessor leaves at or past its own end): a walk from
// a until a position the speculative walk visited (the rest of the chain is then the speculative
// one, and so is the exit) or the chunk's end.
template <int C>
EZ_HD uint32_t kz_verify(const KzWin &w, uint32_t sb, int lane, uint32_t nb, const uint32_t *bm, uint32_t sexit, uint32_t a) {
    uint32_t c0, ce;
    kz_chunk<C>(sb, lane, nb, c0, ce);
    if (a >= ce) return a;         // inside a token that spans the chunk (or a chunk past the stream's end)
    uint32_t q = a < c0 ? c0 : a;  // (a < c0 cannot happen: an exit is at or past its chunk's end)
    while (q < ce) {
        if ((bm[(q - c0) >> 5] >> ((q - c0) & 31)) & 1u) return sexit;
        q = kz_next(w, q, nb);
    }
    return q;
}

// One round of the repair after kz_verify, for every lane: lane jf is the lowest one whose assumed entry
// differs from its predecessor's verified exit e, the true chain's (the lanes below jf are right and
// stay so).  The lanes from jf on whose chunks end at or before e (a token spans them) pass e through,
// and the lane whose chunk holds e walks again from it; the lanes after it keep what they have: where
// that walk meets the speculative chain, as it mostly does, they were right all along.  (Walking
// them again from their predecessors' present exits was tried and is worse: a far exit that one
// lane's speculation took from a literal's bytes then moves down the wave a lane per round.)  jf rises
// every round: 63 rounds repair any super-block.  Returns whether the lane walked.
template <int C>
EZ_HD bool kz_fix(const KzWin &w, uint32_t sb, int lane, uint32_t nb, const uint32_t *bm, uint32_t sexit, int jf, uint32_t e, uint32_t &a,
                  uint32_t &x) {
    uint32_t c0, ce;
    kz_chunk<C>(sb, lane, nb, c0, ce);
    // (ce does not decrease with the lane: the lanes e passes, then the one that holds it, follow jf without a gap)
    if (lane < jf || (e < ce && e < c0)) return false;
    a = e;
    x = e >= ce ? e : kz_verify<C>(w, sb, lane, nb, bm, sexit, e);
    return e < ce;
}

struct KzSum {
    uint64_t out;   // output bytes of the chunk's tokens
    uint32_t maxd;  // its longest copy distance
    uint32_t fl;    // kZBad: a form k2_scan hands over, or a chain that does not leave at x;
                    // kZReset (and its argument in bits 8-15); kZResetLate: output before it in this chunk
};

// The true chain of the chunk, from its entry a to its exit x, with every form checked.
template <int C>
EZ_HD KzSum kz_sum(const KzWin &w, uint32_t sb, int lane, uint32_t nb, uint32_t a, uint32_t x, int32_t lim32, int64_t limit) {
    uint32_t c0, ce;
    kz_chunk<C>(sb, lane, nb, c0, ce);
    KzSum r{0, 0, 0};
    uint32_t p = a;
    while (p < ce) {
        K2Tok t;
        const V16 h = kz_at(w, p);
        const int k = k2_scan(h, (int32_t)p, (int32_t)nb, lim32, limit, t);
        if (k == kParseHandOver) {
            r.fl |= kZBad;
            return r;
        }
        if (k == kScanReset) {
            r.fl = (r.fl & 0xffu) | kZReset | (r.out ? kZResetLate : 0u) | (t.marg << 8);
        } else if (k == kParseToken) {
            r.out += (uint64_t)(uint32_t)t.L;
            r.maxd = t.cp && t.D > r.maxd ? t.D : r.maxd;
        }
        p = kz_clamp_pad((uint32_t)h.lo & 0xff, p + (uint32_t)t.adv, nb);
    }
    if (p != x) r.fl |= kZBad;  // (the fast step and k2_scan agree on every form k2_scan takes)
    return r;
}

// a MetaReset is valid only before any output (obefore: the stream's output before this chunk)
EZ_HD bool kz_reset_bad(uint32_t fl, uint64_t obefore) { return (fl & kZReset) && (obefore != 0 || (fl & kZResetLate)); }

// The stream's end (kj_scan's checks): the chain ends exactly at the input's end, the window is set
// before the first token, the longest distance lies within the window (ErrOverflow, reader.go:256-258,
// is the exact decoder's to report).  bsl: log2 of the window, -1 without a MetaReset.
EZ_HD bool kz_end_ok(uint32_t end, uint32_t nb, uint64_t total, int32_t bsl, uint32_t maxd) {
    if (end != nb) return false;
    if (total > 0 && bsl < 0) return false;
    if (bsl >= 0 && bsl < 30 && maxd > (1u << bsl)) return false;
    return true;
}

// The whole chain by one walker, in order: what the chunked walk computes, without the speculation.
// K2z's lane-per-stream kernel for large batches of short streams runs it, and the host check holds the
// chunked walk to it.  at(p): the 16 bytes at stream position p (zeros past the stream's end).
// Returns whether the stream is taken (else: hand it over); total = its output bytes.
template <class At>
EZ_HD bool kz_serial(At at, uint32_t nb, int32_t lim32, int64_t limit, uint64_t &total) {
    uint32_t p = 0, maxd = 0;
    int32_t bsl = -1;
    total = 0;
    while (p < nb) {
        K2Tok t;
        const V16 h = at(p);
        const int k = k2_scan(h, (int32_t)p, (int32_t)nb, lim32, limit, t);
        if (k == kParseHandOver || (k == kScanReset && total != 0)) return false;
        if (k == kScanReset) bsl = (int32_t)t.marg;
        if (k == kParseToken) {
            total += (uint64_t)(uint32_t)t.L;
            maxd = t.cp && t.D > maxd ? t.D : maxd;
        }
        p = kz_clamp_pad((uint32_t)h.lo & 0xff, p + (uint32_t)t.adv, nb);
    }
    return kz_end_ok(p, nb, total, bsl, maxd);
}

}  // namespace ez
