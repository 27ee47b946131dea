// ez_k2_brk.h — the per-lane steps of K2b, the batch Break index (ez_decompress_brk.hip): the output
// position of every Break meta of a stream, without decoding.
//
// Writer.WriteBreak (writer.go:352-366) writes the two bytes 80 1f; Reader.Read returns ErrBreak there
// and stays valid (reader.go:66-75, :312-313): a Break's position is the number of bytes the Reader has
// produced by then.  It depends on the tokens' lengths alone, so K2b follows the true token chain as
// K2z and K2g do (kz_walk, ez_k2_walk.h, over ez_k2_size.h's steps) with K2g's bookkeeping (ez_k2_segs.h)
// without its cuts: the total counts across MetaResets, the window and the longest distance start
// again at each Reset with output before it.  In place of kg_sum and kg_cuts:
//   kb_sum     a lane walks its chunk's true chain with the full k2_scan up to the chunk's first event,
//              a MetaReset or a form k2_scan hands over, and records the chunk's output bytes, longest
//              distance and Breaks before it; brk(k, out) is called for Break k of the chunk with the
//              chunk's output before it (the count pass passes a callback that does nothing, the fill
//              pass runs the step again with the lane's bases from the wave's in-order prefix);
//   kb_walk    from an event to the chunk's exit, with the stream's state (every lane runs the same
//              walk): brk(k, out) for Break k of the stream.  A segment that fails K2z's checks
//              (kg_seg_ok) or a form k2_scan hands over stops the walk, and a stop sends the whole
//              stream to the exact decoder: nothing partial is kept;
//   kb_end_ok  kg_end_ok's test at the stream's end.
// kb_serial is the whole chain by one walker, which tools/k2_brk_check.hip holds the chunked walk to.
// All of them are functions over a byte pointer (the host check runs them over 64 emulated lanes).
#pragma once

#include "ez_k2_segs.h"

namespace ez {

// a step k2_scan skipped is a Break: the meta 80 1f (kMetaBreak, no length)
EZ_HD bool kb_is_break(const V16 h, int k) { return k == kParseSkip && ((uint32_t)h.lo & 0xffffu) == 0x1f80u; }

struct KbSum {
    uint64_t out;   // output bytes of the chunk's tokens before the event (the whole chunk's without one)
    uint32_t maxd;  // the longest copy distance among them
    uint32_t nbrk;  // the Breaks among them
    uint32_t fl;    // 0, kZReset or kZBad: the event
    uint32_t epos;  // the event's input position
};

// The true chain of the chunk from its entry a, up to its first event or its exit x.
template <int C, class Brk>
EZ_HD KbSum kb_sum(const KzWin &w, uint32_t sb, int lane, uint32_t nb, uint32_t a, uint32_t x, int32_t lim32, int64_t limit, Brk brk) {
    uint32_t c0, ce;
    kz_chunk<C>(sb, lane, nb, c0, ce);
    KbSum r{0, 0, 0, 0, a};
    uint32_t p = a;
    while (p < ce) {
        K2Tok t;
        const V16 h = kz_at(w, p);
        const int k = k2_scan(h, (int32_t)p, (int32_t)nb, lim32, limit, t);
        if (k == kParseHandOver || k == kScanReset) {
            r.fl = k == kScanReset ? kZReset : kZBad;
            r.epos = p;
            return r;
        }
        if (k == kParseToken) {
            r.out += (uint64_t)(uint32_t)t.L;
            r.maxd = t.cp && t.D > r.maxd ? t.D : r.maxd;
        } else if (kb_is_break(h, k)) {
            brk(r.nbrk, r.out);
            r.nbrk++;
        }
        p = kz_clamp_pad((uint32_t)h.lo & 0xff, p + (uint32_t)t.adv, nb);
    }
    if (p != x) return KbSum{0, 0, 0, kZBad, a};  // (kb_walk walks the chunk again and stops the stream)
    return r;
}

// the stream's state in chain order
struct KbState {
    uint64_t total;  // output bytes so far, across Resets
    uint32_t maxd;   // the longest distance since the last Reset with output before it
    int32_t bsl;     // log2 of the window, -1 without a MetaReset
    uint32_t nbrk;   // Breaks so far
    bool stop;       // the stream goes to the exact decoder
};
EZ_HD KbState kb_start() { return KbState{0, 0, -1, 0, false}; }

// One step of the chain at p with the state: returns the next position.  brk(k, out): Break k of the
// stream, with out output bytes before it.  (kg_step's bookkeeping: a Reset with output before it closes
// a segment, which has to pass kg_seg_ok.)
template <class Brk>
EZ_HD uint32_t kb_step(const V16 h, uint32_t p, uint32_t nb, int32_t lim32, int64_t limit, KbState &st, Brk brk) {
    K2Tok t;
    const int k = k2_scan(h, (int32_t)p, (int32_t)nb, lim32, limit, t);
    if (k == kParseHandOver) {
        st.stop = true;
        return p;
    }
    if (k == kScanReset) {
        if (st.total != 0) {
            if (!kg_seg_ok(st.bsl, st.maxd)) {
                st.stop = true;
                return p;
            }
            st.maxd = 0;
        }
        st.bsl = (int32_t)t.marg;
    } else if (k == kParseToken) {
        st.total += (uint64_t)(uint32_t)t.L;
        st.maxd = t.cp && t.D > st.maxd ? t.D : st.maxd;
    } else if (kb_is_break(h, k)) {
        brk(st.nbrk, st.total);
        st.nbrk++;
    }
    return kz_clamp_pad((uint32_t)h.lo & 0xff, p + (uint32_t)t.adv, nb);
}

// The chain of lane's chunk from the event at e to the chunk's exit x, with the state.
template <int C, class Brk>
EZ_HD void kb_walk(const KzWin &w, uint32_t sb, int lane, uint32_t nb, uint32_t e, uint32_t x, int32_t lim32, int64_t limit, KbState &st,
                   Brk brk) {
    uint32_t c0, ce;
    kz_chunk<C>(sb, lane, nb, c0, ce);
    uint32_t p = e;
    while (p < ce && !st.stop) p = kb_step(kz_at(w, p), p, nb, lim32, limit, st, brk);
    if (!st.stop && p != x) st.stop = true;  // (the fast step and k2_scan agree on every form k2_scan takes)
}

// The stream's end (kg_end_ok's test): the walk went through, the chain ended at the input's end, and
// the last segment passes kz_end_ok's checks.  Then the stream decodes to st.total bytes with EZ_OK and
// its Breaks are the walk's; else the exact decoder lists them.
EZ_HD bool kb_end_ok(const KbState &st, uint32_t end, uint32_t nb) { return !st.stop && kz_end_ok(end, nb, st.total, st.bsl, st.maxd); }

// The whole chain by one walker, in order: what the chunked walk computes, without the speculation.
// at(p): the 16 bytes at stream position p (zeros past the stream's end); *end (optional): where the
// chain ended.
template <class At, class Brk>
EZ_HD KbState kb_serial(At at, uint32_t nb, int32_t lim32, int64_t limit, Brk brk, uint32_t *end = nullptr) {
    KbState st = kb_start();
    uint32_t p = 0;
    while (p < nb && !st.stop) p = kb_step(at(p), p, nb, lim32, limit, st, brk);
    if (end) *end = p;
    return st;
}

}  // namespace ez
