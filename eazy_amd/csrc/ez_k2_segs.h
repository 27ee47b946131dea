// ez_k2_segs.h — the per-lane steps of K2g, the batch segment query (ez_decompress_segs.hip): where a
// stream that holds MetaResets after output can be cut into streams that decode on their own.
//
// Reader.reset (reader.go:327-344) zeroes the block and sets r.pos = 0, so everything from a MetaReset
// on decodes exactly like a fresh stream: a stream with k Resets after output is k + 1 streams whose
// input and output ranges tile its own.  The cuts lie on the true token chain (a literal's body may
// hold 80 10 14), which K2g follows as K2z does (kz_walk, ez_k2_walk.h, over ez_k2_size.h's steps).
// In place of kz_sum:
//   kg_sum     a lane walks its chunk's true chain with the full k2_scan up to the chunk's first event,
//              a MetaReset or a form k2_scan hands over, and records the event's input position (a
//              Reset's is its 0x80 tag byte: padding before it belongs to what came before), the chunk's
//              output bytes and longest distance before it;
//   kg_cuts    from an event to the chunk's exit, with the stream's state (the wave's in-order prefix
//              supplies it; every lane runs the same walk): each Reset with output before it in the
//              stream closes a segment, and is a cut if that segment passes K2z's checks (kg_seg_ok:
//              kz_end_ok's, with bsl and maxd starting again at each cut).  The first segment that
//              fails, or holds a form k2_scan hands over, stops the stream's walk: the cuts so far
//              stand and the rest of the stream is the last segment, which the decoders see exactly
//              as they see it today.
//   kg_end_ok  the size query's end step (k2g_size): a walk that went through, with a last segment that
//              passes too, gives the stream's decoded length, the state's total.
// kg_serial is the whole chain by one walker, which tools/k2_segs_check.hip and
// tools/k2_segs_size_check.hip hold the chunked walk to.
// All of them are functions over a byte pointer (the host check runs them over 64 emulated lanes).
#pragma once

#include "ez_k2_size.h"

namespace ez {

struct KgSum {
    uint64_t out;   // output bytes of the chunk's tokens before the event (the whole chunk's without one)
    uint32_t maxd;  // the longest copy distance among them
    uint32_t fl;    // 0, kZReset or kZBad: the event
    uint32_t epos;  // the event's input position
};

// The true chain of the chunk from its entry a, up to its first event or its exit x.
template <int C>
EZ_HD KgSum kg_sum(const KzWin &w, uint32_t sb, int lane, uint32_t nb, uint32_t a, uint32_t x, int32_t lim32, int64_t limit) {
    uint32_t c0, ce;
    kz_chunk<C>(sb, lane, nb, c0, ce);
    KgSum r{0, 0, 0, a};
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
        }
        p = kz_clamp_pad((uint32_t)h.lo & 0xff, p + (uint32_t)t.adv, nb);
    }
    if (p != x) return KgSum{0, 0, kZBad, a};  // (kg_cuts walks the chunk again and stops the stream)
    return r;
}

// the stream's state in chain order
struct KgState {
    uint64_t total;  // output bytes so far
    uint32_t maxd;   // the longest distance since the last cut
    int32_t bsl;     // log2 of the window, -1 without a MetaReset
    uint32_t ncut;   // cuts so far
    bool stop;       // the walk of this stream is over: no more cuts
};
EZ_HD KgState kg_start() { return KgState{0, 0, -1, 0, false}; }

// the checks on a segment that a cut closes (kz_end_ok's; the segment holds output, or it is empty
// and follows a cut, whose Reset set its window)
EZ_HD bool kg_seg_ok(int32_t bsl, uint32_t maxd) { return bsl >= 0 && !(bsl < 30 && maxd > (1u << bsl)); }

// One step of the chain at p with the state: returns the next position.  cut(i, pos, out): cut i of the
// stream, at input position pos with out output bytes before it.
template <class Cut>
EZ_HD uint32_t kg_step(const V16 h, uint32_t p, uint32_t nb, int32_t lim32, int64_t limit, KgState &st, Cut cut) {
    K2Tok t;
    const int k = k2_scan(h, (int32_t)p, (int32_t)nb, lim32, limit, t);
    if (k == kParseHandOver) {
        st.stop = true;
        return p;
    }
    if (k == kScanReset) {
        if (st.total != 0) {  // output before it: the Reset closes a segment
            if (!kg_seg_ok(st.bsl, st.maxd)) {
                st.stop = true;
                return p;
            }
            cut(st.ncut, p, st.total);
            st.ncut++;
            st.maxd = 0;
        }
        st.bsl = (int32_t)t.marg;
    } else if (k == kParseToken) {
        st.total += (uint64_t)(uint32_t)t.L;
        st.maxd = t.cp && t.D > st.maxd ? t.D : st.maxd;
    }
    return kz_clamp_pad((uint32_t)h.lo & 0xff, p + (uint32_t)t.adv, nb);
}

// The chain of lane's chunk from the event at e to the chunk's exit x, with the state.
template <int C, class Cut>
EZ_HD void kg_cuts(const KzWin &w, uint32_t sb, int lane, uint32_t nb, uint32_t e, uint32_t x, int32_t lim32, int64_t limit, KgState &st,
                   Cut cut) {
    uint32_t c0, ce;
    kz_chunk<C>(sb, lane, nb, c0, ce);
    uint32_t p = e;
    while (p < ce && !st.stop) p = kg_step(kz_at(w, p), p, nb, lim32, limit, st, cut);
    if (!st.stop && p != x) st.stop = true;  // (the fast step and k2_scan agree on every form k2_scan takes)
}

// The stream's end for the size query behind K2z (k2g_size, ez_decompress_segs.hip): the walk went
// through without a stop, the chain ended at position end, and the last segment, the one since the
// last cut, passes kz_end_ok's checks as every segment before it passed kg_seg_ok's.  Then the stream
// decodes to st.total bytes with EZ_OK; else it is handed on.
EZ_HD bool kg_end_ok(const KgState &st, uint32_t end, uint32_t nb) { return !st.stop && kz_end_ok(end, nb, st.total, st.bsl, st.maxd); }

// The whole chain by one walker, in order: what the chunked walk computes, without the speculation.
// at(p): the 16 bytes at stream position p (zeros past the stream's end); *end (optional): where the
// chain ended.
template <class At, class Cut>
EZ_HD KgState kg_serial(At at, uint32_t nb, int32_t lim32, int64_t limit, Cut cut, uint32_t *end = nullptr) {
    KgState st = kg_start();
    uint32_t p = 0;
    while (p < nb && !st.stop) p = kg_step(at(p), p, nb, lim32, limit, st, cut);
    if (end) *end = p;
    return st;
}

}  // namespace ez
