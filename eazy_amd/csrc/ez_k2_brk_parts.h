// ez_k2_brk_parts.h — the steps of K2b's parts route (ez_decompress_brk_parts.hip): the Break index of a
// long stream cut over many waves, as K2g's parts route cuts the segment query (ez_k2_segs_parts.h over
// ez_k2_parts.h's grid: parts of 64 chunks of C bytes, the warm-up chunk, the record of the chain that
// enters at ent, the in-order join at the true entry).
//
// K2b's state (KbState, ez_k2_brk.h) is K2g's with the Breaks so far in place of the cuts so far, and
// its rules at a Reset are kg_step's: so what a part's record must say about Resets, windows and
// distances is exactly KsRec (ez_k2_segs_parts.h, where the argument is written down), and ks_class and
// ks_take apply as they stand.  A Break adds nothing that depends on the incoming state: the Breaks of a
// piece of chain are a count, additive over pieces, and a Break's position is the entry state's total
// plus the output before it inside the part.  So the record is KsRec and the part's Breaks:
//   kq_sum     a lane's chunk of the true chain as a KqSum: ks_sum's fields and the chunk's Breaks (a
//              Break belongs to the chunk, and so to the part, that holds its 80);
//   kq_append  b after a in chain order: ks_append and an add (associative: the kernel's tree);
//   kq_class   ks_class with K2b's state;
//   kq_take    ks_take with K2b's state, and the record's Breaks;
//   KqEnt      a part's entry state, which the order pass leaves for the fill pass: total, position,
//              maxd, bsl, Breaks so far, live, and whether the part's true chain holds a Break (so a
//              part without one is never staged again);
//   kq_fills   whether the fill pass walks the part.
// All of them are functions over a byte pointer: tools/k2_brk_parts_check.hip runs them on the host.
#pragma once

#include "ez_k2_brk.h"
#include "ez_k2_segs_parts.h"

namespace ez {

// a piece of chain: K2g's sum and its Breaks
struct KqSum {
    KsSum s;
    uint32_t nbrk;
};

// The true chain of lane's chunk, from its entry a to its exit x (ks_sum's walk, which also counts the
// Breaks it steps over).
template <int C>
EZ_HD KqSum kq_sum(const KzWin &w, uint32_t sb, int lane, uint32_t nb, uint32_t a, uint32_t x, int32_t lim32, int64_t limit) {
    uint32_t c0, ce;
    kz_chunk<C>(sb, lane, nb, c0, ce);
    KqSum q{ks_none(), 0};
    KsSum &r = q.s;
    uint32_t md = 0;  // the longest distance since the last Reset
    uint32_t p = a;
    while (p < ce) {
        K2Tok t;
        const V16 h = kz_at(w, p);
        const int k = k2_scan(h, (int32_t)p, (int32_t)nb, lim32, limit, t);
        if (k == kParseHandOver) {
            r.fl |= kSWalk;
            return q;
        }
        if (k == kScanReset) {
            if (r.nreset == 0) {
                r.out0 = r.out;
                r.maxd0 = md;
            } else if (!kg_seg_ok(r.bslz, md)) {  // an interior segment
                r.fl |= kSWalk;
                return q;
            }
            if (r.out == 0) r.nlead++;
            r.nreset++;
            r.bslz = (int32_t)t.marg;
            md = 0;
        } else if (k == kParseToken) {
            r.out += (uint64_t)(uint32_t)t.L;
            md = t.cp && t.D > md ? t.D : md;
        } else if (kb_is_break(h, k)) {
            q.nbrk++;
        }
        p = kz_clamp_pad((uint32_t)h.lo & 0xff, p + (uint32_t)t.adv, nb);
    }
    if (p != x) r.fl |= kSWalk;  // (the fast step and k2_scan agree on every form k2_scan takes)
    r.maxdz = md;
    if (r.nreset == 0) {
        r.out0 = r.out;
        r.maxd0 = md;
    }
    return q;
}

// b after a in the chain's order
EZ_HD void kq_append(KqSum &a, const KqSum &b) {
    ks_append(a.s, b.s);
    a.nbrk += b.nbrk;  // (a part holds fewer than 2^31 Breaks; a marked sum's count is never read)
}

// a part's record: KsRec for the chain that enters at r.ent, and that chain's Breaks in the part
struct KqRec {
    KsRec r;
    uint32_t nbrk;
    uint32_t pad;
};
EZ_HD KqRec kq_rec(const KqSum &q, uint32_t ent, uint32_t exit) { return KqRec{ks_rec(q.s, ent, exit), q.nbrk, 0}; }
EZ_HD KqRec kq_rec_unsettled() { return KqRec{ks_rec_unsettled(), 0, 0}; }

// the stream's state in the order pass: K2b's, and the true chain's position
struct KqState {
    KbState st;
    uint32_t e;
};
EZ_HD KqState kq_start() { return KqState{kb_start(), 0}; }

// K2b's state as K2g's (the same fields but the count, which ks_class and ks_take's checks do not read)
EZ_HD KsState kq_as_ks(const KqState &S) { return KsState{KgState{S.st.total, S.st.maxd, S.st.bsl, 0, S.st.stop}, S.e}; }

// what the true chain at S.e does with the part that ends at pe and whose record is r (kSPass, kSJoin, kSAgain)
EZ_HD int kq_class(const KqState &S, uint32_t pe, const KqRec &r) { return ks_class(kq_as_ks(S), pe, r.r); }

// the record r (kq_class: kSJoin) applied to the state: what kb_step gives over the part's chain
EZ_HD void kq_take(KqState &S, const KqRec &r) {
    KsState g = kq_as_ks(S);
    ks_take(g, r.r);
    S.st.total = g.st.total;
    S.st.maxd = g.st.maxd;
    S.st.bsl = g.st.bsl;
    S.st.stop = g.st.stop;
    S.e = g.e;
    if (!g.st.stop) S.st.nbrk += r.nbrk;  // (a stopped stream goes whole to the exact decoder)
}

// a part's entry state, left by the order pass for every part of a stream that has parts
struct KqEnt {
    uint64_t total;
    uint32_t e;  // the true chain's entry into the part
    uint32_t maxd;
    int32_t bsl;
    uint32_t nbrk;   // the stream's Breaks before the part
    uint32_t live;   // the chain enters this part and the stream's walk has not stopped
    uint32_t holds;  // the part's true chain holds a Break
};
EZ_HD KqEnt kq_ent(const KqState &S, bool live, bool holds) {
    return KqEnt{S.st.total, S.e, S.st.maxd, S.st.bsl, S.st.nbrk, live ? 1u : 0u, holds ? 1u : 0u};
}
EZ_HD KqState kq_from(const KqEnt &n) { return KqState{KbState{n.total, n.maxd, n.bsl, n.nbrk, false}, n.e}; }

// whether the fill pass walks the part (of a stream that was not handed over)
EZ_HD bool kq_fills(const KqEnt &n) { return n.live != 0 && n.holds != 0; }

}  // namespace ez
