// ez_k2_segs_parts.h — the steps of K2g's parts route (ez_decompress_segs_parts.hip): the segment
// query of a long concatenated stream cut over many waves, as K2z's parts route cuts the size query
// (ez_k2_parts.h: the fixed grid of parts of 64 chunks of C bytes, the warm-up chunk, the record of the
// chain that enters at ent, the in-order join at the true entry).  What K2g adds is its state
// (KgState, ez_k2_segs.h: the cuts so far, the window, the longest distance since the last cut, the
// stop), so a part's record must give, for any incoming state, exactly what kg_step gives token by
// token from that state.
//
// The incoming state decides two things only.  (i) Whether the Resets that precede the part's first
// output byte are cuts: they are iff total_in != 0 (Resets before the stream's first output byte stay
// in segment 0; each later one closes an empty segment).  (ii) Whether the segment that the part's
// first Reset closes passes kg_seg_ok(bsl_in, max(maxd_in, the longest distance before that Reset)).
// Every check at a later Reset of the part is decided inside it: its window is the previous Reset's
// and its distances lie between the two.  That holds in both views of (i), because every token has
// output (k2_scan: L >= 1), so a stretch without output has no distance either: a segment between two
// leading Resets passes whether it is checked (total_in != 0) or not, and the segment the first Reset
// after the part's first output closes is checked with the same window and distances in both views.
// (A state with total == 0 and maxd != 0 cannot arise; ks_class sends it to the walk all the same.)
// So the record (KsRec) holds: the output and longest distance before the first Reset, the number of
// Resets and how many lead the part's output, the window and longest distance after the last Reset,
// the part's whole output, and the exit.  The window the leading Resets leave is not kept: the only
// check that would read it is an interior one.
// A part whose chain holds a form k2_scan hands over, or an interior segment that fails kg_seg_ok, or
// whose walk did not settle, is marked kSWalk: the stream stops in it, and the in-order pass walks
// that one part with kg_cuts from the true state.
//   ks_sum     a lane's chunk of the true chain as a KsSum;
//   ks_append  b after a in chain order (associative: the kernel reduces the lanes as a tree);
//   ks_class   what the true chain does with a part: pass through, take the record, walk again;
//   ks_take    the record applied to the state;
//   KsEnt      a part's entry state, which the in-order pass leaves for the fill pass: the fill walks
//              the part's chain from it with kg_sum / kg_cuts, whose cut(i, pos, out) carries the
//              stream's own cut index (st.ncut counts on from the entry state's);
//   ks_slot    a cut's output position in the caller's slot, clamped to it.
// All of them are functions over a byte pointer: tools/k2_segs_parts_check.hip runs them on the host.
#pragma once

#include "ez_k2_parts.h"
#include "ez_k2_segs.h"

namespace ez {

enum : uint32_t { kSWalk = 1 };  // KsSum.fl, KsRec.fl: not summarised, walk it from the true state

// a piece of chain (a lane's chunk, several in order, a part)
struct KsSum {
    uint64_t out;     // its output bytes
    uint64_t out0;    // those before its first Reset (out without one)
    uint32_t maxd0;   // the longest distance before its first Reset (the whole piece's without one)
    uint32_t maxdz;   // the longest distance after its last Reset (maxd0 without one)
    uint32_t nreset;  // its Resets
    uint32_t nlead;   // those of them with no output of the piece before them
    int32_t bslz;     // the last Reset's window (-1 without one)
    uint32_t fl;      // kSWalk
};
EZ_HD KsSum ks_none() { return KsSum{0, 0, 0, 0, 0, 0, -1, 0}; }

EZ_HD uint32_t ks_max(uint32_t a, uint32_t b) { return a > b ? a : b; }

// The true chain of lane's chunk, from its entry a to its exit x.
template <int C>
EZ_HD KsSum ks_sum(const KzWin &w, uint32_t sb, int lane, uint32_t nb, uint32_t a, uint32_t x, int32_t lim32, int64_t limit) {
    uint32_t c0, ce;
    kz_chunk<C>(sb, lane, nb, c0, ce);
    KsSum r = ks_none();
    uint32_t md = 0;  // the longest distance since the last Reset
    uint32_t p = a;
    while (p < ce) {
        K2Tok t;
        const V16 h = kz_at(w, p);
        const int k = k2_scan(h, (int32_t)p, (int32_t)nb, lim32, limit, t);
        if (k == kParseHandOver) {
            r.fl |= kSWalk;
            return r;
        }
        if (k == kScanReset) {
            if (r.nreset == 0) {
                r.out0 = r.out;
                r.maxd0 = md;
            } else if (!kg_seg_ok(r.bslz, md)) {  // an interior segment
                r.fl |= kSWalk;
                return r;
            }
            if (r.out == 0) r.nlead++;
            r.nreset++;
            r.bslz = (int32_t)t.marg;
            md = 0;
        } else if (k == kParseToken) {
            r.out += (uint64_t)(uint32_t)t.L;
            md = t.cp && t.D > md ? t.D : md;
        }
        p = kz_clamp_pad((uint32_t)h.lo & 0xff, p + (uint32_t)t.adv, nb);
    }
    if (p != x) r.fl |= kSWalk;  // (the fast step and k2_scan agree on every form k2_scan takes)
    r.maxdz = md;
    if (r.nreset == 0) {
        r.out0 = r.out;
        r.maxd0 = md;
    }
    return r;
}

// b after a in the chain's order
EZ_HD void ks_append(KsSum &a, const KsSum &b) {
    if ((a.fl | b.fl) & kSWalk) {
        a.fl |= kSWalk;
        return;
    }
    if (b.nreset == 0) {
        a.out += b.out;
        a.maxdz = ks_max(a.maxdz, b.maxd0);
        if (a.nreset == 0) {
            a.out0 = a.out;
            a.maxd0 = a.maxdz;
        }
        return;
    }
    if (a.nreset == 0) {
        a.nlead = a.out == 0 ? b.nlead : 0u;
        a.out0 = a.out + b.out0;
        a.maxd0 = ks_max(a.maxd0, b.maxd0);
    } else {
        // the segment from a's last Reset to b's first is interior to the joined piece
        if (!kg_seg_ok(a.bslz, ks_max(a.maxdz, b.maxd0))) {
            a.fl |= kSWalk;
            return;
        }
        if (a.out == 0) a.nlead += b.nlead;  // (all of a's Resets lead, and so do b's leading ones)
    }
    a.nreset += b.nreset;
    a.out += b.out;
    a.bslz = b.bslz;
    a.maxdz = b.maxdz;
}

// a part's record: the first pass's result for the chain that enters at ent
struct KsRec {
    uint64_t out, out0;
    uint32_t ent;   // where the chain enters the part (at or past its start); kPNoEntry: not settled
    uint32_t exit;  // where it leaves (at or past the part's end)
    uint32_t maxd0, maxdz, nreset, nlead;
    int32_t bslz;
    uint32_t fl;
};
EZ_HD KsRec ks_rec(const KsSum &s, uint32_t ent, uint32_t exit) {
    return KsRec{s.out, s.out0, ent, exit, s.maxd0, s.maxdz, s.nreset, s.nlead, s.bslz, s.fl};
}
EZ_HD KsRec ks_rec_unsettled() { return KsRec{0, 0, kPNoEntry, 0, 0, 0, 0, 0, -1, kSWalk}; }

// the stream's state in the in-order pass: K2g's, and the true chain's position
struct KsState {
    KgState st;
    uint32_t e;
};
EZ_HD KsState ks_start() { return KsState{kg_start(), 0}; }

enum : int { kSPass = 0, kSJoin = 1, kSAgain = 2 };
// what the true chain at S.e does with the part that ends at pe and whose record is r: pass through (a
// token spans it), take the record, or walk the part again from S.e with the true state
EZ_HD int ks_class(const KsState &S, uint32_t pe, const KsRec &r) {
    if (S.e >= pe) return kSPass;
    if (r.ent != S.e || (r.fl & kSWalk) || (S.st.total == 0 && S.st.maxd != 0)) return kSAgain;
    return kSJoin;
}

// the record r (ks_class: kSJoin) applied to the state: what kg_step gives over the part's chain
EZ_HD void ks_take(KsState &S, const KsRec &r) {
    KgState &t = S.st;
    if (r.nreset == 0) {
        t.total += r.out;
        t.maxd = ks_max(t.maxd, r.maxd0);
    } else if (t.total == 0 && r.nlead != 0) {  // (i): the leading Resets are no cuts; the others passed inside
        t.ncut += r.nreset - r.nlead;
        t.total += r.out;
        t.maxd = r.maxdz;
        t.bsl = r.bslz;
    } else {  // (ii): the first Reset closes the segment the state brings
        const uint32_t md = ks_max(t.maxd, r.maxd0);
        t.total += r.out0;
        if (!kg_seg_ok(t.bsl, md)) {
            t.maxd = md;
            t.stop = true;
            return;
        }
        t.ncut += r.nreset;
        t.total += r.out - r.out0;
        t.maxd = r.maxdz;
        t.bsl = r.bslz;
    }
    S.e = r.exit;
}

// a part's entry state, left by the in-order pass for every part of a stream that has parts
struct KsEnt {
    uint64_t total;
    uint32_t e;  // the true chain's entry into the part
    uint32_t maxd;
    int32_t bsl;
    uint32_t ncut;
    uint32_t live;  // the chain enters this part and the stream's walk has not stopped
    uint32_t pad;
};
EZ_HD KsEnt ks_ent(const KsState &S, bool live) { return KsEnt{S.st.total, S.e, S.st.maxd, S.st.bsl, S.st.ncut, live ? 1u : 0u, 0}; }
EZ_HD KsState ks_from(const KsEnt &n) { return KsState{KgState{n.total, n.maxd, n.bsl, n.ncut, false}, n.e}; }

// whether the fill pass walks the part: its record holds a Reset (or was not summarised) and the chain is live there
EZ_HD bool ks_fills(const KsRec &r, const KsEnt &n) { return n.live != 0 && (r.nreset != 0 || (r.fl & kSWalk) || r.ent != n.e); }

// a cut's output position in the slot [o0, o1): o0 + the output before it, clamped to the slot
EZ_HD uint64_t ks_slot(uint64_t o0, uint64_t o1, uint64_t out) { return out < o1 - o0 ? o0 + out : o1; }

}  // namespace ez
