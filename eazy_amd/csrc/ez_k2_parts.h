// ez_k2_parts.h — the steps of K2z's parts route (ez_decompress_parts.hip): every stream's token
// chain cut over many waves.
//
// A stream is cut on a fixed grid of parts of 64 chunks of C input bytes (part k: stream positions
// [k * 64 * C, (k + 1) * 64 * C)); a stream without parts (an empty one, one of 2 GiB or more, one the
// automatic route's probe leaves to the wave route) is sized by the wave route.  The first pass gives every part a wave, which cannot know where
// the true chain enters its part: lane 0 warms up over the chunk before the part as the other lanes
// do over the chunk before theirs (kz_spec without a known entry), and the part's chain is the one
// that follows from lane 0's first position in the part (the walk is kz_walk, ez_k2_walk.h, and the sum
// ez_k2_size.h's).  The part's record (KpRec) holds that assumed entry, the chain's exit and its sums.
// The in-order pass, a wave per stream, then follows the true chain from part to part (kp_take): a
// part the chain enters at or past its end is passed through (a token spans it), a part whose record
// starts at the true entry is taken as recorded, and any other part is walked again from the true
// entry by the stream's wave, which is the wave route's step on that part.  So a record counts only
// where the true chain enters it: what a part's walk made of a literal's body is never added.
// All steps are functions over a byte pointer: tools/k2_size_parts_check.hip runs them on the host.
#pragma once

#include "ez_k2_size.h"

namespace ez {

constexpr uint32_t kPNoEntry = 0xffffffffu;  // KpRec.ent of a part whose first pass did not settle: never a true entry

// stream bytes of a part of chunk size c
constexpr uint32_t kp_part_bytes(uint32_t c) { return (uint32_t)kZLanes * c; }
// staged bytes of a part: the warm-up chunk before it, its chunks, the 16 bytes a header at its end reads
constexpr uint32_t kp_stage_bytes(uint32_t c) { return c + kp_part_bytes(c) + 16; }
// parts of a stream of nb bytes (none for an empty stream, or one too long for 32-bit positions)
EZ_HD uint32_t kp_parts_of(uint64_t nb, uint32_t c) {
    return nb >= (1ull << 31) ? 0u : (uint32_t)((nb + kp_part_bytes(c) - 1) / kp_part_bytes(c));
}
// The automatic route's probe: whether the stream's first kPProbeTokens tokens cover half of it or
// more.  Such a stream is the wave route's (it gets no parts): that route never reads a literal's
// body, while a part inside one is staged and walked for nothing (C4's 4 MiB literal).  A stream
// the probe lets through costs at most its parts' first pass.  at(p): the 16 bytes at stream
// position p < nb (zeros past the stream's end).
constexpr int kPProbeTokens = 8;
template <class At>
EZ_HD bool kp_probe_wave(At at, uint32_t nb) {
    uint32_t p = 0;
    for (int k = 0; k < kPProbeTokens && p < nb; k++) {
        const V16 h = at(p);
        p = kz_clamp_pad((uint32_t)h.lo & 0xff, p + (uint32_t)jadv_fast(h), nb);
    }
    return p >= nb - nb / 2;
}

// the first stream byte staged for the part at ps
EZ_HD uint32_t kp_stage_base(uint32_t ps, uint32_t c) { return ps >= c ? ps - c : 0u; }

// the stream of part g of the batch: the last s < count with base[s] <= g (base: the exclusive scan of
// the streams' part counts, count + 1 entries; streams without parts share their successor's base)
EZ_HD uint64_t kp_stream_of(const uint32_t *base, uint64_t count, uint32_t g) { return last_le(base, count, g); }

// a part's record: the first pass's result for the chain that enters at ent
struct KpRec {
    uint64_t out;   // output bytes of the chain's tokens in the part
    uint32_t ent;   // where the chain enters the part (at or past its start); kPNoEntry: not settled
    uint32_t exit;  // where it leaves (at or past the part's end)
    uint32_t maxd;  // its longest copy distance
    uint32_t fl;    // KzSum.fl of the whole part (kZResetLate: output in this part before a MetaReset)
};

// b after a in the chain's order (a: what precedes, sums of a part or of the stream so far)
EZ_HD void kp_append(KzSum &a, const KzSum &b) {
    if (b.fl & kZBad) a.fl |= kZBad;
    if (b.fl & kZReset) {
        const bool late = (b.fl & kZResetLate) || a.out != 0 || (a.fl & kZResetLate);
        a.fl = (a.fl & kZBad) | kZReset | (late ? kZResetLate : 0u) | (b.fl & 0xff00u);
    }
    a.out += b.out;
    a.maxd = b.maxd > a.maxd ? b.maxd : a.maxd;
}

// the stream's state in the in-order pass
struct KpState {
    uint64_t total;  // output bytes so far
    uint32_t e;      // the true chain's position
    uint32_t maxd;
    int32_t bsl;     // log2 of the window, -1 without a MetaReset
    bool bad;        // hand the stream over
};
EZ_HD KpState kp_start(uint64_t nb64) { return KpState{0, 0, 0, -1, nb64 >= (1ull << 31)}; }

enum : int { kPPass = 0, kPJoin = 1, kPWalk = 2 };
// what the true chain at S.e does with the part [ps, pe) whose record is r: pass through, take the
// record, or walk the part again from S.e
EZ_HD int kp_class(const KpState &S, uint32_t pe, const KpRec &r) { return S.e >= pe ? kPPass : (r.ent == S.e ? kPJoin : kPWalk); }

// the true chain through a part it entered at S.e, by the record r of that entry (the first pass's, or
// the walk's from S.e)
EZ_HD void kp_take(KpState &S, const KpRec &r) {
    if (r.ent != S.e || (r.fl & kZBad) || kz_reset_bad(r.fl, S.total)) {
        S.bad = true;
        return;
    }
    if (r.fl & kZReset) S.bsl = (int32_t)((r.fl >> 8) & 0xff);
    S.total += r.out;
    S.maxd = r.maxd > S.maxd ? r.maxd : S.maxd;
    S.e = r.exit;
}

EZ_HD bool kp_end_ok(const KpState &S, uint32_t nb) { return !S.bad && kz_end_ok(S.e, nb, S.total, S.bsl, S.maxd); }

}  // namespace ez
