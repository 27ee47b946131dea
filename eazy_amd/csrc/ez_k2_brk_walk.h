// ez_k2_brk_walk.h — the wave-level body of K2b: one block of 64 chunks of a stream's true chain with
// K2b's state (ez_k2_brk.h's steps over kz_walk, ez_k2_walk.h).  The wave route (ez_decompress_brk.hip)
// runs it over a stream's super-blocks one after the other; the parts route
// (ez_decompress_brk_parts.hip) runs it over one part, from the true chain's entry into it, in its
// order pass (parts walked again) and in its fill pass.  Device code; tools/k2_brk_check.hip and
// tools/k2_brk_parts_check.hip hold its host mirror.
#pragma once

#include "ez_k2_brk.h"
#include "ez_k2_walk.h"

namespace ez {

// The block of 64 chunks at ps of the stream b[0 .. nb), staged from sbase on (ps for a super-block,
// kp_stage_base(ps, C) for a part), from the true chain's position e in it, with the state
// (wave-uniform): kb_sum per lane, the in-order prefixes, the events in lane order through kb_walk.
// FILL: put(k, out) is called for Break k of the stream, by the lane that holds it (lane 0 for the
// Breaks behind an event).  Returns where the chain leaves the block; a stop is left in st.
template <int C, bool FILL, class Put>
__device__ __forceinline__ uint32_t kb_block(uint8_t *stage, uint32_t (*bm)[C / 32 + 1], const uint8_t *b, uint32_t nb, uint32_t sbase, uint32_t ps,
                                             uint32_t e, int32_t lim32, int64_t limit, KbState &st, Put put) {
    const int lane = lane_id();
    const auto none = [](uint32_t, uint64_t) {};
    const auto put0 = [&](uint32_t k, uint64_t out) {
        if (FILL && lane == 0) put(k, out);
    };
    const KzWalk k = kz_walk<C>(stage, bm, b, nb, sbase, ps, true, e);
    if (!k.settled) {
        st.stop = true;
        return e;
    }
    const KzWin w{stage, sbase};
    const KbSum r = kb_sum<C>(w, ps, lane, nb, k.a, k.x, lim32, limit, none);
    const uint64_t io = wscan_add_u64(r.out);
    const uint32_t ib = (uint32_t)wscan_add((int32_t)r.nbrk);  // (a block holds at most 32 x C Breaks)
    uint64_t ev = wballot(r.fl != 0);
    uint64_t base = 0;   // the prefixes taken into the state so far
    uint32_t bbase = 0;
    int from = 0;        // the first lane whose sums are not in the state yet
    // the lanes from .. to store their Breaks before their events: the state holds everything before lane `from`
    auto fill = [&](int to) {
        if (!FILL || !(lane >= from && lane <= to && r.nbrk != 0)) return;
        const uint64_t ob = st.total + (io - r.out - base);
        const uint32_t bb = st.nbrk + (ib - r.nbrk - bbase);
        (void)kb_sum<C>(w, ps, lane, nb, k.a, k.x, lim32, limit, [&](uint32_t i, uint64_t out) { put(bb + i, ob + out); });
    };
    while (ev) {
        const int j = ffs64(ev);
        ev &= ev - 1;
        fill(j);
        // the lanes before j, and lane j's tokens before its event
        const uint64_t ioj = __shfl(io, j, kWave);
        const uint32_t ibj = (uint32_t)__shfl((int)ib, j, kWave);
        st.total += ioj - base;
        base = ioj;
        st.nbrk += ibj - bbase;
        bbase = ibj;
        st.maxd = max(st.maxd, wmax_u32(lane >= from && lane <= j ? r.maxd : 0u));
        from = j + 1;
        kb_walk<C>(w, ps, j, nb, (uint32_t)__shfl((int)r.epos, j, kWave), (uint32_t)__shfl((int)k.x, j, kWave), lim32, limit, st, put0);
        if (st.stop) return e;
    }
    fill(kWave - 1);
    st.total += __shfl(io, kWave - 1, kWave) - base;
    st.nbrk += (uint32_t)__shfl((int)ib, kWave - 1, kWave) - bbase;
    st.maxd = max(st.maxd, wmax_u32(lane >= from ? r.maxd : 0u));
    return __shfl(k.x, kWave - 1, kWave);
}

}  // namespace ez
