// ez_k2_walk.h — the wave-level walk of K2z and K2g: how one wave finds the true token chain through
// a block of 64 chunks, a chunk per lane (the per-lane steps: ez_k2_size.h).  The wave route
// (ez_decompress_size.hip), the parts route (ez_decompress_parts.hip) and the segment query
// (ez_decompress_segs.hip) all run kz_walk, then their own sum over each lane's true chain, and
// reduce it with wscan_add_u64 / wmax_u32 (ez_wave.h).  Device code; tools/k2_check_common.h holds its
// host mirror (emu_walk), which the three host checks run.
#pragma once

#include "ez_k2_size.h"
#include "ez_wave.h"

namespace ez {

// at(p): the 16 bytes at position p of the stream b[0 .. nb) in global memory, zeros past its end
struct kz_global_at {
    const uint8_t *b;
    uint32_t nb;
    __device__ __forceinline__ kz_global_at(const uint8_t *b_, uint32_t nb_) : b(b_), nb(nb_) {}
    __device__ __forceinline__ V16 operator()(uint32_t p) const { return p + 16 <= nb ? ld16v(b + p) : ld_clamped(b + p, b, b + nb); }
};

// The stream bytes [sbase, min(nb, end) + 16) go to stage[0 ..) with 16-byte loads, clamped to the
// stream (zeros past its end): end - sbase + 16 bytes at most, the staged array's size, a multiple of
// 16.  Every later step reads LDS.
__device__ __forceinline__ void kz_stage(uint8_t *stage, const uint8_t *b, uint32_t nb, uint32_t sbase, uint32_t end) {
    __syncthreads();  // (the previous block's reads are done)
    const uint32_t need = (nb < end ? nb : end) + 16 - sbase;
    for (uint32_t o = (uint32_t)lane_id() * 16; o < need; o += kWave * 16) {
        const uint32_t y = sbase + o;
        V16 v{0, 0};
        if (y + 16 <= nb) v = ld16v(b + y);
        else if (y < nb) v = ld_clamped(b + y, b, b + nb);
        typedef uint64_t __attribute__((aligned(8))) u64a;
        *(u64a *)(stage + o) = v.lo;
        *(u64a *)(stage + o + 8) = v.hi;
    }
    __syncthreads();
}

// what kz_walk leaves in each lane
struct KzWalk {
    uint32_t a, x;  // the lane's entry into its chunk on the true chain, and its exit
    bool settled;   // (uniform) every lane's entry is its predecessor's exit; else hand the stream over
};

// The block of 64 chunks at ps of the stream b[0 .. nb), by the whole wave: stage it from sbase on (ps,
// or kp_stage_base(ps, C) for a part's warm-up chunk), speculate, take entries, verify, and repair the
// lowest wrong lane first (kz_fix; the lanes a spanning token covers take its end in the same round) for
// at most kZFixRounds rounds.  known, e: kz_spec's; a super-block is (sbase = ps, known, e = ps).  The
// chain that settles is the one from lane 0's entry.  stage holds the bytes afterwards: KzWin{stage, sbase}.
template <int C>
__device__ __forceinline__ KzWalk kz_walk(uint8_t *stage, uint32_t (*bm)[C / 32 + 1], const uint8_t *b, uint32_t nb, uint32_t sbase,
                                          uint32_t ps, bool known, uint32_t e) {
    const int lane = lane_id();
    kz_stage(stage, b, nb, sbase, ps + (uint32_t)kZLanes * C);
    const KzWin w{stage, sbase};
    uint32_t first;
    const uint32_t sexit = kz_spec<C>(w, ps, lane, nb, known, e, bm[lane], first);
    KzWalk r;
    r.a = kz_entry(lane, ps, C, known, e, first, __shfl_up(sexit, 1, kWave));
    // (lane 0 with a known entry is on the true chain: kz_verify would return sexit at its first step; leaving
    // that step to it measured up to 1.6 % slower on the super-block kernels)
    r.x = known && lane == 0 ? sexit : kz_verify<C>(w, ps, lane, nb, bm[lane], sexit, r.a);
    r.settled = true;
    for (int round = 0;; round++) {
        const uint32_t px = __shfl_up(r.x, 1, kWave);
        const uint64_t wrong = wballot(lane > 0 && r.a != px);
        if (wrong == 0) break;
        if (round >= kZFixRounds) {
            r.settled = false;
            break;
        }
        const int jf = ffs64(wrong);
        kz_fix<C>(w, ps, lane, nb, bm[lane], sexit, jf, (uint32_t)__shfl((int)r.x, jf - 1, kWave), r.a, r.x);
    }
    return r;
}

}  // namespace ez
