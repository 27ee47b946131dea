// ez_k2_ring.h — the LDS output ring of the wave-per-stream decoders (K2w, K2t): output
// position p lives at ring slot p & (R - 1); the ring is laid out as [16-byte guard][R bytes]
// [16-byte mirror of the first 16][16-byte guard] so that every 16-byte read at any slot is one
// contiguous LDS access.
#pragma once

#include "ez_bytes.h"
#include "ez_internal.h"

namespace ez {

typedef uint64_t __attribute__((aligned(1))) u64_ua;

// 16 bytes of position p from a ring of R bytes
template <int32_t R>
__device__ __forceinline__ V16 rld(const uint8_t *ring, int32_t p) {
    const uint8_t *q = ring + (p & (R - 1));
    return V16{*(const u64_ua *)q, *(const u64_ua *)(q + 8)};
}
// 16 bytes of position p into the ring: a write that wraps is written again R bytes lower (its
// head lands in the front guard), one into the first 16 bytes again R bytes higher (its tail
// lands in the back guard) -- whole 16-byte LDS writes only
template <int32_t R>
__device__ __forceinline__ void rst(uint8_t *ring, int32_t p, V16 v) {
    const int32_t r = p & (R - 1);
    *(u64_ua *)(ring + r) = v.lo;
    *(u64_ua *)(ring + r + 8) = v.hi;
    if (r > R - 16 || r < 16) {
        const int32_t r2 = r < 16 ? r + R : r - R;
        *(u64_ua *)(ring + r2) = v.lo;
        *(u64_ua *)(ring + r2 + 8) = v.hi;
    }
}
// the first n bytes (1..16) of v at d
__device__ __forceinline__ void put_n(uint8_t *d, V16 v, uint32_t n) {
    if (n >= 16) {
        *(u64_ua *)d = v.lo;
        *(u64_ua *)(d + 8) = v.hi;
    } else {
        put_small(d, v, n);
    }
}
// the 16 input bytes at y of a batch [lo, hi): bytes outside it read 0
__device__ __forceinline__ V16 ld_in(const uint8_t *y, const uint8_t *lo, const uint8_t *hi) {
    return y + 16 <= hi ? ld16v(y) : ld_clamped(y, lo, hi);
}
// n bytes (1..16) of position p into the ring, exact (pieces of one instruction never overlap)
template <int32_t R>
__device__ __forceinline__ void rput(uint8_t *ring, int32_t p, V16 v, uint32_t n) {
    const int32_t r = p & (R - 1);
    put_n(ring + r, v, n);
    if (r + (int32_t)n > R || r < 16) put_n(ring + (r < 16 ? r + R : r - R), v, n);
}

// output [fl, pos) from the ring to out by the whole wave, exact bytes (pos - fl <= R)
template <int32_t R>
__device__ __forceinline__ void flush_exact(const uint8_t *ring, uint8_t *out, int32_t fl, int32_t pos, int lane) {
    for (int32_t x = fl + 16 * lane; x < pos; x += 16 * 64) {
        const V16 v = rld<R>(ring, x);
        if (x + 16 <= pos) st16v(out + x, v);
        else put_small(out + x, v, (uint32_t)(pos - x));
    }
}

// Long literals (C4: a whole fp32 bucket is one literal) are not moved by the stream's one wave:
// the decoder records them (DeferLit) and kd_copy moves their bytes with the whole chip afterwards.
// A far copy reading from such a literal before kd_copy has run reads its bytes from the input.
constexpr int32_t kDeferMin = 16384;  // literals this long are deferred

// Stream s defers its nd-th literal (L bytes from its input position src to its output position pos):
// lane 0 takes a record of the batch-wide list (A.defer: the count, records from word 4; past
// defer_cap the record is dropped) and notes it in defs for the stream's own far reads
__device__ __forceinline__ void defer_record(const DecompressArgs &A, uint64_t s, int32_t *defs, int nd, int32_t pos, int32_t src, int32_t L, int lane) {
    if (lane == 0) {
        const uint32_t at = atomicAdd(&A.defer[0], 1u);
        if (at < A.defer_cap) ((DeferLit *)(A.defer + 4))[at] = DeferLit{A.in_off[s] + (uint64_t)src, A.out_off[s] + (uint64_t)pos, (uint64_t)L};
        defs[3 * nd] = pos;
        defs[3 * nd + 1] = src;
        defs[3 * nd + 2] = L;
    }
}

// the 16 output bytes at sq (< the ring's reach) from HBM, or from the input where they lie in one
// of the nd deferred literals (defs: {output position, input position, length} each, in LDS)
__device__ __forceinline__ V16 far16_def(const uint8_t *out, int32_t cap, const uint8_t *b, int32_t sq, int nd, const int32_t *defs) {
    V16 v{0, 0};
    for (int t = 0; t < 16; t++) {
        const int32_t y = sq + t;
        uint64_t c = y >= 0 ? out[y] : 0;
        for (int k = 0; k < nd; k++)
            if (y >= defs[3 * k] && y < defs[3 * k] + defs[3 * k + 2]) c = b[defs[3 * k + 1] + (y - defs[3 * k])];
        if (t < 8) v.lo |= c << (8 * t);
        else v.hi |= c << (8 * (t - 8));
    }
    return v;
}
__device__ __forceinline__ V16 far16(const uint8_t *out, int32_t cap, const uint8_t *b, int32_t sq, int nd, const int32_t *defs) {
    bool hit = false;
    for (int k = 0; k < nd; k++)
        if (sq < defs[3 * k] + defs[3 * k + 2] && sq + 16 > defs[3 * k]) hit = true;
    if (!hit) return ld_clamped16(out + sq, out, out + cap);
    return far16_def(out, cap, b, sq, nd, defs);
}

}  // namespace ez
