// ez_k1_emit.h — K1e's token writer of one stream by one wave (emit_stream) and the byte copies
// the token writers share.  k1_emit runs it per stream (ez_k1_emit.hip), and k1_long_ring<true>
// runs it inside its own block, one launch per Write on a handle (ez_k1_long.hip), so it lives in a
// header.
#pragma once

#include "ez_k1_device.h"

namespace ez {
namespace k1 {

// 16 bytes at y of the batch [lo, hi) (bytes outside read as 0)
__device__ __forceinline__ V16 ld16_in(const uint8_t *y, const uint8_t *lo, const uint8_t *hi) {
    return y + 16 <= hi ? ld16v(y) : ld_clamped(y, lo, hi);
}

// copy L bytes src -> dst, one lane
__device__ __forceinline__ void copy_lane(uint8_t *dst, const uint8_t *src, int32_t L, const uint8_t *lo, const uint8_t *hi) {
    int32_t q = 0;
    for (; q + 16 <= L; q += 16) st16v(dst + q, ld16_in(src + q, lo, hi));
    if (q < L) put_small(dst + q, ld16_in(src + q, lo, hi), (uint32_t)(L - q));
}

constexpr int32_t kLongLit = 96;  // literals this long are copied by the whole wave
constexpr int kEmitStage = 320;    // records of a stream staged in LDS by k1_emit (C1: ~220 per stream)
constexpr int32_t kEmitIn = 4096;  // streams this short have their bytes staged in LDS by k1_emit too
typedef uint64_t __attribute__((aligned(1))) u64_lds_ua;
// copy L bytes from LDS (src) -> dst, one lane
__device__ __forceinline__ void copy_lane_lds(uint8_t *dst, const uint8_t *src, int32_t L) {
    int32_t q = 0;
    for (; q + 16 <= L; q += 16) st16v(dst + q, V16{*(const u64_lds_ua *)(src + q), *(const u64_lds_ua *)(src + q + 8)});
    if (q < L) put_small(dst + q, V16{*(const u64_lds_ua *)(src + q), *(const u64_lds_ua *)(src + q + 8)}, (uint32_t)(L - q));
}

// WIDE: k1_long's 16-byte records, and (spec_mode) the streams K1x hands over: their header and
// first tokens are written already, the output continues at spec[s].op with the pending literal
// from spec[s].done; streams K1x finished are skipped
// the token writer of stream s (wave-uniform) by one wave
template <bool WIDE>
__device__ __forceinline__ void emit_stream(const CompressArgs &A, const uint64_t *recs, uint64_t rcap, const uint64_t s, const int lane,
                                            uint64_t *stage = nullptr, uint8_t *sin = nullptr) {
    const bool spec = WIDE && A.spec_mode != 0;
    if (spec && A.spec[s].flags != 0) return;
    const uint8_t *lo = A.in, *hi = A.in + A.in_off[A.count];
    const uint8_t *p = A.in + A.in_off[s];
    const int32_t n = (int32_t)(A.in_off[s + 1] - A.in_off[s]);
    uint8_t *out = A.out + A.out_off[s];
    const int64_t cap64 = (int64_t)(A.out_off[s + 1] - A.out_off[s]);
    const int32_t cap = cap64 > 0x7fffffff ? 0x7fffffff : (int32_t)cap64;
    const uint64_t pr = A.out_size[s];
    const uint64_t m64 = pr & 0xffffffffffffull;
    const int32_t m = (int32_t)(m64 < rcap ? m64 : rcap);
    int err = (int)(pr >> 48);
    const uint64_t *rec = recs + s * rcap;

    // header (writer.go:495-517): magic + reset, or reset alone
    const int32_t H = spec ? (int32_t)A.spec[s].op : (A.header ? (A.append_magic ? 9 : 3) : 0);
    // a stream the parse refused before its first record (longer than max_len, more Writes than
    // max_writes) gets its status, size 0 and no byte in its slot, as K1x's refused streams
    const bool refused = !spec && err != 0 && m == 0;
    if (refused || (!spec && H > cap)) {
        if (lane == 0) {
            A.out_size[s] = 0;
            if (A.status) A.status[s] = refused ? err : EZ_ENOSPC;
        }
        return;
    }
    if (lane == 0 && !spec && H > 0) {
        const int32_t bsl = (int32_t)__builtin_ctzll((uint64_t)A.bs);
        const uint64_t hm = A.append_magic ? (0x141080797a616502ull << 8 | 0x80) : (0x80ull | 0x10ull << 8 | (uint64_t)bsl << 16);
        const V16 hv{hm, A.append_magic ? (uint64_t)bsl : 0ull};
        put_small(out, hv, (uint32_t)H);
    }
    int32_t op = H, done = spec ? (int32_t)A.spec[s].done : 0;
    bool full = false;
    // (stage: the stream's records in LDS, read with one round trip for all of them instead of one
    // per 64-record chunk, each of which waited for the previous chunk's stores -- vmcnt is in order)
    const bool staged = !WIDE && stage != nullptr && m <= kEmitStage;
    // (sin: the stream's bytes in LDS too, loaded with the records, so the literals' bytes are LDS
    // reads instead of a load round trip per 64 tokens: C1's 4 KiB streams)
    const bool inl = staged && sin != nullptr && n <= kEmitIn;
    if (!WIDE && staged) {
        uint64_t t[kEmitStage / 64];
        V16 u[kEmitIn / 1024];
#pragma unroll
        for (int q = 0; q < kEmitStage / 64; q++) t[q] = q * 64 + lane < m ? rec[q * 64 + lane] : 0ull;
        if (inl) {
#pragma unroll
            for (int q = 0; q < kEmitIn / 1024; q++) u[q] = 16 * (q * 64 + lane) < n ? ld16_in(p + 16 * (q * 64 + lane), lo, hi) : V16{0, 0};
        }
#pragma unroll
        for (int q = 0; q < kEmitStage / 64; q++) stage[q * 64 + lane] = t[q];
        if (inl) {
            typedef uint64_t __attribute__((aligned(8))) u64a8;
#pragma unroll
            for (int q = 0; q < kEmitIn / 1024; q++) {
                *(u64a8 *)(sin + 16 * (q * 64 + lane)) = u[q].lo;
                *(u64a8 *)(sin + 16 * (q * 64 + lane) + 8) = u[q].hi;
            }
        }
    }
    for (int32_t b0 = 0; b0 < m && !full; b0 += 64) {
        const int32_t k = b0 + lane;
        const bool here = k < m;
        int32_t lit_end, clen, dist;
        bool forced;
        if (WIDE) {
            const uint4 r4 = here ? ((const uint4 *)recs)[s * rcap + (uint64_t)k] : make_uint4(0, 0, 0, 0);
            lit_end = (int32_t)r4.x;
            clen = (int32_t)r4.y;
            dist = (int32_t)r4.z;
            forced = (r4.w & 1) != 0;
        } else {
            const uint64_t r = here ? (staged ? stage[k] : rec[k]) : 0ull;
            lit_end = (int32_t)(r & 0xfffff);
            clen = (int32_t)((r >> 20) & 0xfffff);
            dist = (int32_t)((r >> 40) & 0xfffff);
            forced = (r >> 60) != 0;
        }
        const int32_t end = lit_end + clen;
        const int32_t dk = wshr1(end, done);  // the previous record's end (lane 0: done)
        const int32_t L = lit_end - dk;
        const bool lit = here && (forced || L > 0);
        int32_t ln = 0, tn = 0, on = 0;
        const uint64_t lb = tag_bytes(0x00, L, &ln);
        if (!lit) ln = 0;
        uint64_t tb = tag_bytes(0x80, clen, &tn);
        uint64_t ob = off_bytes(dist, clen, &on);
        if (clen == 0) {  // a Write's end: its trailing literal only (writer.go:324-329)
            tb = ob = 0;
            tn = on = 0;
        }
        const int32_t T = here ? ln + (lit ? L : 0) + tn + on : 0;
        // inclusive prefix sum of T over the wave (DPP)
        const int32_t incl = wscan_add(T);
        const int32_t tok = op + incl - T;  // this token's output position
        const bool fits = here && tok + T <= cap;
        const uint64_t nofit = __ballot(here && !fits);
        const int lastok = nofit ? __builtin_ctzll(nofit) - 1 : 63;  // last lane whose token is written
        const bool wr = fits && lane <= lastok;
        bool longlit = false;
        if (wr) {
            uint8_t *d = out + tok;
            if (ln) put_small(d, V16{lb, 0}, (uint32_t)ln);
            if (lit) {
                if (L >= kLongLit) longlit = true;
                else if (inl) copy_lane_lds(d + ln, sin + dk, L);
                else copy_lane(d + ln, p + dk, L, lo, hi);
            }
            if (tn) {
                const uint64_t c0 = tb | (ob << (8 * tn));
                const uint64_t c1 = ob >> (64 - 8 * tn);
                put_small(d + T - tn - on, V16{c0, c1}, (uint32_t)(tn + on));
            }
        }
        // long literals: the whole wave, one at a time
        for (uint64_t lm = __ballot(longlit); lm; lm &= lm - 1) {
            const int src = __builtin_ctzll(lm);
            const int32_t Ls = rl32(L, src), ds = rl32(dk, src), ts = rl32(tok, src) + rl32(ln, src);
            for (int32_t q = 16 * lane; q < Ls; q += 16 * 64) {
                const V16 v = ld16_in(p + ds + q, lo, hi);
                if (q + 16 <= Ls) st16v(out + ts + q, v);
                else put_small(out + ts + q, v, (uint32_t)(Ls - q));
            }
        }
        if (nofit) {
            full = true;
            err = err ? err : EZ_ENOSPC;
            op = rl32(tok, lastok + 1);
        } else {
            op = rl32(op + incl, 63);
            done = rl32(end, m - b0 >= 64 ? 63 : m - b0 - 1);
        }
    }
    // trailing literal (writer.go:324-329)
    if (!full && !err && done < n) {
        const int32_t L = n - done;
        int32_t ln = 0;
        const uint64_t lb = tag_bytes(0x00, L, &ln);
        if (op + ln + L > cap) {
            err = EZ_ENOSPC;
        } else {
            if (lane == 0) put_small(out + op, V16{lb, 0}, (uint32_t)ln);
            const int32_t ts = op + ln;
            for (int32_t q = 16 * lane; q < L; q += 16 * 64) {
                const V16 v = ld16_in(p + done + q, lo, hi);
                if (q + 16 <= L) st16v(out + ts + q, v);
                else put_small(out + ts + q, v, (uint32_t)(L - q));
            }
            op += ln + L;
        }
    }
    if (lane == 0) {
        A.out_size[s] = (uint64_t)op;
        if (A.status) A.status[s] = err;
    }
}

}  // namespace k1
}  // namespace ez
