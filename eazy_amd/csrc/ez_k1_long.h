// ez_k1_long.h — K1L's parse loop (long_loop) with its windows, sources and exact extension:
// k1_long and k1_long_ring run it (ez_k1_long.hip), and K1c's kc_parse runs it on chunks with its
// visit log (ez_k1_chunk.hip), so it lives in a header.
//
// K1L: long fresh streams.  k1_lean's parse for Writes longer than half the block (C4's gradient buckets, where K1x's rounds
// leave dense streams such as C4s to it): the same window, DPP predecessor search and capped
// judgement, plus the window's ring semantics of writer.go -- far skip (:219-221), the cut branch of
// writeRunlen (:464-473), trim 1 (:280-286) and the ring image before the window, block[y & mask] =
// stream byte y + bs for y < w.pos - bs -- a u32 table, bounds-checked loads (any
// stream of a batch, no edge slots), and 16-byte records.  It resumes the streams K1x hands over
// (spec state: position, pending literal, output so far, table).
#pragma once

#include "ez_k1_device.h"

#include <cstdio>
#include <type_traits>

namespace ez {
namespace k1 {

// distance to the nearest earlier lane of the 16-lane row with the same hash (0: none), by DPP row
// shifts on hashes offset to be nonzero, with bound_ctrl (a lane K below outside the row reads 0,
// which never equals): no v_mov of a row-edge default per step.  Each step is still
// v_mov_dpp + v_cmp + v_cndmask: gfx950 has no DPP form of the VOPC compares.
template <int K>
struct PredZ {
    __device__ __forceinline__ static int32_t get(uint32_t hp, int32_t d) {
        const uint32_t hk = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)hp, 0x110 + K, 0xf, 0xf, true);
        d = hk == hp ? K : d;  // descending K: the nearest one stays
        return PredZ<K - 1>::get(hp, d);
    }
};
template <>
struct PredZ<0> {
    __device__ __forceinline__ static int32_t get(uint32_t, int32_t d) { return d; }
};

// a dword at w, 0 for bytes outside the batch [lo, hi)
__device__ __forceinline__ uint32_t dw_chk(const uint8_t *w, const uint8_t *lo, const uint8_t *hi) {
    if (w >= lo && w + 4 <= hi) return *(const uint32_t *)w;
    uint32_t v = 0;
    for (int t = 0; t < 4; t++)
        if (w + t >= lo && w + t < hi) v |= (uint32_t)w[t] << (8 * t);
    return v;
}
// K1L's window bytes (x-8 .. x+39 of each lane's x) from a 128-byte region held across windows in
// the lanes' registers, with the next one in flight (k1_lean's WinLds scheme with bounds-checked
// loads: any stream of any batch).  Lane k of the group holds dwords 2k and 2k+1 of the region
// [p + cb, p + cb + 128), and a lane assembles its window with ds_bpermute, selects and
// v_alignbyte.  k1_long_ring<false> (a handle's Write too long for LDS staging) parses with it;
// k1_long and kc_parse keep the region in LDS (WinLdsL)
struct WinRollL {
    uint32_t c0, c1, f0, f1;  // this lane's dwords 2k, 2k+1 of the current and the prefetched region
    int32_t cb, fb, pm;       // region starts relative to p (4-byte aligned addresses); p & 3
    __device__ __forceinline__ int32_t floor4(int32_t y) const { return y - ((pm + y) & 3); }
    __device__ __forceinline__ static void ld(const uint8_t *p, int32_t b, int lj, const uint8_t *lo, const uint8_t *hi,
                                              uint32_t &d0, uint32_t &d1) {
        const uint8_t *a = p + b + 8 * lj;
        if (a >= lo && a + 8 <= hi) {
            typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
            typedef const __attribute__((address_space(1))) u32x2 *gu64p;
            const u32x2 v = *(gu64p)a;
            d0 = v.x;
            d1 = v.y;
        } else {
            d0 = dw_chk(a, lo, hi);
            d1 = dw_chk(a + 4, lo, hi);
        }
    }
    // (c only ever from these moves after f's load: no load is pending on c's registers at the loop's
    // head, where a wait for one would wait for the prefetch behind it too)
    __device__ __forceinline__ void init(const uint8_t *p, int32_t i, int lj, bool live, const uint8_t *lo, const uint8_t *hi) {
        pm = (int32_t)((uintptr_t)p & 3);
        cb = floor4(i - 8);
        fb = cb + 64;
        f0 = f1 = 0;
        if (live) ld(p, cb, lj, lo, hi, f0, f1);
        asm volatile("v_mov_b32 %0, %1" : "=v"(c0) : "v"(f0));
        asm volatile("v_mov_b32 %0, %1" : "=v"(c1) : "v"(f1));
        if (live) ld(p, fb, lj, lo, hi, f0, f1);
    }
    // the region for the window at i (group-uniform: 0 <= i - 8 - cb <= 64), after this window's gathers
    __device__ __forceinline__ void advance(const uint8_t *p, int32_t i, int lj, bool live, const uint8_t *lo, const uint8_t *hi) {
        const int32_t y = i - 8;
        if (live && !(y >= cb && y - cb <= 64)) {
            if (!(y >= fb && y - fb <= 64)) {  // a long jump (or back: the cut branch): loaded on the chain
                fb = floor4(y);
                ld(p, fb, lj, lo, hi, f0, f1);
            }
            cb = fb;
            asm volatile("v_mov_b32 %0, %1" : "=v"(c0) : "v"(f0));
            asm volatile("v_mov_b32 %0, %1" : "=v"(c1) : "v"(f1));
            fb = cb + 64;
            ld(p, fb, lj, lo, hi, f0, f1);
        }
    }
    __device__ __forceinline__ void bytes48(int32_t i, int g, int lj, V16 &w0, V16 &w1, V16 &w2) const {
        const uint32_t o = (uint32_t)(i - 8 - cb + lj), q = o >> 2, r = o & 3;  // o <= 79: q >> 1 <= 9
        const int src = 4 * (16 * g + (int)(q >> 1));
        uint32_t e[14];
#pragma unroll
        for (int t = 0; t < 7; t++) {
            e[2 * t] = (uint32_t)__builtin_amdgcn_ds_bpermute(src + 4 * t, (int)c0);
            e[2 * t + 1] = (uint32_t)__builtin_amdgcn_ds_bpermute(src + 4 * t, (int)c1);
        }
        const uint32_t m = 0u - (q & 1);
        uint32_t d[13];
#pragma unroll
        for (int t = 0; t < 13; t++) d[t] = (e[t + 1] & m) | (e[t] & ~m);
        uint32_t b[12];
#pragma unroll
        for (int t = 0; t < 12; t++) b[t] = __builtin_amdgcn_alignbyte(d[t + 1], d[t], r);
        w0 = V16{(uint64_t)b[0] | ((uint64_t)b[1] << 32), (uint64_t)b[2] | ((uint64_t)b[3] << 32)};
        w1 = V16{(uint64_t)b[4] | ((uint64_t)b[5] << 32), (uint64_t)b[6] | ((uint64_t)b[7] << 32)};
        w2 = V16{(uint64_t)b[8] | ((uint64_t)b[9] << 32), (uint64_t)b[10] | ((uint64_t)b[11] << 32)};
    }
};
// WinRollL with the current region in LDS (as WinLds): the group's buffer holds stream bytes
// [cb, cb + 128); a window's 48 bytes are thirteen aligned dword reads and twelve v_alignbyte
struct WinLdsL {
    uint32_t f0, f1;  // this lane's dwords of the prefetched region
    int32_t cb, fb, pm;
    uint8_t *wl;  // the group's buffer (LDS)
    __device__ __forceinline__ int32_t floor4(int32_t y) const { return y - ((pm + y) & 3); }
    __device__ __forceinline__ void put(int lj) const { *(uint64_t *)(wl + 8 * lj) = (uint64_t)f0 | ((uint64_t)f1 << 32); }
    __device__ __forceinline__ void init(const uint8_t *p, int32_t i, int lj, bool live, const uint8_t *lo, const uint8_t *hi) {
        pm = (int32_t)((uintptr_t)p & 3);
        cb = floor4(i - 8);
        fb = cb + 64;
        f0 = f1 = 0;
        if (live) WinRollL::ld(p, cb, lj, lo, hi, f0, f1);
        put(lj);
        if (live) WinRollL::ld(p, fb, lj, lo, hi, f0, f1);
    }
    __device__ __forceinline__ void advance(const uint8_t *p, int32_t i, int lj, bool live, const uint8_t *lo, const uint8_t *hi) {
        const int32_t y = i - 8;
        if (live && !(y >= cb && y - cb <= 64)) {
            if (!(y >= fb && y - fb <= 64)) {  // a long jump (or back: the cut branch): loaded on the chain
                fb = floor4(y);
                WinRollL::ld(p, fb, lj, lo, hi, f0, f1);
            }
            cb = fb;
            put(lj);
            fb = cb + 64;
            WinRollL::ld(p, fb, lj, lo, hi, f0, f1);
        }
    }
    __device__ __forceinline__ void bytes48(int32_t i, int g, int lj, V16 &w0, V16 &w1, V16 &w2) const {
        const uint32_t o = (uint32_t)(i - 8 - cb + lj), r = o & 3;  // o <= 79
        const uint32_t *q = (const uint32_t *)(wl + (o & ~3u));
        uint32_t d[13];
#pragma unroll
        for (int t = 0; t < 13; t++) d[t] = q[t];
        uint32_t b[12];
#pragma unroll
        for (int t = 0; t < 12; t++) b[t] = __builtin_amdgcn_alignbyte(d[t + 1], d[t], r);
        w0 = V16{(uint64_t)b[0] | ((uint64_t)b[1] << 32), (uint64_t)b[2] | ((uint64_t)b[3] << 32)};
        w1 = V16{(uint64_t)b[4] | ((uint64_t)b[5] << 32), (uint64_t)b[6] | ((uint64_t)b[7] << 32)};
        w2 = V16{(uint64_t)b[8] | ((uint64_t)b[9] << 32), (uint64_t)b[10] | ((uint64_t)b[11] << 32)};
    }
};
// bytes y-8 .. y+39 (bytes outside the batch read 0)
__device__ __forceinline__ void bytes48_chk(const uint8_t *p, int32_t y, V16 &c0, V16 &c1, V16 &c2, const uint8_t *lo,
                                            const uint8_t *hi) {
    const uintptr_t a = (uintptr_t)(p + y - 8);
    const uint8_t *w = (const uint8_t *)(a & ~(uintptr_t)3);
    const uint32_t r = (uint32_t)(a & 3);
    uint32_t d[13];
    if (w >= lo && w + 52 <= hi) {
        const LeanIn L;
        const uint4 q0 = L.dw4(w), q1 = L.dw4(w + 16), q2 = L.dw4(w + 32);
        const uint32_t q3 = L.dw(w + 48);
        d[0] = q0.x, d[1] = q0.y, d[2] = q0.z, d[3] = q0.w, d[4] = q1.x, d[5] = q1.y, d[6] = q1.z, d[7] = q1.w;
        d[8] = q2.x, d[9] = q2.y, d[10] = q2.z, d[11] = q2.w, d[12] = q3;
    } else {
        for (int t = 0; t < 13; t++) d[t] = dw_chk(w + 4 * t, lo, hi);
    }
    uint32_t b[12];
#pragma unroll
    for (int t = 0; t < 12; t++) b[t] = __builtin_amdgcn_alignbyte(d[t + 1], d[t], r);
    c0 = V16{(uint64_t)b[0] | ((uint64_t)b[1] << 32), (uint64_t)b[2] | ((uint64_t)b[3] << 32)};
    c1 = V16{(uint64_t)b[4] | ((uint64_t)b[5] << 32), (uint64_t)b[6] | ((uint64_t)b[7] << 32)};
    c2 = V16{(uint64_t)b[8] | ((uint64_t)b[9] << 32), (uint64_t)b[10] | ((uint64_t)b[11] << 32)};
}
// 16 bytes from y of the window's ring image at w.pos = done (bytes y >= done: 0, capped away by
// trim 2; y < done - bs: stream byte y + bs; before the stream: 0)
template <class SRC>
__device__ __forceinline__ V16 ring16(const SRC &P, int32_t y, int32_t done, int64_t bs) {
    uint64_t lo, hi;
    P.around(y + 8, lo, hi);
    V16 v = keep_low16(V16{lo, hi}, done - y);
    const int64_t edge = (int64_t)done - bs;
    if ((int64_t)y < edge) {
        P.around((int32_t)((int64_t)y + bs + 8), lo, hi);
        const int32_t k = (int32_t)(edge - y);  // bytes 0 .. k-1 lie before the window
        const V16 m = keep_low16(V16{~0ull, ~0ull}, k);
        v = V16{(v.lo & ~m.lo) | (lo & m.lo), (v.hi & ~m.hi) | (hi & m.hi)};
    }
    return v;
}
// gext with the long window's ring image on the source side (mode 2: ring16; 0 zeros; 1 stream)
template <int G, class SRC>
__device__ __forceinline__ void gext_long(const SRC &P, bool runf, bool runb, int g, int lj, int32_t a, int32_t b, int mode,
                                          int32_t done, int64_t bs, int32_t fromf, int32_t limf, int32_t limb, int32_t &resf,
                                          int32_t &resb) {
    constexpr int H = G / 2;
    constexpr uint32_t kHalf = (1u << H) - 1;
    const bool fw = lj < H;
    const int t = lj % H;
    resf = fromf < limf ? fromf : limf;
    resb = 8 < limb ? 8 : limb;
    bool gof = runf && fromf < limf, gob = runb && 8 < limb;
    int32_t basef = fromf, baseb = 8;
    while (__ballot(gof || gob) != 0) {
        const bool mine = fw ? gof : gob;
        const int32_t lim = fw ? limf : limb;
        const int32_t k = (fw ? basef : baseb) + 16 * t;
        int32_t mb = 16;
        if (mine) {
            if (k < lim) {
                const int32_t ya = fw ? a + k : a - k - 16, yb = fw ? b + k : b - k - 16;
                uint64_t alo, ahi;
                P.around(ya + 8, alo, ahi);
                V16 vb{0, 0};
                if (mode == 1) P.around(yb + 8, vb.lo, vb.hi);
                else if (mode == 2) vb = ring16(P, yb, done, bs);
                const uint64_t dl = alo ^ vb.lo, dh = ahi ^ vb.hi;
                if (fw) mb = dl ? (int32_t)(__builtin_ctzll(dl) >> 3) : (dh ? 8 + (int32_t)(__builtin_ctzll(dh) >> 3) : 16);
                else mb = dh ? (int32_t)(__builtin_clzll(dh) >> 3) : (dl ? 8 + (int32_t)(__builtin_clzll(dl) >> 3) : 16);
                if (mb > lim - k) mb = lim - k;
            } else {
                mb = 0;
            }
        }
        const uint32_t bad = gball<G>(mine && mb < 16, g);
        const uint32_t bf = bad & kHalf, bb = bad >> H;
        const int lf = bf ? __builtin_ctz(bf) : 0, lb = bb ? __builtin_ctz(bb) : 0;
        const int32_t mbf = bcast(mb, G * g + lf), mbb = bcast(mb, G * g + H + lb);
        if (gof) {
            if (bf) {
                resf = basef + 16 * lf + mbf;
                resf = resf < limf ? resf : limf;
                gof = false;
            } else {
                basef += 16 * H;
                if (basef >= limf) { resf = limf; gof = false; }
            }
        }
        if (gob) {
            if (bb) {
                resb = baseb + 16 * lb + mbb;
                resb = resb < limb ? resb : limb;
                gob = false;
            } else {
                baseb += 16 * H;
                if (baseb >= limb) { resb = limb; gob = false; }
            }
        }
    }
}

// The history a window match compares against, as a linear byte view (positions relative to the
// parse's p; ring16 turns it into the ring image).  FreshSrc: a fresh Writer, nothing before p (the
// zero ring).  RingSrc (ez_k1_long.hip): a Writer handle's Write at stream position start: the bytes
// before p are the handle's ring as the Write found it (block[(start + y) & mask]; zeros
// where the stream has not reached yet), p's own from 0 on.
struct FreshSrc : GW {
    __device__ __forceinline__ void bytes48(int32_t cand, V16 &c0, V16 &c1, V16 &c2) const {
        bytes48_chk(p, cand, c0, c1, c2, blo, bhi);
        c0.lo &= cand >= 8 ? ~0ull : (cand <= 0 ? 0ull : ~0ull << (8 * (8 - cand)));  // before the stream: zeros
    }
};
// a source that also serves the window's bytes (window48) specialises this to true (LdsSrc)
template <class SRC>
struct WindowFromSrc {
    static constexpr bool value = false;
};

// the parse of one stream by a 16-lane group from (i, done) with the table in htw; LW: the
// window's region in LDS at wl (WinLdsL), else in the lanes' registers (WinRollL).  The capped
// judgement compares 40 bytes forward (k1_lean: 24): the long parse is a latency chain (few streams
// per SIMD), and at C2 one accepted copy in nine is 24 - 39 bytes long, whose exact extension
// (gext_long) is a group-wide round trip that every stream of the wave waits for.
constexpr int32_t kLCap = 40;
// K1c's side outputs of a chunk's speculative parse (see kc_parse); NoEv: none (K1L)
struct NoEv {
    static constexpr bool kOn = false;
    int32_t stop, keep;
    uint32_t cnt;
    __device__ __forceinline__ void visit(int32_t, int32_t, bool, bool, int, int, int32_t, bool, int32_t) {}
};
template <class SRC, bool LW = false, class EV = NoEv>
__device__ __forceinline__ void long_loop(const SRC &P, const uint8_t *p, int32_t n, int32_t i, int32_t done, int64_t bs, int lj,
                                          int g, uint32_t *htw, uint32_t hsh, uint4 *rec, uint64_t rcap, const uint8_t *blo,
                                          const uint8_t *bhi, int32_t &nrec_out, int &err, uint8_t *wl = nullptr, EV *ev = nullptr) {
    constexpr int G = 16;
    int32_t nrec = 0;
    bool live = !err && i + 4 <= n && (!EV::kOn || i < ev->stop);
    int64_t guard = 4 * (int64_t)n + 64;
    V16 w0{0, 0}, w1{0, 0}, w2{0, 0};  // bytes x-8 .. x+7, x+8 .. x+23, x+24 .. x+39 of this lane's position x
    typename std::conditional<LW, WinLdsL, WinRollL>::type wr;
    if constexpr (LW) wr.wl = wl;
    if (!WindowFromSrc<SRC>::value) wr.init(p, i, lj, live, blo, bhi);
    constexpr bool kWinSrc = WindowFromSrc<SRC>::value;
#if (EZ_EXP & 4)
    uint64_t prof[8] = {0, 0, 0, 0, 0, 0, 0, 0}, prof_t = __builtin_amdgcn_s_memtime(), prof_it = 0, prof_acc = 0, prof_ef = 0, prof_eb = 0;
#endif
    while (__ballot(live) != 0) {
#if (EZ_EXP & 4)
        prof_it++;
#endif
        if constexpr (kWinSrc) {
            P.window48(live ? i + lj : 0, w0, w1, w2);
        } else {
            wr.bytes48(i, g, lj, w0, w1, w2);
        }
        EZ_PROF_MARK(0);
        if (live && --guard < 0) { err = EZ_ESTUCK; live = false; }
        const int32_t nvalid = n - 3 - i < G ? n - 3 - i : G;
        const int32_t x = i + lj;
        const bool valid = live && lj < nvalid;

        // ---- visit (writer.go:213-217): hash, table, nearest earlier lane with the same hash
        const uint32_t h = valid ? ((uint32_t)w0.hi * kHashMul) >> hsh : 0u;
        const int32_t tv = valid ? (int32_t)htw[h] : 0;
        const int32_t d = PredZ<G - 1>::get(valid ? h + 1 : 0u, 0);
        const int32_t cand = valid ? (d ? x - d : tv) : 0;
        const bool rl = cand >= done && cand < x;
        const bool far = !rl && (int64_t)done - cand > bs;  // writer.go:221-224
        EZ_PROF_MARK(1);
        V16 c0{0, 0}, c1{0, 0}, c2{0, 0};
        if (valid && !far) {
            P.bytes48(cand, c0, c1, c2);
            if (!rl && (int64_t)cand - 8 < (int64_t)done - bs) c0.lo = ring16(P, cand - 8, done, bs).lo;  // rare
        }
        EZ_PROF_MARK(2);

        // ---- capped judgement, writer.go:219-301 (window) and :441-473 (writeRunlen, cut)
        int32_t jf = first_diff40(w0.hi ^ c0.hi, w1.lo ^ c1.lo, w1.hi ^ c1.hi, w2.lo ^ c2.lo, w2.hi ^ c2.hi);
        jf = jf < n - x ? jf : n - x;
        int32_t bl = x - done;
        if (rl) bl = bl < cand ? bl : cand;
        int32_t jb = last_diff8(w0.lo ^ c0.lo);
        jb = jb < bl ? jb : bl;
        const bool zr = rl && c0.hi == 0 && cand + 8 < n;
        const int32_t fw = rl ? jf : (jf < done - cand ? jf : done - cand);
        const int64_t t1 = bs - (int64_t)(x - cand);  // trim 1: the copy ends within bs of x
        const int32_t len = rl ? fw + jb : (int32_t)((int64_t)(fw + jb) < t1 ? (int64_t)(fw + jb) : (t1 < 0 ? -1 : t1));
        const bool acc = valid && !far && (zr || len >= kMinCopyChunk);
        const bool cut = rl && !zr && (int64_t)(x - cand) >= bs - 8;

        // ---- this lane's action if it is the group's first acceptor
        int32_t lit, nx, dist, ext;
        bool force = false;
        if (zr) {  // writeZeros :407-439
            int32_t zf = first_diff40(0, c1.lo, c1.hi, c2.lo, c2.hi);
            zf = zf < n - cand ? zf : n - cand;
            int32_t zb = last_diff8(c0.lo);
            zb = zb < cand - done ? zb : cand - done;
            lit = cand - zb;
            nx = cand + zf;
            dist = 0;
            ext = (zf == kLCap && n - cand > kLCap ? 1 : 0) | (zb == 8 && cand - done > 8 ? 2 : 0);
        } else if (cut) {  // the cut branch: a literal to done + i - st, no copy (writer.go:464-473)
            lit = done + (x - cand);
            nx = lit;
            dist = 0;
            ext = 0;
        } else {  // writeRunlen :441-489 / window match :303-321
            lit = x - jb;
            nx = lit + len;
            dist = x - cand;
            force = rl;
            const int32_t room = rl ? n - x : (done - cand < n - x ? done - cand : n - x);
            ext = (jf == kLCap && room > kLCap && (rl || (int64_t)(jb + kLCap) < t1) ? 1 : 0) | (jb == 8 && bl > 8 ? 2 : 0);
        }
        const uint64_t am64 = __ballot(acc);
        const uint32_t am = (uint32_t)(am64 >> (G * g)) & 0xffffu;
        const int a = am ? __builtin_ctz(am) : -1;
        const bool act = live && a >= 0;
        const int al = G * g + (a < 0 ? 0 : a);
        int32_t nxt = bcast(nx, al);
        const int32_t ea = bcast(ext, al);
        EZ_PROF_MARK(3);
#if (EZ_EXP & 4)
        prof_acc += act ? 1 : 0;
        prof_ef += act && (ea & 1) ? 1 : 0;
        prof_eb += act && (ea & 2) ? 1 : 0;
#endif
        if (__ballot(act && ea != 0) != 0) {
            // rare: a saturated count; exact lengths by the whole group
            const int32_t xa = i + (a < 0 ? 0 : a);
            const int32_t ca = bcast(cand, al), jba = bcast(jb, al), fwa = bcast(zr ? nx - cand : fw, al);
            const int32_t fl = bcast((int32_t)rl | ((int32_t)zr << 1), al);
            const bool rla = fl & 1, zra = (fl >> 1) & 1;
            const bool need = act && ea != 0;
            const int mode = zra ? 0 : (rla ? 1 : 2);
            const int32_t fa = zra ? ca : xa;
            const int32_t blim = zra ? ca - done : (rla ? ((xa - done) < ca ? (xa - done) : ca) : xa - done);
            const int32_t flim = zra ? n - ca : (rla ? n - xa : ((done - ca) < n - xa ? done - ca : n - xa));
            int32_t fx, cx;
            gext_long<G, SRC>(P, need && (ea & 1), need && (ea & 2), g, lj, fa, ca, mode, done, bs, kLCap, flim, blim, fx, cx);
            if (need) {
                int32_t f = (ea & 1) ? fx : fwa;
                const int32_t c = (ea & 2) ? cx : (zra ? fa - bcast(lit, al) : jba);
                if (!zra && !rla) {  // trim 1 on the exact lengths
                    const int64_t t1a = bs - (int64_t)(xa - ca);
                    if ((int64_t)(f + c) > t1a) f = (int32_t)(t1a - c);
                }
                nxt = fa + f;
                if (lj == a) {
                    lit = fa - c;
                    nx = nxt;
                }
            }
        }
        EZ_PROF_MARK(4);
        // K1c: the window's visits (and the i+1 insert) into the chunk's log, in the parse's order
        bool keep = true;
        uint32_t logi = 0;
        if constexpr (EV::kOn) {
            const bool insb = bcast((int32_t)(act && lj == a && !rl && !zr && x + 1 + 4 <= n), al) != 0;
            ev->visit(x, cand, valid && (a < 0 || lj <= a), act && lj == a, g, lj, i, insb, i + (a < 0 ? 0 : a) + 1);
            logi = ev->cnt;
            keep = nxt >= ev->keep;
        }
        // ---- table: the visited lanes' positions (the last of a hash wins), then lane a's i+1
        if (valid && (a < 0 || lj <= a)) htw[h] = (uint32_t)x;
        if (act && lj == a) {
            if (!rl && !zr && x + 1 + 4 <= n) htw[((uint32_t)(w0.hi >> 8) * kHashMul) >> hsh] = (uint32_t)(x + 1);
        }
        // the record, stored after the next region's load is issued (as in lean_run)
        const bool st_rec = act && lj == a && keep && (uint64_t)nrec < rcap;
        // (K1c: the log's length after this window in the flags word's bits 1..31; k1_emit reads bit 0)
        const u32x4 recv{(uint32_t)lit, (uint32_t)(nx - lit), (uint32_t)dist, (force ? 1u : 0u) | (logi << 1)};
        u32x4 *const recp = (u32x4 *)(rec + nrec);
        if (act) {
            if (keep) {
                if ((uint64_t)nrec >= rcap) { err = EZ_ESTUCK; live = false; }
                nrec++;
            }
            i = done = nxt;
        } else if (live) {
            i += nvalid;
        }
        if (live && (err || i + 4 > n || (EV::kOn && i >= ev->stop))) live = false;
        if (!kWinSrc) wr.advance(p, i, lj, live, blo, bhi);  // the next window's region
        __builtin_amdgcn_sched_barrier(0);
        if (st_rec) __builtin_nontemporal_store(recv, recp);
        EZ_PROF_MARK(5);
    }
#if (EZ_EXP & 4)
    if (blockIdx.x < 8 && lj == 0)
        printf("lprof blk %u g %d it %llu acc %llu ef %llu eb %llu: window %llu visit %llu cload %llu judge %llu ext %llu upd %llu\n", blockIdx.x, g,
               (unsigned long long)prof_it, (unsigned long long)prof_acc, (unsigned long long)prof_ef, (unsigned long long)prof_eb, (unsigned long long)prof[0], (unsigned long long)prof[1],
               (unsigned long long)prof[2], (unsigned long long)prof[3], (unsigned long long)prof[4], (unsigned long long)prof[5]);
#endif
    nrec_out = nrec;
}

}  // namespace k1
}  // namespace ez
