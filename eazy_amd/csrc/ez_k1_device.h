// ez_k1_device.h — what more than one K1 kernel family uses (ez_k1_parse.hip, ez_k1_lean.hip,
// ez_k1_long.hip, ez_k1_chunk.hip, ez_k1_emit.hip, ez_k1_probe.hip): the match records and their
// slots, the cooperative exact extension of a capped count, the branch-free byte counts, the
// one-atomic table visit, k1_lean's edge area (the routing sizes the scratch with it) and the
// diagnostic builds' cycle marks.  Everything here is inlined into its callers: device functions
// cannot cross a translation unit.
#pragma once

#include "ez_format.h"
#include "ez_internal.h"
#include "ez_wave.h"
#include "ez_k1_common.h"

// diagnostic builds only (make exp X=<bits>), each bit observes live kernels: 4 = cycle profile of
// the parse loops (k1_parse, long_loop), 65536 = k1_lean's acceptor histogram and K1c's read
// diagnosis, 2097152 = k1_lean's wave timeline
#ifndef EZ_EXP
#define EZ_EXP 0
#endif

#if (EZ_EXP & 4)
#define EZ_PROF_MARK(k)                                   \
    do {                                                  \
        __builtin_amdgcn_s_waitcnt(0);                    \
        const uint64_t t_ = __builtin_amdgcn_s_memtime(); \
        prof[k] += t_ - prof_t;                           \
        prof_t = t_;                                      \
    } while (0)
#else
#define EZ_PROF_MARK(k) do {} while (0)
#endif

namespace ez {
namespace k1 {

// a match record, 8 bytes: lit_end | copy length << 20 | distance << 40 | force << 60
// (positions < 2^20: streams <= kMaxT32); force: the literal is emitted even when
// empty (writeRunlen :480)
__host__ __device__ __forceinline__ constexpr uint64_t rec_pack(int32_t lit_end, int32_t clen, int32_t dist, bool force) {
    return (uint64_t)(uint32_t)lit_end | ((uint64_t)(uint32_t)clen << 20) | ((uint64_t)(uint32_t)dist << 40) | ((uint64_t)force << 60);
}
// the same record as its two dwords (k1_lean's windows build it this way: no 64-bit shift or or):
// lo = lit_end | clen << 20 (the length's low 12 bits), hi = clen >> 12 | dist << 8 | force << 28
struct Rec32 {
    uint32_t lo, hi;
};
__host__ __device__ constexpr Rec32 rec_pack32(int32_t lit_end, int32_t clen, int32_t dist, bool force) {
    return Rec32{(uint32_t)lit_end | ((uint32_t)clen << 20), ((uint32_t)clen >> 12) | ((uint32_t)dist << 8) | ((uint32_t)force << 28)};
}
constexpr bool rec_pack32_same(int32_t lit_end, int32_t clen, int32_t dist, bool force) {
    const Rec32 r = rec_pack32(lit_end, clen, dist, force);
    return (((uint64_t)r.hi << 32) | r.lo) == rec_pack(lit_end, clen, dist, force);
}
// every field at its ends and across the dword seam (bit 12 of the length), positions < 2^20
static_assert(rec_pack32_same(0, 0, 0, false) && rec_pack32_same((1 << 20) - 1, (1 << 20) - 1, (1 << 20) - 1, true) &&
                  rec_pack32_same(0, 4095, 1, false) && rec_pack32_same(1, 4096, 0, true) && rec_pack32_same(64, 4097, 4096, false) &&
                  rec_pack32_same(12345, 65472, 32768, true) && rec_pack32_same((1 << 20) - 1, 0, 0, false) &&
                  rec_pack32_same(0, (1 << 20) - 1, 0, false) && rec_pack32_same(0, 0, (1 << 20) - 1, false) && rec_pack32_same(0, 0, 0, true),
              "rec_pack32 is rec_pack's two halves");
constexpr int64_t kMaxT16 = 65536;  // T16 positions fit 16 bits (a stream's visited positions are < n - 3)
constexpr int64_t kMaxT32 = 1 << 19; // the judgement packs the candidate into 20 bits (and 2n <= block)

// record slot of stream s: s * rec_cap .. ; every match advances done by >= 6,
// and every Write but the last ends with a marker record
__host__ __device__ __forceinline__ uint64_t rec_cap(const CompressArgs &a) {
    return a.max_len / 6 + 1 + (a.write_idx ? a.max_writes : 0);
}

// bytes [0, k) of v kept, the rest 0 (k <= 0: none, k >= 16: all)
__device__ __forceinline__ V16 keep_low16(V16 v, int32_t k) {
    const uint64_t ml = k >= 8 ? ~0ull : (k <= 0 ? 0ull : (1ull << (8 * k)) - 1);
    const uint64_t mh = k >= 16 ? ~0ull : (k <= 8 ? 0ull : (1ull << (8 * (k - 8))) - 1);
    return V16{v.lo & ml, v.hi & mh};
}

// 16 bytes from y of the match's source side: mode 0 zeros (zero region),
// 1 the stream itself (run length), 2 the ring image of a fresh window
// (bytes before the stream start and from `done` on read 0)
template <class SRC>
__device__ __forceinline__ V16 src16(const SRC &P, int32_t y, int mode, int32_t done) {
    if (mode == 0) return V16{0, 0};
    uint64_t lo, hi;
    P.around(y + 8, lo, hi);  // bytes y .. y+15, zeros before the stream start
    const V16 v{lo, hi};
    return mode == 2 ? keep_low16(v, done - y) : v;
}

// Exact forward and backward match counts of one group at once, past the
// bytes the capped judgement already compared (fromf forward, 8 backward):
// lanes 0..G/2-1 scan forward
// (a+k vs b+k), lanes G/2..G-1 backward (a-1-k vs b-1-k), 16 bytes per lane
// per step, so a count below fromf + 8G bytes costs one load round trip.
template <int G, class SRC>
__device__ __forceinline__ void gext(const SRC &P, bool runf, bool runb, int g, int lj, int32_t a, int32_t b, int mode,
                                     int32_t done, int32_t fromf, int32_t limf, int32_t limb, int32_t &resf, int32_t &resb) {
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
                const V16 vb = src16(P, yb, mode, done);
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

// Aligned loads of stream bytes in the global address space (k1_lean's windows and candidates,
// K1L's candidates inside the batch): plain global_load instructions, not flat ones, which would
// also count against the LDS counter and wait on the ds_bpermute traffic
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) uint32_t *gu32p;
typedef const __attribute__((address_space(1))) u32x4 *gu128p;
struct LeanIn {
    __device__ __forceinline__ uint32_t dw(const uint8_t *w) const { return *(gu32p)w; }
    __device__ __forceinline__ uint4 dw4(const uint8_t *w) const {
        const u32x4 v = *(gu128p)w;
        return make_uint4(v.x, v.y, v.z, v.w);
    }
};

// a group's window buffer in LDS (WinLds, WinLdsL): a 128-byte region and the reads' overhang
constexpr int32_t kWinLdsBytes = 144;

// Byte counts without branches: v_ffbl / v_ffbh return ~0u for 0, and saturating adds keep that
// "no bit here" through the word offsets, so a min over the words finds the first set bit.
__device__ __forceinline__ uint32_t ffbl32(uint32_t x) {
    uint32_t r;
    asm("v_ffbl_b32 %0, %1" : "=v"(r) : "v"(x));
    return r;
}
__device__ __forceinline__ uint32_t ffbh32(uint32_t x) {
    uint32_t r;
    asm("v_ffbh_u32 %0, %1" : "=v"(r) : "v"(x));
    return r;
}
__device__ __forceinline__ uint32_t sat_add(uint32_t a, uint32_t b) { return __builtin_elementwise_add_sat(a, b); }
// equal leading (low-address) bytes of the 24 bytes whose xor is (e0, e1, e2): 0 .. 24
__device__ __forceinline__ int32_t first_diff24(uint64_t e0, uint64_t e1, uint64_t e2) {
    uint32_t m = ffbl32((uint32_t)e0);
    m = min(m, sat_add(ffbl32((uint32_t)(e0 >> 32)), 32u));
    m = min(m, sat_add(ffbl32((uint32_t)e1), 64u));
    m = min(m, sat_add(ffbl32((uint32_t)(e1 >> 32)), 96u));
    m = min(m, sat_add(ffbl32((uint32_t)e2), 128u));
    m = min(m, sat_add(ffbl32((uint32_t)(e2 >> 32)), 160u));
    return (int32_t)min(m >> 3, 24u);
}
// the same over 40 bytes: 0 .. 40
__device__ __forceinline__ int32_t first_diff40(uint64_t e0, uint64_t e1, uint64_t e2, uint64_t e3, uint64_t e4) {
    uint32_t m = ffbl32((uint32_t)e0);
    m = min(m, sat_add(ffbl32((uint32_t)(e0 >> 32)), 32u));
    m = min(m, sat_add(ffbl32((uint32_t)e1), 64u));
    m = min(m, sat_add(ffbl32((uint32_t)(e1 >> 32)), 96u));
    m = min(m, sat_add(ffbl32((uint32_t)e2), 128u));
    m = min(m, sat_add(ffbl32((uint32_t)(e2 >> 32)), 160u));
    m = min(m, sat_add(ffbl32((uint32_t)e3), 192u));
    m = min(m, sat_add(ffbl32((uint32_t)(e3 >> 32)), 224u));
    m = min(m, sat_add(ffbl32((uint32_t)e4), 256u));
    m = min(m, sat_add(ffbl32((uint32_t)(e4 >> 32)), 288u));
    return (int32_t)min(m >> 3, 40u);
}
// equal trailing (high-address) bytes of the 8 bytes whose xor is e: 0 .. 8
__device__ __forceinline__ int32_t last_diff8(uint64_t e) {
    const uint32_t m = min(ffbh32((uint32_t)(e >> 32)), sat_add(ffbh32((uint32_t)e), 32u));
    return (int32_t)min(m >> 3, 8u);
}

// Visit by one LDS atomic (MSK): ds_mskor_rtn_b32 sets the lane's u16 table entry to its position
// and returns the word as it was -- lanes of one wave instruction that hit the same word apply in
// ascending lane order (probed once per process, k_lds_mskor_order), so a lane reads the position
// of the nearest earlier lane of its window with the same hash, or the table's entry when there is
// none: the table read, the 15-step DPP predecessor search and the visited lanes' table store in
// one instruction.  Lanes after the window's acceptor, which Go never visits, then put back what
// they found unless it is a position of another such lane (only the first of a hash past the
// acceptor restores; its value is the one Go's table holds).  (The wait is in the asm: the
// compiler does not count an asm's LDS operation.)
__device__ __forceinline__ uint32_t lds_mskor16(uint16_t *hth, uint32_t h, uint32_t val) {
    const uint32_t sh = (h & 1u) << 4;
    const uint32_t addr = (uint32_t)(uintptr_t)((__attribute__((address_space(3))) uint8_t *)hth) + ((h >> 1) << 2);
    uint32_t r;
    asm volatile("ds_mskor_rtn_b32 %0, %1, %2, %3\n\ts_waitcnt lgkmcnt(0)" : "=v"(r) : "v"(addr), "v"(0xffffu << sh), "v"(val << sh) : "memory");
    return (r >> sh) & 0xffffu;
}

// k1_lean's edge area, after the records in the K1s scratch (ez_k1_lean.hip describes its use;
// split_scratch_words sizes the scratch with it)
constexpr int kEdgeSlots = 40;
constexpr int32_t kEdgeBefore = 64;  // readable bytes before a stream (WinLds's regions), 64 after it
__host__ __device__ __forceinline__ uint64_t edge_slot_bytes(const CompressArgs &a) { return (a.max_len + kEdgeBefore + 64 + 15) & ~15ull; }
__host__ __device__ __forceinline__ uint64_t edge_area_bytes(const CompressArgs &a) { return 128 + kEdgeSlots * edge_slot_bytes(a) + 16; }

// K1L's and K1c's 16-byte records (k1_emit<true>, ke_* read them)
struct WideRec {
    uint32_t lit_end, clen, dist, flags;  // flags bit 0: force the literal (writeRunlen, A.6)
};

typedef uint64_t __attribute__((aligned(1))) u64_ua;
typedef uint32_t __attribute__((aligned(1))) u32_ua;

}  // namespace k1
}  // namespace ez
