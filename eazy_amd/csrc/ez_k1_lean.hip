// ez_k1_lean.hip — K1p, lean single-Write form: k1_lean and its launcher.
// The same parse as k1_parse<16, true, false> (one Write per fresh stream, u16 table,
// 16 or 8 lanes per stream, inputs through L1/L2) with a shorter per-window chain:
//  * loads need no bounds logic on waves whose streams all have 8 readable bytes before
//    and 48 after them inside the batch (every wave but the batch's first and last);
//  * the capped forward count compares real stream bytes and takes min(count, done - cand)
//    for window matches: below `done` the ring image is the stream, and trim 2
//    (writer.go:292-296) cuts any window match at w.pos = done, so the zeros the ring holds
//    from done on never reach a decision or a length;
//  * the accepting lane computes its own record and the group's next position; the other
//    lanes take that position with one v_readlane per group (no LDS round trip); the
//    extra insert of i+1 (writer.go:315-318) is the accepting lane's own second store, after
//    the visited lanes' one (LDS stores of one wave land in issue order), hashed from its
//    own bytes x+1 .. x+4;
//  * only counts at their cap (24 or 40 forward / 8 backward) take the cooperative extension
//    (gext), as a rare branch, which also finds whether the match has room past the cap;
//  * while every group of the wave is far enough from its stream's end, the window runs in an
//    interior form without end clamps, liveness terms and record-room test (lean_run).
// Loads of the lean parse carry no bounds logic: every stream the loop reads has 64 readable bytes
// before it and 64 after it (k1_lean copies the few streams at the batch's edges into padded
// slots first), so each piece is one plain aligned load (LeanIn, ez_k1_device.h).
#include "ez_k1_internal.h"

#include <cstdio>
#include <cstring>
#include <algorithm>
#include <type_traits>
#include <vector>

namespace ez {
namespace {
using namespace k1;

// gext's view of a padded stream: GW::around without the batch-bounds branch (bytes before the
// stream start read 0; gext reads at most 16 bytes before it and 16 after its end)
struct GWU {
    const uint8_t *p;
    __device__ __forceinline__ void around(int32_t y, uint64_t &before, uint64_t &from) const {
        V16 v = ld16v(p + (y - 8));
        if (y < 8) {
            const int32_t k = 8 - y;
            v.lo &= k >= 8 ? 0ull : ~0ull << (8 * k);
            v.hi &= k >= 16 ? 0ull : (k <= 8 ? ~0ull : ~0ull << (8 * (k - 8)));
        }
        before = v.lo;
        from = v.hi;
    }
};

// The window's bytes from a 128-byte region held across windows, with the next one in flight.
// The group's 144-byte LDS buffer holds stream bytes [cb, cb + 128) (each lane loads 128 / G bytes
// of it, one aligned load); a window at i reads bytes i-8 .. i+38, so the region serves every
// window with 0 <= i - 8 - cb <= R.  Most windows advance by 16 (no accept) or by a short match, so
// a region serves ~4 of them, and the region 64 bytes further on (f, issued one region switch
// earlier, after that window's candidate gathers) is usually resident when the parse gets there:
// the window-bytes load leaves the per-window chain (window bytes -> table -> candidate gather ->
// decision -> next window) except after long jumps.  Regions never start past bmax (their 128
// bytes end at most 64 bytes after the stream) nor more than 64 bytes before it: k1_lean's edge
// slots guarantee both.  A window's 32 bytes are nine aligned dword reads and eight v_alignbyte.
// R: the farthest window start the region serves (80 for 32-byte windows; 64 for the 48-byte
// windows of the 40-byte judgement, whose bytes reach i + 15 + 39)
template <int R = 80, int G = 16>
struct WinLds {
    static constexpr int LB = 128 / G;  // bytes of the 128-byte region per lane (8 or 16)
    typedef unsigned int u32v __attribute__((ext_vector_type(LB / 4)));
    u32v f;  // this lane's dwords of the prefetched region
    int32_t cb, fb, bmax, pm;
    uint8_t *wl;  // the group's buffer (LDS)
    __device__ __forceinline__ int32_t floor4(int32_t y) const { return y - ((pm + y) & 3); }
    __device__ __forceinline__ void ld(const uint8_t *p, int32_t b, int lj, u32v &d) const {
        typedef const __attribute__((address_space(1))) u32v *gp;
        d = *(gp)(p + b + LB * lj);
    }
    __device__ __forceinline__ void put(int lj) const { *(u32v *)(wl + LB * lj) = f; }
    __device__ __forceinline__ void init(const uint8_t *p, int32_t n, int lj, bool live) {
        pm = (int32_t)((uintptr_t)p & 3);
        bmax = floor4(n - 64);
        cb = min(floor4(-8), bmax);
        fb = min(cb + 64, bmax);
        f = u32v{};
        if (live) ld(p, cb, lj, f);
        put(lj);
        if (live) ld(p, fb, lj, f);
    }
    __device__ __forceinline__ void advance(const uint8_t *p, int32_t i, int lj, bool live) {
        const int32_t y = i - 8;
        if (live && !(y >= cb && y - cb <= R)) {
            if (!(y >= fb && y - fb <= R)) {
                fb = min(floor4(y), bmax);
                ld(p, fb, lj, f);
            }
            cb = fb;
            put(lj);
            fb = min(cb + 64, bmax);
            ld(p, fb, lj, f);
        }
    }
    __device__ __forceinline__ void bytes(int32_t i, int g, int lj, V16 &w0, V16 &w1) const {
        const uint32_t o = (uint32_t)(i - 8 - cb + lj), r = o & 3;
        const uint32_t *q = (const uint32_t *)(wl + (o & ~3u));
        uint32_t d[9];
#pragma unroll
        for (int t = 0; t < 9; t++) d[t] = q[t];
        uint32_t b[8];
#pragma unroll
        for (int t = 0; t < 8; t++) b[t] = __builtin_amdgcn_alignbyte(d[t + 1], d[t], r);
        w0.lo = (uint64_t)b[0] | ((uint64_t)b[1] << 32);
        w0.hi = (uint64_t)b[2] | ((uint64_t)b[3] << 32);
        w1.lo = (uint64_t)b[4] | ((uint64_t)b[5] << 32);
        w1.hi = (uint64_t)b[6] | ((uint64_t)b[7] << 32);
    }
    // x-8 .. x+39 (R = 64: o <= 79, the reads end at byte 131 of the 144-byte buffer).  (Three
    // byte-addressed ds_read_b128 instead -- the LDS runs in unaligned mode under ROCm -- save 14
    // VALU per window, the 12 v_alignbyte among them, but measured slower: C1 K1 2.13 against
    // 1.96 ms, two alternating runs on one box; the unaligned reads cost the LDS more cycles)
    __device__ __forceinline__ void bytes48(int32_t i, int g, int lj, V16 &w0, V16 &w1, V16 &w2) const {
        static_assert(R <= 64, "48-byte windows need the region to reach i + 54");
        const uint32_t o = (uint32_t)(i - 8 - cb + lj), r = o & 3;
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

// The 32 bytes y-8 .. y+23 by dword-aligned loads (dwordx4, dwordx4, dword from floor4(p + y - 8))
// and v_alignbyte: a 16-byte load at a byte-unaligned address costs the L1 one access per dword it
// touches, an aligned one a single access (tools/mb_ta.hip, L1-resident: 64 vs 16 ns per scattered
// wave-load), so this is 3 accesses per lane instead of ~8.
__device__ __forceinline__ void bytes32(const LeanIn &L, const uint8_t *p, int32_t y, V16 &c0, V16 &c1) {
    const uintptr_t a = (uintptr_t)(p + y - 8);
    const uint32_t r = (uint32_t)(a & 3);
    const uint8_t *w = (const uint8_t *)(a & ~(uintptr_t)3);
    const uint4 q0 = L.dw4(w), q1 = L.dw4(w + 16);
    const uint32_t q2 = L.dw(w + 32);
    const uint32_t d[9] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2};
    uint32_t b[8];
#pragma unroll
    for (int t = 0; t < 8; t++) b[t] = __builtin_amdgcn_alignbyte(d[t + 1], d[t], r);
    c0.lo = (uint64_t)b[0] | ((uint64_t)b[1] << 32);
    c0.hi = (uint64_t)b[2] | ((uint64_t)b[3] << 32);
    c1.lo = (uint64_t)b[4] | ((uint64_t)b[5] << 32);
    c1.hi = (uint64_t)b[6] | ((uint64_t)b[7] << 32);
}

// y-8 .. y+39 (the 40-byte judgement): dwordx4 x3 + dword from floor4(p + y - 8), unchecked (padded
// streams: k1_lean's edge slots leave 64 readable bytes after every stream)
__device__ __forceinline__ void bytes48(const LeanIn &L, const uint8_t *p, int32_t y, V16 &c0, V16 &c1, V16 &c2) {
    // (floor4(p + y - 8) = floor4(p + y) - 8: one address add, the -8 in the loads' offsets)
    const uintptr_t a = (uintptr_t)(p + y);
    const uint32_t r = (uint32_t)(a & 3);
    const uint8_t *w = (const uint8_t *)(a & ~(uintptr_t)3) - 8;
    const uint4 q0 = L.dw4(w), q1 = L.dw4(w + 16), q2 = L.dw4(w + 32);
    const uint32_t q3 = L.dw(w + 48);
    const uint32_t d[13] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, q3};
    uint32_t b[12];
#pragma unroll
    for (int t = 0; t < 12; t++) b[t] = __builtin_amdgcn_alignbyte(d[t + 1], d[t], r);
    c0 = V16{(uint64_t)b[0] | ((uint64_t)b[1] << 32), (uint64_t)b[2] | ((uint64_t)b[3] << 32)};
    c1 = V16{(uint64_t)b[4] | ((uint64_t)b[5] << 32), (uint64_t)b[6] | ((uint64_t)b[7] << 32)};
    c2 = V16{(uint64_t)b[8] | ((uint64_t)b[9] << 32), (uint64_t)b[10] | ((uint64_t)b[11] << 32)};
}

// The wave's lane mask of one compare.  A ballot of a single compare is that compare's own SGPR
// result; a ballot of a compound bool is first made a VGPR 0/1 (v_cndmask) and compared again
// (v_cmp_ne), two VALU per window each.  So a compound condition is formed from its component
// compares' masks on the scalar side (s_and_b64 / s_or_b64): lanes(a, b) is the mask of a && b.
__device__ __forceinline__ uint64_t lanes(bool c) { return __builtin_amdgcn_ballot_w64(c); }
template <class... B>
__device__ __forceinline__ uint64_t lanes(bool c, B... more) { return lanes(c) & lanes(more...); }

// v + 1 in the lanes of mask m: one add with carry-in (a select of 0 / 1 and an add otherwise)
__device__ __forceinline__ int32_t add_lanes(int32_t v, uint64_t m) {
    asm("v_addc_co_u32_e64 %0, %1, 0, %0, %1" : "+v"(v), "+s"(m));
    return v;
}

// bit 0: s_setprio 3 on the chain up to the candidate loads; bit 2: the i+1 insert by lane a+1
// (EZ_K1S_NEXT1=0 (A/B): by the acceptor, with its own hash).  A constant of the product build,
// so the window carries no branch on it; experiment builds (EZ_KNOBS) take it from the launcher
constexpr int kLeanPrio = 1 | 4;
#ifdef EZ_KNOBS
constexpr bool kLeanPrioKnob = true;
#else
constexpr bool kLeanPrioKnob = false;
#endif

#if (EZ_EXP & 65536)
// [0..17] windows by acceptor lane (0: none); [18], [19] acceptors whose capped count had / had not room
// left; [20] wave iterations that took the gext branch, [21] wave iterations, [22] those in which an
// acceptor had room left (the branch's condition before the limits moved into it)
__device__ unsigned long long g_lean_hist[23];
#endif

// k1_lean's parse of fresh single-Write streams, G lanes (a group) per stream, 64 / G groups per
// wave: the table's visit is lds_mskor16, the window's region is in LDS (WinLds).
// FW: the judgement's forward cap, 24 or 40 bytes (40: 48-byte windows and candidates).
template <int FW, int G>
__device__ __forceinline__ void lean_run(const CompressArgs &A, int lj, int g, uint16_t *hth, uint32_t table_words, uint32_t hsh,
                                         uint64_t *recs, uint64_t rcap, int prio_knob, uint8_t *edge, uint8_t *wl) {
    constexpr int S = 64 / G;
    const int prio = kLeanPrioKnob ? prio_knob : kLeanPrio;
    constexpr uint32_t kGMask = (1u << G) - 1;
    constexpr bool W40 = FW == 40;
    static_assert(FW == 24 || W40, "the judgement's forward cap is 24 or 40 bytes");
    constexpr int32_t CAP = FW;
    const LeanIn L{};
    const uint8_t *blo = A.in, *bhi = A.in + A.in_off[A.count];
    uint32_t *slots = (uint32_t *)(edge + 128 + kEdgeSlots * edge_slot_bytes(A));  // edge slots taken
    const uint32_t rcap32 = (uint32_t)rcap;

    // the group's stream: index, bytes, size, error, record base; its parse state
    uint64_t s = (uint64_t)blockIdx.x * S + (uint64_t)g;
    const uint8_t *p = edge + 16;
    int32_t n = 0, i = 0, done = 0, nrec = 0;
    int32_t nin = 0;  // n - kIn: the last i of an interior window
    int err = 0;
    bool live = false, pending = false;  // pending: the stream's size word is still to be written
    uint64_t *rec = recs;
    V16 z0{0, 0}, z1{0, 0}, z2{0, 0};
    WinLds<W40 ? 64 : 80, G> wr;
    wr.wl = wl;
    // iterations left to the wave (SALU): the bound of its streams' parses, so a correct parse
    // never reaches 0 and a wrong one cannot hang the grid
    int64_t budget = 0;

    // open stream s for the group (group-uniform, in a branch of the group's lanes): table zeroed,
    // edge streams copied into a padded slot, the first region of the window loaded.  (A lambda
    // called once, from when a group took further streams from a queue: spelled inline the compiler
    // allocates the prologue's registers differently, and retiring the queue left the machine code
    // as it was)
    auto open = [&]() {
        pending = s < A.count;
        n = 0;
        const uint8_t *src = blo;
        if (pending) {
            n = (int32_t)(A.in_off[s + 1] - A.in_off[s]);
            src = A.in + A.in_off[s];
        }
        for (int32_t k = 4 * lj; k < (int32_t)table_words; k += 4 * G) *(uint4 *)((uint32_t *)hth + k) = make_uint4(0, 0, 0, 0);
        // the launcher sized records and tables from max_len: longer streams are refused
        err = !pending || (uint64_t)n > A.max_len ? EZ_EINVAL : 0;
        live = !err && n >= 4;
        p = live ? src : edge + 16;
        const bool edge_stream = live && (src - kEdgeBefore < blo || src + n + 64 > bhi);
        if (edge_stream) {
            // [64 zero bytes][the stream][64 zero bytes]
            int32_t slot = 0;
            if (lj == 0) slot = (int32_t)atomicAdd(slots, 1u);
            slot = bcast(slot, G * g);
            if (slot >= kEdgeSlots) {  // cannot happen (the batch has at most two edge regions)
                err = EZ_ESTUCK;
                live = false;
                p = edge + 16;
            } else {
                uint8_t *d = edge + 128 + (uint64_t)slot * edge_slot_bytes(A);
                for (int32_t k = lj; k < n + kEdgeBefore + 64; k += G)
                    d[k] = (k >= kEdgeBefore && k < n + kEdgeBefore) ? src[k - kEdgeBefore] : (uint8_t)0;
                p = d + kEdgeBefore;
            }
            __threadfence_block();
        }
        i = done = nrec = 0;
        nin = n - (G + FW - 1);
        rec = recs + (pending ? s : 0) * rcap;
        wr.init(p, n, lj, live);
        // the bytes around stream position 0, the candidate of every zero table entry:
        // judged without a load (a load for every lane measured 2.35 against 2.00 ms at C1: the
        // vector-memory path is the parse's busiest)
        z0 = z1 = z2 = V16{0, 0};
        if (live) {
            if constexpr (W40) bytes48(L, p, 0, z0, z1, z2);
            else bytes32(L, p, 0, z0, z1);
            z0.lo = 0;
        }
    };
    open();
    budget += (int64_t)(4 * A.max_len + 64) * S;

    V16 w0{0, 0}, w1{0, 0}, w2{0, 0};  // bytes x-8 .. x+7, x+8 .. x+23 (and x+24 .. x+39) of this lane's x

    // A group is interior while its stream is live, its record area has room for a record and
    // i + kIn <= n.  A window at i judges x = i .. i+G-1; with i + G - 1 + CAP <= n, for every lane:
    //  * n - 3 - i >= G: all G positions are visits (nvalid = G, valid);
    //  * n - x >= CAP: the forward count (<= CAP) ends inside the stream, and so does the zero
    //    run's (its candidate is below x: n - cand > CAP, and cand + 8 < n);
    //  * x + 1 + 4 <= n: a window match makes its i+1 insert;
    //  * the window's bytes end at x + CAP - 1 < n.
    // open() keeps nin = n - kIn, so the test before every window is i <= nin.
    // So the interior window has no end clamp, no liveness term and no record-room test; the exact
    // limits of a saturated count are gext's, in both forms of the window.  (The counts alone
    // would bear a bound one byte looser, since a count that reaches CAP goes to gext, which holds
    // it to the stream's end; the bound here is the one at which no lane needs that.)
    constexpr int32_t kIn = G + CAP - 1;
    static_assert(kIn == G + FW - 1, "open()'s nin");

    // One window of every group of the wave.  IN: every group is interior (above); else the
    // general window, which also serves ending streams, dead groups and a full record area.
    auto window = [&](auto in_tag) __attribute__((always_inline)) {
        constexpr bool IN = decltype(in_tag)::value;
        budget--;
        if constexpr (W40) wr.bytes48(i, g, lj, w0, w1, w2);
        else wr.bytes(i, g, lj, w0, w1);
        const int32_t nvalid = IN ? G : (n - 3 - i < G ? n - 3 - i : G);
        const int32_t x = i + lj;
        const bool valid = IN || (live && lj < nvalid);

        // ---- visit (writer.go:213-217): hash, and in one LDS atomic the table's entry or the
        // nearest earlier lane with the same hash, and this lane's position into the table
        if (prio & 1) __builtin_amdgcn_s_setprio(3);
        const uint32_t h = valid ? ((uint32_t)w0.hi * kHashMul) >> hsh : 0u;
        int32_t cand = 0;
        if (valid) cand = (int32_t)lds_mskor16(hth, h, (uint32_t)x);
        V16 c0 = z0, c1 = z1, c2 = z2;
        if (cand != 0) {
            if constexpr (W40) bytes48(L, p, cand, c0, c1, c2);
            else bytes32(L, p, cand, c0, c1);
            // bytes before the stream start are the fresh ring's zeros (rare: a branch)
            if (__builtin_expect(cand < 8, 0)) c0.lo &= ~0ull << (8 * (8 - cand));
        }
        if (prio & 1) __builtin_amdgcn_s_setprio(0);

        // ---- capped judgement, writer.go:219-301 (window) and :441-463 (writeRunlen)
        const bool rl = cand >= done && cand < x;
        const uint64_t e0 = w0.hi ^ c0.hi, e1 = w1.lo ^ c1.lo, e2 = w1.hi ^ c1.hi;
        int32_t jf = W40 ? first_diff40(e0, e1, e2, w2.lo ^ c2.lo, w2.hi ^ c2.hi) : first_diff24(e0, e1, e2);
        if constexpr (!IN) jf = jf < n - x ? jf : n - x;
        int32_t bl = x - done;
        if (rl) bl = bl < cand ? bl : cand;
        int32_t jb = last_diff8(w0.lo ^ c0.lo);
        jb = jb < bl ? jb : bl;
        const bool zr = rl && c0.hi == 0 && (IN || cand + 8 < n);
        const int32_t fw = rl ? jf : (jf < done - cand ? jf : done - cand);
        // acc = valid && (zr || fw + jb >= kMinCopyChunk), as the wave's mask from the single compares
        uint64_t am64 = lanes(cand >= done, cand < x, c0.hi == 0);
        if constexpr (!IN) am64 &= lanes(cand + 8 < n);
        am64 |= lanes(fw + jb >= kMinCopyChunk);
        if constexpr (!IN) am64 &= lanes(live, lj < nvalid);

        // ---- this lane's action if it is the group's first acceptor.  ext: a count that reached
        // its cap (bit 0 forward, bit 1 backward); whether the match has room to go on past the
        // cap is gext's to find, from its exact limits
        int32_t lit, nx, dist, ext;
        bool force = false;
        if (zr) {  // writeZeros :407-439
            int32_t zf = W40 ? first_diff40(0, c1.lo, c1.hi, c2.lo, c2.hi) : first_diff24(0, c1.lo, c1.hi);
            if constexpr (!IN) zf = zf < n - cand ? zf : n - cand;
            int32_t zb = last_diff8(c0.lo);
            zb = zb < cand - done ? zb : cand - done;
            lit = cand - zb;
            nx = cand + zf;
            dist = 0;
            ext = (zf == CAP ? 1 : 0) | (zb == 8 ? 2 : 0);
        } else {  // writeRunlen :441-489 / window match :303-321
            lit = x - jb;
            nx = x + fw;
            dist = x - cand;
            force = rl;
            ext = (jf == CAP ? 1 : 0) | (jb == 8 ? 2 : 0);
        }
        // the group's next position, whether the acceptor's counts reached their caps, and whether
        // it makes the i+1 insert (a window match, writer.go:315-318)
        const bool ins1 = !rl && !zr && (IN || x + 1 + 4 <= n);
        const uint32_t am = (uint32_t)(am64 >> (G * g)) & kGMask;
        const bool any = am != 0;
        const int a = am ? __builtin_ctz(am) : -1;
        const int32_t pack = nx | (ext << 28) | ((int32_t)ins1 << 30);
        // (one ds_bpermute from each group's first acceptor: fewer VALU than four v_readlane + selects)
        const int32_t sel = __builtin_amdgcn_ds_bpermute(4 * (G * g + (a < 0 ? 0 : a)), pack);
        const int a0 = any ? a : 0;  // (a lane to read from where there is no acceptor)
#if (EZ_EXP & 65536)
        if ((IN || live) && lj == 0) atomicAdd(&g_lean_hist[any ? a + 1 : 0], 1ull);  // (experiment builds: the acceptor lane, 0 none)
        if (lj == 0 && g == 0) atomicAdd(&g_lean_hist[21], 1ull);
#endif
        uint64_t actm = lanes(any);
        if constexpr (!IN) actm &= lanes(live);
        const bool act = (IN || live) && any;
        int32_t nxt = sel & 0x0fffffff;
        if ((actm & lanes((sel & (3 << 28)) != 0)) != 0) {
            // rare: a count at its cap; exact lengths by the whole group (as k1_parse).  A count
            // with no room past its cap (flim <= CAP, blim <= 8) comes back from gext as it was.
            // the acceptor's candidate, capped backward count (<= 8) and branch
            const int32_t info = cand | (((zr ? cand : x) - lit) << 16) | ((int32_t)rl << 29) | ((int32_t)zr << 30);
            const int32_t ib = bcast(info, G * g + a0);
            const int32_t xa = i + a0;
            const int32_t ca = ib & 0xffff;
            const bool rla = (ib >> 29) & 1, zra = (ib >> 30) & 1;
            const int32_t e = (sel >> 28) & 3;
            const bool need = act && e != 0;
            const int mode = zra ? 0 : (rla ? 1 : 2);
            const int32_t fa = zra ? ca : xa;
            const int32_t blim = zra ? ca - done : (rla ? ((xa - done) < ca ? (xa - done) : ca) : xa - done);
            const int32_t flim = zra ? n - ca : (rla ? n - xa : ((done - ca) < n - xa ? done - ca : n - xa));
            int32_t fx, cx;
#if (EZ_EXP & 65536)
            if (need && lj == 0) atomicAdd(&g_lean_hist[18 + ((e & 1 && flim > CAP) || (e & 2 && blim > 8) ? 0 : 1)], 1ull);
            if (lj == 0 && g == 0) atomicAdd(&g_lean_hist[20], 1ull);
            if (__builtin_amdgcn_ballot_w64(need && ((e & 1 && flim > CAP) || (e & 2 && blim > 8))) != 0 && lj == 0 && g == 0) atomicAdd(&g_lean_hist[22], 1ull);
#endif
            gext<G, GWU>(GWU{p}, need && (e & 1), need && (e & 2), g, lj, fa, ca, mode, done, CAP, flim, blim, fx, cx);
            if (need) {
                const int32_t f = (e & 1) ? fx : (sel & 0x0fffffff) - fa;
                const int32_t c = (e & 2) ? cx : ((ib >> 16) & 0xf);
                nxt = fa + f;
                if (lj == a) {
                    lit = fa - c;
                    nx = nxt;
                }
            }
        }
        // ---- table: the visited lanes' positions (the last of a hash wins), then lane a's i+1.
        // Lanes past the acceptor put back what their visit found (visits Go never makes); lane a+1
        // hashed position i+1 itself and is the only lane past a that restores that entry, so it
        // writes i+1 there instead when the acceptor makes the insert (prio bit 2; the acceptor
        // still does it when a is the group's last lane)
        const bool ins_next = (prio & 4) && a >= 0 && a < G - 1 && ((sel >> 30) & 1);
        if (valid && a >= 0 && lj > a && cand <= i + a) hth[h] = (uint16_t)(ins_next && lj == a + 1 ? x : cand);
        if (act && lj == a && !ins_next) {
            if (ins1) {
                const uint32_t h1 = ((uint32_t)(w0.hi >> 8) * kHashMul) >> hsh;
                hth[h1] = (uint16_t)(x + 1);
            }
        }
        // the record, stored after the next region's load is issued (a region switch waits for every
        // vector-memory operation before it, stores included), at the count as it was: nrec - 1 by
        // then, the -1 in the store's offset
        const bool st_rec = act && lj == a;
        const Rec32 rv = rec_pack32(lit, nx - lit, dist, force);
        const bool rec_room = IN || (uint32_t)nrec < rcap32;
        nrec = add_lanes(nrec, actm);
        if (act) {
            if (!rec_room) { err = EZ_ESTUCK; live = false; }
            i = done = nxt;
        } else if (IN || live) {
            i += nvalid;
        }
        // (an interior group that reaches its stream's end is marked when the interior loop ends)
        if constexpr (!IN) {
            if (live && (err || i + 4 > n)) live = false;
        }
        wr.advance(p, i, lj, IN || live);  // the next window's region (up to the stream's end: in bounds)
        __builtin_amdgcn_sched_barrier(0);
        if (st_rec && rec_room) __builtin_nontemporal_store(u32x2{rv.lo, rv.hi}, (u32x2 *)(rec + (uint32_t)nrec - 1));
    };

    for (;;) {
        // groups whose stream ended: its size word
        if (__builtin_amdgcn_ballot_w64(!live && pending) != 0) {
            if (!live && pending) {
                if (lj == 0) A.out_size[s] = (uint64_t)nrec | ((uint64_t)err << 48);
                pending = false;
            }
        }
        if (__builtin_amdgcn_ballot_w64(live) == 0) break;
        if (budget < 0) {
            if (live) err = EZ_ESTUCK;
            live = false;
            continue;
        }
        // the interior loop, while every group of the wave is interior: the test is made before
        // every window, so the window itself needs none.  It counts the budget down and leaves the
        // test of it to this outer loop: every window advances its group's i or, where a match
        // ends at i itself, done up to i (done <= i <= n), so the loop ends within 2n windows
        // whatever the budget says, and a wrong parse still cannot hang the grid.
        if (lanes(live, i <= nin, (uint32_t)nrec < rcap32) == ~0ull) {
            do {
                window(std::true_type{});
            } while (lanes(i <= nin, (uint32_t)nrec < rcap32) == ~0ull);
            // a match that ran to the stream's end; the group that left the interior has its next
            // window in the general loop below
            if (i + 4 > n) live = false;
            continue;
        }
        // the general loop, until one of the groups' streams ends (the bookkeeping above stays out
        // of it): a group leaves the interior for good, so the wave does not return to it
        const uint64_t lm = __builtin_amdgcn_ballot_w64(live);
        do {
            window(std::false_type{});
        } while (__builtin_amdgcn_ballot_w64(live) == lm && budget >= 0);
    }
}

// Edge slots (after the records in the K1 scratch): a zeroed 128-byte dummy region for lane groups
// without a stream, then kEdgeSlots slots of edge_slot_bytes, then the slot counter (zeroed by the
// launcher).  A live stream (n >= 4) lacks the 64 bytes before or the 64 after it only if it starts
// in the batch's first 64 bytes (at most 16 such streams, each >= 4 bytes) or ends in its last 64
// (at most 16): 32 slots always suffice.

// waves per SIMD the VGPR budget is cut for: 8-lane groups are held to ~2 by their tables' LDS, so
// they keep VGPRs (no spills)
constexpr int kLeanWaves16 = 5;
#if (EZ_EXP & 2097152)
constexpr uint32_t kLeanTMax = 1u << 18;
__device__ uint64_t g_lean_t[2 * kLeanTMax];
#endif
template <int FW, int G>
__global__ __launch_bounds__(64, G == 8 ? 2 : kLeanWaves16) void k1_lean(CompressArgs A, uint32_t stride_words, uint32_t table_words, uint64_t *recs,
                                                                          uint64_t rcap, int prio, uint8_t *edge) {
    constexpr int S = 64 / G;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int lane = (int)(threadIdx.x & 63);
    const int g = lane / G, lj = lane % G;
    const int32_t hs = (int32_t)A.hs;
    const uint32_t hsh = 32u - (uint32_t)(64 - __builtin_clzll((uint64_t)(hs - 1)));
    uint16_t *hth = (uint16_t *)((uint32_t *)smem + (uint32_t)g * stride_words);
    // (the groups' window buffers after the S tables)
    uint8_t *wl = smem + (size_t)4 * stride_words * S + (size_t)g * kWinLdsBytes;
#if (EZ_EXP & 2097152)
    const uint64_t t_start = __builtin_amdgcn_s_memrealtime();
#endif
    lean_run<FW, G>(A, lj, g, hth, table_words, hsh, recs, rcap, prio, edge, wl);
#if (EZ_EXP & 2097152)
    {  // (timing builds) the wave's start and end (100 MHz), its XCC and CU
        const uint64_t t_end = __builtin_amdgcn_s_memrealtime();
        uint32_t hw = 0, xcc = 0;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        if (lane == 0 && blockIdx.x < kLeanTMax) {
            g_lean_t[2 * blockIdx.x] = t_start;
            g_lean_t[2 * blockIdx.x + 1] = (t_end & 0xffffffffffull) | ((uint64_t)((hw >> 8) & 15) << 40) | ((uint64_t)((hw >> 13) & 7) << 44) |
                                           ((uint64_t)((hw >> 12) & 1) << 47) | ((uint64_t)(xcc & 15) << 48) | ((uint64_t)((hw >> 4) & 3) << 52);
        }
    }
#endif
}

#if (EZ_EXP & 2097152)
// (timing builds) after a launch of `blocks` waves: waves active over time, and when each XCC's
// last wave ends
void lean_report_timeline(uint64_t blocks, hipStream_t st) {
    const uint64_t nb = blocks < kLeanTMax ? blocks : kLeanTMax;
    std::vector<uint64_t> t(2 * nb);
    (void)hipStreamSynchronize(st);
    (void)hipMemcpyFromSymbol(t.data(), HIP_SYMBOL(g_lean_t), 16 * nb);
    uint64_t t0 = ~0ull, t1 = 0, xe[16] = {0}, xs[16], cnt[16] = {0};
    for (int k = 0; k < 16; k++) xs[k] = ~0ull;
    for (uint64_t b = 0; b < nb; b++) {
        const uint64_t st0 = t[2 * b] & 0xffffffffffull, en = t[2 * b + 1] & 0xffffffffffull;
        const int x = (int)((t[2 * b + 1] >> 48) & 15);
        t0 = st0 < t0 ? st0 : t0;
        t1 = en > t1 ? en : t1;
        xe[x] = en > xe[x] ? en : xe[x];
        xs[x] = st0 < xs[x] ? st0 : xs[x];
        cnt[x]++;
    }
    const int bins = 40;
    std::vector<double> act(bins, 0.0);
    std::vector<uint64_t> ends(nb), lens(nb);
    for (uint64_t b = 0; b < nb; b++) {
        const uint64_t st0 = (t[2 * b] & 0xffffffffffull) - t0, en = (t[2 * b + 1] & 0xffffffffffull) - t0;
        ends[b] = en;
        lens[b] = en - st0;
        for (int k = 0; k < bins; k++) {
            const double lo = (double)(t1 - t0) * k / bins, hi = (double)(t1 - t0) * (k + 1) / bins;
            const double ov = std::min((double)en, hi) - std::max((double)st0, lo);
            if (ov > 0) act[k] += ov / (hi - lo);
        }
    }
    std::sort(ends.begin(), ends.end());
    std::sort(lens.begin(), lens.end());
    fprintf(stderr, "lean waves %llu span %.1f us; wave life p10 %.1f p50 %.1f p90 %.1f max %.1f us; end p50 %.1f p90 %.1f p99 %.1f us\n",
            (unsigned long long)nb, (t1 - t0) / 100.0, lens[nb / 10] / 100.0, lens[nb / 2] / 100.0, lens[nb * 9 / 10] / 100.0, lens[nb - 1] / 100.0,
            ends[nb / 2] / 100.0, ends[nb * 9 / 10] / 100.0, ends[nb * 99 / 100] / 100.0);
    fprintf(stderr, "lean active waves per bin of %.1f us:", (t1 - t0) / 100.0 / bins);
    for (int k = 0; k < bins; k++) fprintf(stderr, " %.0f", act[k]);
    fprintf(stderr, "\nlean per xcc (waves, first start, last end, us):");
    for (int x = 0; x < 16; x++)
        if (cnt[x]) fprintf(stderr, " [%d %llu %.1f %.1f]", x, (unsigned long long)cnt[x], (xs[x] - t0) / 100.0, (xe[x] - t0) / 100.0);
    fprintf(stderr, "\n");
}
#endif
#if (EZ_EXP & 65536)
// (experiment builds) the acceptor-lane histogram of the launch before
void lean_report_hist(hipStream_t st) {
    unsigned long long hst[23];
    (void)hipStreamSynchronize(st);
    (void)hipMemcpyFromSymbol(hst, HIP_SYMBOL(g_lean_hist), sizeof hst);
    unsigned long long tot = 0, vis = 0;
    for (int t = 0; t < 18; t++) tot += hst[t];
    for (int t = 1; t < 17; t++) vis += hst[t] * (unsigned long long)t;
    vis += hst[0] * 16ull;
    fprintf(stderr, "lean windows %llu (no accept %llu); visited lanes %.3f of 16; by acceptor lane:", tot, hst[0], (double)vis / (double)tot);
    for (int t = 1; t < 17; t++) fprintf(stderr, " %.3f", (double)hst[t] / (double)tot);
    fprintf(stderr, "\nlean capped counts: %llu acceptors with room left, %llu without; gext branch in %llu of %llu wave iterations (%.2f %%), %llu with room left (%.2f %%)\n",
            hst[18], hst[19], hst[20], hst[21], 100.0 * (double)hst[20] / (double)(hst[21] ? hst[21] : 1), hst[22],
            100.0 * (double)hst[22] / (double)(hst[21] ? hst[21] : 1));
    memset(hst, 0, sizeof hst);
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_lean_hist), hst, sizeof hst);
}
#endif

template <int FW, int G>
hipError_t launch_lean_v(const CompressArgs &a, uint64_t *recs, uint32_t stride, uint32_t tw, size_t lds, int prio, uint8_t *edge,
                         hipStream_t st) {
    static bool attr_done = false;
    if (!attr_done) {
        (void)hipFuncSetAttribute((const void *)k1_lean<FW, G>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        attr_done = true;
    }
    constexpr uint64_t S = 64 / G;
    const uint64_t blocks = (a.count + S - 1) / S;
    hipLaunchKernelGGL((k1_lean<FW, G>), dim3((unsigned)blocks), dim3(64), lds, st, a, stride, tw, recs, rec_cap(a), prio, edge);
    return hipGetLastError();
}

}  // namespace

// (the caller has checked lds_mskor_in_lane_order: the visit is one ds_mskor)
hipError_t launch_lean(const CompressArgs &a, uint64_t *recs, hipStream_t st) {
    // 8-lane groups (8 streams per wave) for streams over 4 KiB: a window's acceptor is one of lanes
    // 0..7 in 74 % of C1's windows (6.3 of 16 lanes are visits on average), so half-width windows
    // take ~37 % fewer wave iterations; with the same streams per CU (the tables bound them) but half
    // the waves, C1 measured 2.01 -> 2.14 ms, 8 KiB streams 8.58 -> 8.11, 16 KiB 11.06 -> 9.49 (with
    // the 40-byte judgement), 64 KiB 14.10 -> 11.67.  (8 tables of at most 4,096 u16 entries fit
    // the LDS: split_stride<8, true> is never 0 where split_stride<16, true> is not)
    const bool g8 = a.max_len > 4096;
    // the judgement's forward cap: 40 bytes (48-byte windows and candidates; C1 K1 2.081 -> 2.012 ms,
    // A/B on one box) for streams up to 16 KiB (8-lane groups: 9.79 -> 9.49 ms), else 24 (8-lane at
    // 64 KiB 11.67 against 11.77; 16-lane groups at 16 and 64 KiB ran 9-12 % slower with 40)
    const bool w40 = a.max_len <= 16384;
    const int S = g8 ? 8 : 4;
    const uint32_t stride = split_stride<16, true>(a), tw = split_table_words<true>(a);
    const uint64_t rcap = rec_cap(a);
    // (kLeanPrio's bits; the product build's kernels have them as constants)
    static const int prio = knob("EZ_K1S_PRIO", kLeanPrio & 1) | (knob("EZ_K1S_NEXT1", 1) ? (kLeanPrio & 4) : 0);
    uint8_t *edge = (uint8_t *)(recs + a.count * rcap);
    // (the edge area's first 128 bytes: the dummy region of idle groups; its last 16: the edge-slot
    // counter)
    hipError_t z = hipMemsetAsync(edge, 0, 128, st);
    if (z == hipSuccess) z = hipMemsetAsync(edge + 128 + kEdgeSlots * edge_slot_bytes(a), 0, 16, st);
    if (z != hipSuccess) return z;
    // EZ_K1S_LDSPAD (experiments): extra LDS per block, to cap the streams resident per CU
    static const size_t pad = (size_t)knob("EZ_K1S_LDSPAD", 0);
    // the tables, then the groups' window regions (WinLds; C1 K1 2.18 -> 2.08 ms against the region
    // in the lanes' registers, A/B on one box)
    const size_t lds = (size_t)stride * 4 * S + (size_t)kWinLdsBytes * S + pad;
    hipError_t e;
    const char *route;  // group width and forward cap
    if (!g8) route = "s:lean g16 fw40", e = launch_lean_v<40, 16>(a, recs, stride, tw, lds, prio, edge, st);
    else if (w40) route = "s:lean g8 fw40", e = launch_lean_v<40, 8>(a, recs, stride, tw, lds, prio, edge, st);
    else route = "s:lean g8 fw24", e = launch_lean_v<24, 8>(a, recs, stride, tw, lds, prio, edge, st);
    set_compress_route(route);
    if (e != hipSuccess) return e;
#if (EZ_EXP & 2097152)
    lean_report_timeline((a.count + S - 1) / S, st);
#endif
#if (EZ_EXP & 65536)
    lean_report_hist(st);
#endif
    return launch_emit(a, recs, rcap, false, st);
}

}  // namespace ez
