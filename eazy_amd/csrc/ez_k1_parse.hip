// ez_k1_parse.hip — K1s: batch compression of fresh streams in two
// kernels, the greedy parse (K1p) and the token writer (K1e).
//
// Writer.Write (writer.go:206-337) for a fresh stream (SURVEY §8 unit of
// work; 2n <= block, so the ring is the linear history with zeros from `done`
// on: no far skip, no cut, no trim 1).
//
// Why two kernels.  The parse is a serial chain per stream: every window's
// decision needs the table after the previous one.  Writing the tokens
// (Encoder.Tag/Offset :537-597, appendLiteral/appendCopy :519-527) does not
// feed back into that chain, but done inside it (a one-kernel form, round 1) it puts the literal
// loads, the encodes and the stores on every iteration's critical path.  Here
//   K1p (G lanes per stream, the table in LDS) runs only the chain: visit,
//       capped judgement, exact extension of an accepted match, the i+1
//       insert, and one 8-byte match record per accepted match
//       {lit_end, copy length, distance, flag} into a per-stream record slot;
//   K1e (one wave per stream) turns the records into the byte stream: token
//       sizes, a wave prefix sum for their output positions, then every lane
//       writes its token (literal tag, literal bytes, copy tag + offset) with
//       16-byte stores and exact-length tails; long literals are copied by the
//       whole wave.  Streams whose tokens do not fit their slot stop at the
//       last token that fits (EZ_ENOSPC), as the single-kernel path does.
//
// The window.  The G lanes of a stream judge positions i .. i+G-1 at once
// against the table as Go's sequential visits (writer.go:213-217) would leave
// it, and the first accepting lane wins.  Two ways to visit a window:
//   T16 (u16 table, 2 bytes per entry, twice the streams per CU of T32):
//       lanes read the table, a lane's candidate is the nearest earlier lane of
//       the window with the same hash (DPP row shifts) or else the table value,
//       and after the decision the lanes Go visits (those up to the accepting
//       one) store their positions with one ds_write_b16, where same-address
//       stores of one instruction land in ascending lane order (checked on the
//       device once per process; T32 is used if it fails).  Exact for any
//       table contents, so backward jumps need nothing special.
//   T32 (u32 table): one ds_wrxchg_rtn_b32 visits the window in lane order,
//       inserts of lanes Go does not visit are undone with one ds_min_u32,
//       which needs inserts monotone in position: windows that start at or
//       below the highest inserted position are judged one position at a time.
// Acceptance is decided with capped counts, 24 bytes forward and 8 backward
// (minCopyChunk = 6 < 8, writer.go:119, 301); only a saturated count is
// extended, forward and backward at once, 16 bytes per lane.  Each accepted match advances `done` by
// its copy length (>= 6), so a stream of n bytes makes at most n/6 records.
//
// This file holds K1p's general form, k1_parse (multi-Write streams, the u32 table, and the
// single-Write u16 batch of a device whose ds_mskor probe fails), and its launcher.  The other
// families: ez_k1_lean.hip (single-Write u16 batches), ez_k1_long.hip (K1L), ez_k1_chunk.hip (K1c),
// ez_k1_emit.hip (K1e); ez_compress_split.hip routes a batch to one of them.
#include "ez_k1_internal.h"

#include <cstdio>

namespace ez {
namespace {
using namespace k1;

// v of the lane K below in the same 16-lane row (~0u where there is none)
template <int K>
__device__ __forceinline__ uint32_t row_shr(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)~0u, (int)v, 0x110 + K, 0xf, 0xf, false);
}
// distance to the nearest earlier lane of the group with the same hash (0: none)
// (ROW: the group is the whole 16-lane row, so a lane K below outside it reads ~0u and never matches)
template <int K, bool ROW>
struct Pred {
    __device__ __forceinline__ static int32_t get(uint32_t h, int lj, int32_t d) {
        const uint32_t hk = row_shr<K>(h);
        d = ((ROW || K <= lj) && hk == h) ? K : d;  // descending K: the nearest one stays
        return Pred<K - 1, ROW>::get(h, lj, d);
    }
};
template <bool ROW>
struct Pred<0, ROW> {
    __device__ __forceinline__ static int32_t get(uint32_t, int, int32_t d) { return d; }
};

// ---------------------------------------------------------------- K1p
// MW: streams of several Writes (CompressArgs::write_idx), else one Write each
template <int G, bool T16, bool MW>
__global__ __launch_bounds__(64, 5) void k1_parse(CompressArgs A, uint32_t stride_words, uint32_t table_words, uint64_t *recs,
                                                  uint64_t rcap, int prio) {
    constexpr int S = 64 / G;
    static_assert(!T16 || G <= 16, "T16 predecessor search works within 16-lane DPP rows");
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int lane = (int)(threadIdx.x & 63);
    const int g = lane / G, lj = lane % G;
    const int32_t hs = (int32_t)A.hs;
    const uint32_t hsh = 32u - (uint32_t)(64 - __builtin_clzll((uint64_t)(hs - 1)));
    uint32_t *htw = (uint32_t *)smem + (uint32_t)g * stride_words;
    uint16_t *hth = (uint16_t *)htw;

    const uint64_t s = (uint64_t)blockIdx.x * S + g;
    const bool have = s < A.count;
    int32_t n = 0;
    const uint8_t *gp = A.in;
    if (have) {
        n = (int32_t)(A.in_off[s + 1] - A.in_off[s]);
        gp = A.in + A.in_off[s];
    }
    GW P;  // stream bytes through L1/L2 (staging them in LDS after the table cost residency: round 1)
    P.p = gp;
    P.blo = A.in;
    P.bhi = A.in + A.in_off[A.count];
    uint64_t *rec = recs + (have ? s * rcap : 0);
    // ht zero = stream position 0 (writer.go:183, A.2)
    for (int32_t k = 4 * lj; k < (int32_t)table_words; k += 4 * G) *(uint4 *)(htw + k) = make_uint4(0, 0, 0, 0);

    // the launcher sized records and tables from max_len: longer streams are refused
    int err = have && (uint64_t)n > A.max_len ? EZ_EINVAL : 0;
    int32_t i = 0, done = 0, hiw = -1, nrec = 0;  // hiw: highest position in the table (T32)
    // Writes of the stream (writer.go:206: each Write's loop runs to its own len(p)):
    // wend = the current Write's end, wk / wlast = its index / the last one's
    uint64_t wk = 0, wlast = 0;
    int32_t wend = n, wstart = 0;
    if (MW && have) {
        wk = A.write_idx[s];
        wlast = A.write_idx[s + 1] - 1;
        if (A.write_idx[s + 1] <= wk) err = EZ_EINVAL;
        // more Writes than the caller's max_writes: their end markers have no record reserved (rec_cap);
        // refused here with the status of the record guard below, whether or not the records would run out
        else if (!err && A.write_idx[s + 1] - wk > A.max_writes) err = EZ_ESTUCK;
        else wend = (int32_t)(A.write_end[wk] - A.in_off[s]);
    }
    bool live = have && !err && (n >= 4 || wk < wlast);
    int32_t guard = 4 * n + 64 + 2 * (int32_t)(wlast - wk);
    // bytes x-8 .. x+7 around this lane's position x (loaded one window ahead)
    // and x+8 .. x+23 (px2, px3), loaded with them: off the table -> candidate chain
    uint64_t pxb = 0, pxf = 0, px2 = 0, px3 = 0;
    if (live) {
        P.around(i + lj, pxb, pxf);
        P.around(i + lj + 16, px2, px3);
    }
#if (EZ_EXP & 4)
    uint64_t prof[8] = {0, 0, 0, 0, 0, 0, 0, 0}, prof_t = __builtin_amdgcn_s_memtime(), prof_it = 0;
#endif
    while (__ballot(live) != 0) {
#if (EZ_EXP & 4)
        prof_it++;
#endif
        if (live && --guard < 0) { err = EZ_ESTUCK; live = false; }
        // a Write that has no position left ends (its trailing literal, writer.go:324-329, is
        // the emitter's: a marker record), and the next Write starts where it ended
        while (MW && live && i + 4 > wend && wk < wlast) {
            if (lj == 0 && (uint64_t)nrec < rcap) __builtin_nontemporal_store(rec_pack(wend, 0, 0, false), rec + nrec);
            if ((uint64_t)nrec >= rcap) { err = EZ_ESTUCK; live = false; }
            nrec++;
            i = done = wstart = wend;
            wk++;
            wend = (int32_t)(A.write_end[wk] - A.in_off[s]);
            if (live) {
                P.around(i + lj, pxb, pxf);
                P.around(i + lj + 16, px2, px3);
            }
        }
        if (live && i + 4 > wend) live = false;  // the last Write has no position left
        int32_t nvalid = wend - 3 - i < G ? wend - 3 - i : G;
        if (!T16 && i <= hiw) nvalid = 1;  // T32, not monotone: one position per window
        const int32_t x = i + lj;
        const bool valid = live && lj < nvalid;

        // ---- visit: hash, lookup (+ insert for T32) in lane order, writer.go:213-217
        // (the chain up to the candidate loads' issue at high wave priority: the loads leave
        // sooner when several waves of the SIMD are ready)
        if (prio & 1) __builtin_amdgcn_s_setprio(3);
        const uint32_t h = valid ? ((uint32_t)pxf * kHashMul) >> hsh : 0u;
        int32_t cand = 0;
        if constexpr (T16) {
            const int32_t tv = valid ? (int32_t)hth[h] : 0;
            const int32_t d = Pred<G - 1, G == 16>::get(h, lj, 0);
            cand = d ? x - d : tv;
        } else {
            if (valid) cand = (int32_t)atomicExch(&htw[h], (uint32_t)x);
        }
        EZ_PROF_MARK(0);

        // ---- capped judgement (exact decision), writer.go:219-301, writeRunlen :441-463
        bool acc = false;
        int32_t info = 0;  // cand | forward count << 20 | backward count << 25 | rl << 29 | zr << 30
        uint64_t pcb = 0, pcf = 0, pc2 = 0, pc3 = 0;
        if (valid) {  // the candidate's bytes, in one wait
            P.around(cand, pcb, pcf);
            P.around(cand + 16, pc2, pc3);
        }
        if (prio & 1) __builtin_amdgcn_s_setprio(0);
        EZ_PROF_MARK(5);
        if (valid) {
            const bool rl = cand >= done && cand < x;
            const bool zr = rl && cand + 8 < wend && pcf == 0;
            // writeRunlen's backward scan stays inside this Write's p (st+jb >= 0, writer.go:458)
            const int32_t bl = rl ? ((x - done) < cand - wstart ? (x - done) : cand - wstart) : x - done;
            int32_t jb = clz_bytes(pxb ^ pcb);
            jb = jb < bl ? jb : bl;
            // forward, 24 bytes capped; the window branch compares the ring image (0 from done on)
            V16 c2{pc2, pc3};
            if (!rl) c2 = keep_low16(c2, done - cand - 8);
            const uint64_t d0 = pxf ^ (rl ? pcf : low_bytes(pcf, done - cand));
            const uint64_t d1 = px2 ^ c2.lo, d2 = px3 ^ c2.hi;
            int32_t jf = d0 ? ctz_bytes(d0) : (d1 ? 8 + ctz_bytes(d1) : 16 + ctz_bytes(d2));
            jf = jf < wend - x ? jf : wend - x;
            acc = rl ? (zr || jf + jb >= kMinCopyChunk) : ((jf < done - cand ? jf : done - cand) + jb >= kMinCopyChunk);
            int32_t zb = clz_bytes(pcb);
            zb = zb < cand - done ? zb : cand - done;
            // zero region: the zeros from cand on, 24 bytes capped
            int32_t zf = pc2 ? 8 + ctz_bytes(pc2) : 16 + ctz_bytes(pc3);
            zf = zf < wend - cand ? zf : wend - cand;
            const int32_t fk = zr ? zf : jf, bk = zr ? zb : jb;
            info = cand | (fk << 20) | (bk << 25) | ((int32_t)rl << 29) | ((int32_t)zr << 30);
        }
        EZ_PROF_MARK(1);
        const uint32_t am = gball<G>(acc, g);
        const int a = am ? __builtin_ctz(am) : -1;  // the group's first accepting lane

        // ---- T32: undo the inserts of the lanes Go does not visit
        if constexpr (!T16) {
            if (valid && a >= 0 && lj > a) atomicMin(&htw[h], (uint32_t)cand);
        }

        // ---- the accepted match: exact lengths (cooperative extension of saturated counts)
        const int32_t ib = bcast(info, G * g + (a < 0 ? 0 : a));
        // the hash of xa+1 is lane a+1's (when it visited), for the extra insert
        const uint32_t h1v = (uint32_t)bcast((int32_t)h, G * g + (a + 1 < G ? a + 1 : G - 1));
        const bool act = live && a >= 0;
        const int32_t xa = i + a;
        const int32_t ca = ib & 0xfffff, fk = (ib >> 20) & 0x1f, bk8 = (ib >> 25) & 0xf;
        const bool rl = (ib >> 29) & 1, zr = (ib >> 30) & 1;
        const int mode = zr ? 0 : (rl ? 1 : 2);
        const int32_t fa = zr ? ca : xa;
        EZ_PROF_MARK(2);
        const int32_t blim = zr ? ca - done : (rl ? ((xa - done) < ca - wstart ? (xa - done) : ca - wstart) : xa - done);
        int32_t fx, cx;
        gext<G, GW>(P, act && fk == 24, act && bk8 == 8, g, lj, fa, ca, mode, done, 24, wend - fa, blim, fx, cx);
        const int32_t f = fk == 24 ? fx : fk;
        const int32_t c = bk8 == 8 ? cx : bk8;
        EZ_PROF_MARK(3);
        int32_t lit_end = 0, nxt = 0;
        if (act) {
            if (zr) {  // writeZeros :407-439
                lit_end = ca - c;
                nxt = ca + f;
            } else if (rl) {  // writeRunlen :441-489
                lit_end = xa - c;
                nxt = xa + f;
            } else {  // window match, trim 2 (:292-296)
                const int32_t over = ca + f - done;
                lit_end = xa - c;
                nxt = xa + f - (over > 0 ? over : 0);
            }
            const int32_t top = rl ? xa : xa + 1;
            hiw = hiw > top ? hiw : top;
            i = done = nxt;
        } else if (live) {
            const int32_t top = i + nvalid - 1;
            hiw = hiw > top ? hiw : top;
            i += nvalid;
        }
        if (live && (err || (i + 4 > wend && wk == wlast))) live = false;
        // the next window's bytes, in flight while this window's table writes and record go out
        EZ_PROF_MARK(6);
        if (prio & 2) __builtin_amdgcn_s_setprio(3);
        if (live) {
            P.around(i + lj, pxb, pxf);
            P.around(i + lj + 16, px2, px3);
        }
        if (prio & 2) __builtin_amdgcn_s_setprio(0);
        EZ_PROF_MARK(7);

        // ---- T16: the lanes Go visits store their positions (the last of a hash wins)
        if constexpr (T16) {
            if (valid && (a < 0 || lj <= a)) hth[h] = (uint16_t)x;
        }
        if (act && lj == 0) {
            if ((uint64_t)nrec < rcap)
                // non-temporal: the records must not evict the streams' inputs from L2
                __builtin_nontemporal_store(rec_pack(lit_end, nxt - lit_end, zr ? 0 : xa - ca, rl && !zr), rec + nrec);
            // the extra insert of i+1 after a window match (writer.go:315-318)
            if (!rl && xa + 1 + 4 <= wend) {
                const uint32_t h1 = a + 1 < nvalid ? h1v : ((P.u32(xa + 1) * kHashMul) >> hsh);
                if constexpr (T16) hth[h1] = (uint16_t)(xa + 1);
                else htw[h1] = (uint32_t)(xa + 1);
            }
        }
        if (act) {
            if ((uint64_t)nrec >= rcap) { err = EZ_ESTUCK; live = false; }
            nrec++;
        }
        EZ_PROF_MARK(4);
    }
#if (EZ_EXP & 4)
    if (blockIdx.x < 4 && lane == 0)
        printf("prof blk %u it %llu: visit %llu cload %llu judge %llu ballot %llu ext %llu upd %llu xload %llu fin %llu\n", blockIdx.x,
               (unsigned long long)prof_it, (unsigned long long)prof[0], (unsigned long long)prof[5], (unsigned long long)prof[1],
               (unsigned long long)prof[2], (unsigned long long)prof[3], (unsigned long long)prof[6], (unsigned long long)prof[7],
               (unsigned long long)prof[4]);
#endif
    if (have && lj == 0) A.out_size[s] = (uint64_t)nrec | ((uint64_t)err << 48);
}

}  // namespace

template <int G, bool T16, bool MW>
hipError_t launch_split_g(const CompressArgs &a, uint64_t *recs, hipStream_t st) {
    static bool attr_done = false;
    if (!attr_done) {
        (void)hipFuncSetAttribute((const void *)k1_parse<G, T16, MW>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        attr_done = true;
    }
    constexpr int S = 64 / G;
    const uint32_t stride = split_stride<G, T16>(a), tw = split_table_words<T16>(a);
    const uint64_t rcap = rec_cap(a);
    const unsigned grid = (unsigned)((a.count + S - 1) / S);
    // EZ_K1S_LDSPAD (experiments): extra LDS per block, to cap the streams resident per CU
    static const size_t pad = (size_t)knob("EZ_K1S_LDSPAD", 0);
    // wave priority (s_setprio 3) on the chain up to the candidate loads' issue: bit 0 (default),
    // bit 1 around the next window's load; EZ_K1S_PRIO=0|1|2|3 (A/B, same box: 3.58 / 3.52 /
    // 3.58 / 3.53 ms at C1)
    static const int prio = knob("EZ_K1S_PRIO", 1);
    set_compress_route(T16 ? (MW ? "s:parse t16 mw" : "s:parse t16") : (MW ? "s:parse t32 mw" : "s:parse t32"));
    hipLaunchKernelGGL((k1_parse<G, T16, MW>), dim3(grid), dim3(64), (size_t)stride * 4 * S + pad, st, a, stride, tw, recs, rcap,
                       prio);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_emit(a, recs, rcap, false, st);
}
template hipError_t launch_split_g<16, true, true>(const CompressArgs &, uint64_t *, hipStream_t);
template hipError_t launch_split_g<16, true, false>(const CompressArgs &, uint64_t *, hipStream_t);
template hipError_t launch_split_g<16, false, true>(const CompressArgs &, uint64_t *, hipStream_t);
template hipError_t launch_split_g<16, false, false>(const CompressArgs &, uint64_t *, hipStream_t);
template hipError_t launch_split_g<32, false, true>(const CompressArgs &, uint64_t *, hipStream_t);
template hipError_t launch_split_g<32, false, false>(const CompressArgs &, uint64_t *, hipStream_t);

}  // namespace ez
