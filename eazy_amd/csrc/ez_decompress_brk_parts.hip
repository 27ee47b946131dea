// ez_decompress_brk_parts.hip — K2b's parts route: the Break index of long streams cut over many waves,
// for the few long framed logs that the wave route (k2b_walk, ez_decompress_brk.hip) gives one wave
// each, twice over where they own Breaks.
//
// The steps are ez_k2_brk_parts.h's, over K2z's part grid (ez_k2_parts.h) and K2g's record
// (ez_k2_segs_parts.h).  Kernels on the caller's stream, which never wait for it:
//   kp_layout (ez_decompress_parts.hip's, through launch_parts_layout; the steps are ez_k2_layout.h's)
//             checks the caller's in_bytes hint against the real extent and lays the streams' parts
//             out; on a mismatch it leaves the gate closed: the kernels of this file do nothing, and
//             k2b_walk, launched behind them with the gate and the layout in its arguments, walks every
//             stream, else only the streams without parts (empty, 2 GiB or more);
//   kq_first  a wave per part, grid-stride: kz_walk (ez_k2_walk.h) over the part with the warm-up chunk
//             before it, kq_sum per lane, the lanes' sums joined as a tree (kq_append), the record;
//   kq_order  a wave per stream, 64 records per load: follows the true chain through the records
//             (kq_class, kq_take), walks again from the true state the parts whose record starts
//             elsewhere or is marked kSWalk (kb_block, ez_k2_brk_walk.h: the body k2b_walk runs over a
//             super-block, with a put that does nothing), leaves every part's entry state, and ends as
//             k2b_walk's count pass ends: out_size, EZ_OK, brk_idx[s] = the stream's Breaks and
//             handed[s] = 0, or brk_idx[s] = 0, handed[s] = 1 and the stream on the hand-over list (a
//             stop is all or nothing: the exact decoder takes the whole stream);
//   (k2b_walk's count pass, the exact count and k2b_scan, ez_decompress_brk.hip)
//   kq_fill   a wave per part whose true chain holds a Break, whose entry state is live and whose
//             stream was not handed over, where brk_total[0] != 0: kb_block from the entry state with
//             the filling put, one plain store per Break from the lane that holds it (lane 0 behind an
//             event) at brk_pos[brk_idx[s] + its index in the stream].  A part without Breaks is never
//             staged again.
// The scratch ([header][part bases: count + 1][records][entry states]) is sized from the hint alone and
// leased per (device, HIP stream) from a cache of K2b's own (PartsScratch, ez_cache.h, which also reads
// the header's counters back: ez_breaks_parts_last).  Nothing in it is carried from call to call.
#include <hip/hip_runtime.h>

#include <atomic>

#include "ez_bytes.h"
#include "ez_cache.h"
#include "ez_internal.h"
#include "ez_k2_brk_parts.h"
#include "ez_k2_brk_walk.h"

namespace ez {
namespace {

struct Scratch {
    uint32_t *hdr, *base;
    KqRec *recs;
    KqEnt *ents;
    size_t bytes;
};
Scratch scratch_at(uint8_t *w, uint64_t count, uint64_t cap) {
    Scratch x;
    size_t o = (((size_t)kHWords + count + 1) * 4 + 15) / 16 * 16;
    x.hdr = (uint32_t *)w;
    x.base = x.hdr + kHWords;
    x.recs = (KqRec *)(w + o);
    o += (size_t)cap * sizeof(KqRec);
    x.ents = (KqEnt *)(w + o);
    o += (size_t)cap * sizeof(KqEnt);
    x.bytes = o;
    return x;
}

__device__ __forceinline__ KqSum sum_down(const KqSum &q, int d) {
    KqSum o;
    o.s.out = __shfl_down(q.s.out, d, kWave);
    o.s.out0 = __shfl_down(q.s.out0, d, kWave);
    o.s.maxd0 = (uint32_t)__shfl_down((int)q.s.maxd0, d, kWave);
    o.s.maxdz = (uint32_t)__shfl_down((int)q.s.maxdz, d, kWave);
    o.s.nreset = (uint32_t)__shfl_down((int)q.s.nreset, d, kWave);
    o.s.nlead = (uint32_t)__shfl_down((int)q.s.nlead, d, kWave);
    o.s.bslz = __shfl_down(q.s.bslz, d, kWave);
    o.s.fl = (uint32_t)__shfl_down((int)q.s.fl, d, kWave);
    o.nbrk = (uint32_t)__shfl_down((int)q.nbrk, d, kWave);
    return o;
}

// The part at ps of the stream b[0 .. nb) by the whole wave: its record for the chain that enters at
// the speculative position (valid in lane 0).
template <int C>
__device__ KqRec part_rec(uint8_t *stage, uint32_t (*bm)[C / 32 + 1], const uint8_t *b, uint32_t nb, uint32_t ps, int32_t lim32, int64_t limit) {
    const int lane = lane_id();
    const uint32_t sbase = kp_stage_base(ps, C);
    const KzWalk k = kz_walk<C>(stage, bm, b, nb, sbase, ps, false, 0);
    if (!k.settled) return kq_rec_unsettled();
    KqSum r = kq_sum<C>(KzWin{stage, sbase}, ps, lane, nb, k.a, k.x, lim32, limit);
    // the lanes in order, as a tree: after the step of width d, lane l (a multiple of 2 d) holds lanes l .. l + 2 d - 1
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const KqSum o = sum_down(r, d);
        if ((lane & (2 * d - 1)) == 0) kq_append(r, o);
    }
    return kq_rec(r, k.a, (uint32_t)__shfl((int)k.x, kWave - 1, kWave));
}

template <int C>
__global__ __launch_bounds__(64) void kq_first(BrkArgs A, uint32_t *hdr, const uint32_t *base, KqRec *recs) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[kp_stage_bytes(C)];
    __shared__ uint32_t bm[kZLanes][C / 32 + 1];
    if (hdr[kHGate] == 0) return;
    const uint32_t parts = hdr[kHParts];
    const int64_t limit = A.block_size_limit;
    const int32_t lim32 = k2_lim32(limit);
    uint32_t done = 0;
    for (uint32_t g = blockIdx.x; g < parts; g += gridDim.x) {
        const uint64_t s = kp_stream_of(base, A.count, g);
        const uint32_t nb = (uint32_t)(A.in_off[s + 1] - A.in_off[s]);  // (below 2^31: the stream has parts)
        const uint32_t ps = (g - base[s]) * kp_part_bytes(C);
        const KqRec r = part_rec<C>(stage, bm, A.in + A.in_off[s], nb, ps, lim32, limit);
        if (lane_id() == 0) recs[g] = r;
        done++;
    }
    if (lane_id() == 0 && done) atomicAdd(&hdr[kHFirst], done);
}

template <int C>
__global__ __launch_bounds__(64) void kq_order(BrkArgs A, uint32_t *hdr, const uint32_t *base, const KqRec *recs, KqEnt *ents) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[kp_stage_bytes(C)];
    __shared__ uint32_t bm[kZLanes][C / 32 + 1];
    if (hdr[kHGate] == 0) return;
    const int lane = lane_id();
    const int64_t limit = A.block_size_limit;
    const int32_t lim32 = k2_lim32(limit);
    constexpr uint32_t P = kp_part_bytes(C);
    uint32_t joined = 0, again = 0;
    for (uint64_t s = blockIdx.x; s < A.count; s += gridDim.x) {
        const uint32_t n = base[s + 1] - base[s];
        if (n == 0) continue;  // (the wave route's, launched behind this kernel)
        const uint32_t nb = (uint32_t)(A.in_off[s + 1] - A.in_off[s]);  // (below 2^31: the stream has parts)
        const uint8_t *b = A.in + A.in_off[s];
        const KqRec *rs = recs + base[s];
        KqEnt *es = ents + base[s];
        KqState S = kq_start();
        uint32_t j = 0;  // the next part to look at: every part before it has its entry state
        while (j < n) {
            if (S.st.stop || S.e >= nb) {  // the walk is over: the chain enters no later part
                for (uint32_t q = j + (uint32_t)lane; q < n; q += kWave) es[q] = kq_ent(S, false, false);
                break;
            }
            const uint32_t at = S.e / P;  // the next part the chain enters: the parts a token spans are not even loaded
            if (at > j) {
                const uint32_t to = at < n ? at : n;
                for (uint32_t q = j + (uint32_t)lane; q < to; q += kWave) es[q] = kq_ent(S, false, false);
                j = to;
                continue;
            }
            KqRec mine = kq_rec_unsettled();
            if (j + (uint32_t)lane < n) mine = rs[j + lane];
            const uint32_t m = n - j < (uint32_t)kWave ? n - j : (uint32_t)kWave;
            uint32_t k = 0;
            for (; k < m && !S.st.stop; k++) {
                const uint32_t ps = (j + k) * P;
                const uint32_t pe = nb - ps > P ? ps + P : nb;
                KqRec r;
                r.r.out = __shfl(mine.r.out, (int)k, kWave);
                r.r.out0 = __shfl(mine.r.out0, (int)k, kWave);
                r.r.ent = (uint32_t)__shfl((int)mine.r.ent, (int)k, kWave);
                r.r.exit = (uint32_t)__shfl((int)mine.r.exit, (int)k, kWave);
                r.r.maxd0 = (uint32_t)__shfl((int)mine.r.maxd0, (int)k, kWave);
                r.r.maxdz = (uint32_t)__shfl((int)mine.r.maxdz, (int)k, kWave);
                r.r.nreset = (uint32_t)__shfl((int)mine.r.nreset, (int)k, kWave);
                r.r.nlead = (uint32_t)__shfl((int)mine.r.nlead, (int)k, kWave);
                r.r.bslz = __shfl(mine.r.bslz, (int)k, kWave);
                r.r.fl = (uint32_t)__shfl((int)mine.r.fl, (int)k, kWave);
                r.nbrk = (uint32_t)__shfl((int)mine.nbrk, (int)k, kWave);
                const int cls = kq_class(S, pe, r);
                const KqState in = S;  // the part's entry state
                if (cls == kSAgain) {
                    const uint32_t x = kb_block<C, false>(stage, bm, b, nb, kp_stage_base(ps, C), ps, S.e, lim32, limit, S.st, [](uint32_t, uint64_t) {});
                    if (!S.st.stop) S.e = x;
                    again++;
                } else if (cls == kSJoin) {
                    kq_take(S, r);
                    joined++;
                }
                if (lane == 0) es[j + k] = kq_ent(in, cls != kSPass, S.st.nbrk != in.st.nbrk);
            }
            j += k;
        }
        if (lane == 0) {  // (k2b_walk's count pass ends so)
            const bool ok = kb_end_ok(S.st, S.e, nb);
            A.handed[s] = ok ? 0u : 1u;
            if (ok) {
                A.out_size[s] = S.st.total;
                if (A.status) A.status[s] = EZ_OK;
                A.brk_idx[s] = S.st.nbrk;
            } else {
                A.brk_idx[s] = 0;
                const uint32_t at = atomicAdd(&A.list[0], 1u);
                A.list[1 + at] = (uint32_t)s;
            }
        }
    }
    if (lane == 0) {
        if (joined) atomicAdd(&hdr[kHJoined], joined);
        if (again) atomicAdd(&hdr[kHAgain], again);
    }
}

template <int C>
__global__ __launch_bounds__(64) void kq_fill(BrkArgs A, uint32_t *hdr, const uint32_t *base, const KqEnt *ents) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[kp_stage_bytes(C)];
    __shared__ uint32_t bm[kZLanes][C / 32 + 1];
    if (hdr[kHGate] == 0 || A.brk_total[0] == 0) return;  // (no Break, or more than brk_cap: nothing to write)
    const uint32_t parts = hdr[kHParts];
    const int64_t limit = A.block_size_limit;
    const int32_t lim32 = k2_lim32(limit);
    uint32_t filled = 0;
    for (uint32_t g = blockIdx.x; g < parts; g += gridDim.x) {
        const KqEnt n = ents[g];
        if (!kq_fills(n)) continue;
        const uint64_t s = kp_stream_of(base, A.count, g);
        if (A.handed[s]) continue;  // (the exact decoder fills the listed streams)
        const uint64_t i0 = A.in_off[s];
        const uint32_t nb = (uint32_t)(A.in_off[s + 1] - i0);
        const uint32_t ps = (g - base[s]) * kp_part_bytes(C);
        const uint64_t g0 = A.brk_idx[s], nbrk = A.brk_idx[s + 1] - g0;
        KqState S = kq_from(n);
        (void)kb_block<C, true>(stage, bm, A.in + i0, nb, kp_stage_base(ps, C), ps, S.e, lim32, limit, S.st, [&](uint32_t k, uint64_t out) {
            if (k < nbrk) A.brk_pos[g0 + k] = out;
        });
        filled++;
    }
    if (lane_id() == 0 && filled) atomicAdd(&hdr[kHFilled], filled);
}

PartsScratch &scratch() {
    static PartsScratch *x = new PartsScratch();
    return *x;
}

std::atomic<int> g_route{0};  // 0: automatic; 'p', 'v'

template <int C>
hipError_t launch_front(const BrkArgs &a, const Scratch &x, uint64_t cap, hipStream_t st) {
    const hipError_t e = launch_parts_layout(C, a.in, a.in_off, a.count, a.in_bytes, x.hdr, x.base, nullptr, cap, 0, st);
    if (e != hipSuccess) return e;
    // the chip's LDS holds two such blocks per CU at chunk 1,024; the parts beyond go round the grid
    hipLaunchKernelGGL(kq_first<C>, dim3((unsigned)(cap < 2048 ? cap : 2048)), dim3(64), 0, st, a, x.hdr, x.base, x.recs);
    hipLaunchKernelGGL(kq_order<C>, dim3((unsigned)(a.count < 2048 ? a.count : 2048)), dim3(64), 0, st, a, x.hdr, x.base, x.recs, x.ents);
    return hipGetLastError();
}

}  // namespace

DevCache &breaks_parts_cache() { return scratch().cache; }

void select_breaks_route(int v) { g_route = v; }
int selected_breaks_route() { return g_route; }

void breaks_parts_none() { scratch().none(); }

// The parts route's chunk for a Break query, 0: the wave route, which takes every batch whose caller
// did not give its input bytes, an empty one, one of more than 2^20 streams, and all of them under
// ez_select_breaks_route('v').
// Forced (ez_select_breaks_route('p')): at any length, 1,024 where the wave route takes 1,024, else 256.
// Automatic: the wave route.  The candidate rule is K2g's (segs_parts_route: up to 64 streams whose
// longest is 480 KiB or more, chunk 1,024), but no K2b figure stands behind it yet
// (tools/breaks_bench.py --route --forced is the measurement), so the route ships
// forced-only.
int breaks_parts_route(uint64_t max_len, uint64_t count, uint64_t in_bytes) {
    const int sel = selected_breaks_route();
    if (count == 0 || in_bytes == 0 || count > (1u << 20) || sel == 'v') return 0;
    if (sel == 'p') return size_chunk(max_len) == 1024 ? 1024 : 256;
    return 0;
}

hipError_t launch_breaks_parts(BrkArgs &a, int chunk, hipStream_t st, CacheLease &lease, void **pws, uint64_t *pws_cap) {
    const uint64_t cap = parts_cap(a.in_bytes, kp_part_bytes((uint32_t)chunk), a.count);
    if (cap == 0) return hipErrorOutOfMemory;
    uint8_t *w = nullptr;
    const hipError_t e = scratch().acquire(nullptr, 0, scratch_at(nullptr, a.count, cap).bytes, st, lease, &w);
    if (e != hipSuccess) return e;
    const Scratch x = scratch_at(w, a.count, cap);
    a.parts_gate = x.hdr + kHGate;
    a.parts_base = x.base;
    *pws = w;
    *pws_cap = cap;
    return chunk == 1024 ? launch_front<1024>(a, x, cap, st) : launch_front<256>(a, x, cap, st);
}

hipError_t launch_breaks_parts_fill(const BrkArgs &a, int chunk, void *pws, uint64_t pws_cap, hipStream_t st) {
    const Scratch x = scratch_at((uint8_t *)pws, a.count, pws_cap);
    const unsigned grid = (unsigned)(pws_cap < 2048 ? pws_cap : 2048);
    if (chunk == 1024) hipLaunchKernelGGL(kq_fill<1024>, dim3(grid), dim3(64), 0, st, a, x.hdr, x.base, x.ents);
    else hipLaunchKernelGGL(kq_fill<256>, dim3(grid), dim3(64), 0, st, a, x.hdr, x.base, x.ents);
    return hipGetLastError();
}

// of the last query: parts walked in the first pass, records taken as they stood, parts walked again,
// parts the fill pass wrote (zeros where the route did not run); the caller has synchronised the
// query's stream
hipError_t breaks_parts_last(uint64_t counts[4]) {
    uint32_t h[kHWords];
    const hipError_t e = scratch().last(h);
    counts[0] = h[kHFirst];
    counts[1] = h[kHJoined];
    counts[2] = h[kHAgain];
    counts[3] = h[kHFilled];
    return e;
}

}  // namespace ez
