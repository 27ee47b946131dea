// ez_decompress_parts.hip — K2z's parts route: every stream's token chain cut over many waves, for
// the few long streams that the wave route (ez_decompress_size.hip) gives one wave each.
//
// The steps are ez_k2_parts.h's.  Three kernels on the caller's stream:
//   kp_layout checks the caller's in_bytes hint against the real extent and lays the streams' parts
//             out (ez_k2_layout.h's steps: an exclusive scan of every stream's part count; on the
//             automatic route a stream that starts with tokens over half of it gets none,
//             kp_probe_wave); on a mismatch it leaves the gate closed: the next two kernels do
//             nothing.  The wave route, launched behind them with the gate and the layout as
//             arguments, sizes every stream if the gate is closed, else the streams without parts.
//             K2g's parts route (ez_decompress_segs_parts.hip) lays its parts out with the same
//             kernel (launch_parts_layout);
//   kp_first  a wave per part, grid-stride: kz_walk (ez_k2_walk.h) over the part with the warm-up chunk
//             before it, then sum, reduce, and write the part's record;
//   kp_order  a wave per stream: follows the true chain through the records, 64 of them per load,
//             walks again the parts whose record starts elsewhere, and ends as the wave route does:
//             out_size[s] and EZ_OK, or the stream on the slow list for the exact decoder run dry.
// The scratch ([header][part bases: count + 1][records]) is sized from the hint alone, so the call
// never waits for the stream; it is the caller's own or leased from a cache per (device, HIP stream)
// (PartsScratch, ez_cache.h, which also reads the header's counters back after the call).
#include <hip/hip_runtime.h>

#include <atomic>

#include "ez_bytes.h"
#include "ez_cache.h"
#include "ez_internal.h"
#include "ez_k2_parts.h"
#include "ez_k2_walk.h"

namespace ez {
namespace {

// The one layout kernel of the parts routes, from ez_k2_layout.h's steps: every stream's part count (none
// for a stream the probe leaves to the wave route), the gate, and the counts' exclusive scan in base;
// listed (the size query's stage of K2g's route, may be null): a flag per stream, cleared here
template <int C>
__global__ __launch_bounds__(kLayoutThreads) void kp_layout(const uint8_t *in, const uint64_t *in_off, uint64_t count, uint64_t in_bytes, uint32_t *hdr,
                                                            uint32_t *base, uint32_t *listed, uint64_t cap, int probe) {
    __shared__ uint64_t sums[kLayoutThreads];
    const int t = (int)threadIdx.x;
    const LayoutRange r = layout_range(count, kLayoutThreads, t);
    uint64_t n = 0;
    for (uint64_t s = r.lo; s < r.hi; s++) {
        const uint64_t nb64 = in_off[s + 1] - in_off[s];
        uint32_t parts = kp_parts_of(nb64, C);
        if (probe && parts) {
            const uint8_t *b = in + in_off[s];
            const uint32_t nb = (uint32_t)nb64;
            if (kp_probe_wave(kz_global_at(b, nb), nb)) parts = 0;
        }
        base[s] = parts;
        if (listed) listed[s] = 0;
        n += parts;
    }
    sums[t] = n;
    __syncthreads();
    // the records are sized from the hint: nothing indexes them unless the real extent is within it
    if (t == 0) (void)layout_gate(sums, kLayoutThreads, in_off, count, in_bytes, cap, hdr, base);
    __syncthreads();
    layout_scan(base, r, sums[t]);
}

// One part of the stream b[0 .. nb) at ps, by the whole wave: its record for the chain that enters at
// the speculative position (known false: the first pass) or at the true one e (the in-order pass).
template <int C>
__device__ KpRec part_walk(uint8_t *stage, uint32_t (*bm)[C / 32 + 1], const uint8_t *b, uint32_t nb, uint32_t ps, bool known, uint32_t e,
                           int32_t lim32, int64_t limit) {
    const int lane = lane_id();
    const uint32_t sbase = kp_stage_base(ps, C);
    const KzWalk k = kz_walk<C>(stage, bm, b, nb, sbase, ps, known, e);
    KpRec rec{0, kPNoEntry, 0, 0, 0};
    if (!k.settled) return rec;
    const KzSum r = kz_sum<C>(KzWin{stage, sbase}, ps, lane, nb, k.a, k.x, lim32, limit);
    const uint64_t io = wscan_add_u64(r.out);
    // (kp_append over the lanes in order)
    const bool bad = wballot((r.fl & kZBad) != 0) != 0;
    const uint64_t rm = wballot((r.fl & kZReset) != 0);
    const bool late = wballot((r.fl & kZReset) && ((r.fl & kZResetLate) || io != r.out)) != 0;
    rec.out = __shfl(io, kWave - 1, kWave);
    rec.ent = (uint32_t)__shfl((int)k.a, 0, kWave);
    rec.exit = (uint32_t)__shfl((int)k.x, kWave - 1, kWave);
    rec.maxd = wmax_u32(r.maxd);
    rec.fl = bad ? kZBad : 0u;
    if (rm) rec.fl |= kZReset | (late ? kZResetLate : 0u) | ((uint32_t)__shfl((int)r.fl, 63 - __builtin_clzll(rm), kWave) & 0xff00u);
    return rec;
}

template <int C>
__global__ __launch_bounds__(64) void kp_first(DecompressArgs A, uint32_t *hdr, const uint32_t *base, KpRec *recs) {
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
        const KpRec r = part_walk<C>(stage, bm, A.in + A.in_off[s], nb, ps, false, 0, lim32, limit);
        if (lane_id() == 0) recs[g] = r;
        done++;
    }
    if (lane_id() == 0 && done) atomicAdd(&hdr[kHFirst], done);
}

template <int C>
__global__ __launch_bounds__(64) void kp_order(DecompressArgs A, uint32_t *hdr, const uint32_t *base, const KpRec *recs) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[kp_stage_bytes(C)];
    __shared__ uint32_t bm[kZLanes][C / 32 + 1];
    if (hdr[kHGate] == 0) return;
    const int lane = lane_id();
    const int64_t limit = A.block_size_limit;
    const int32_t lim32 = k2_lim32(limit);
    uint32_t joined = 0, walked = 0;
    for (uint64_t s = blockIdx.x; s < A.count; s += gridDim.x) {
        const uint64_t nb64 = A.in_off[s + 1] - A.in_off[s];
        const uint8_t *b = A.in + A.in_off[s];
        KpState S = kp_start(nb64);
        const uint32_t nb = S.bad ? 0u : (uint32_t)nb64;
        const uint32_t n = base[s + 1] - base[s];
        if (n == 0) continue;  // (the wave route's, launched behind this kernel)
        const KpRec *rs = recs + base[s];
        uint32_t j = 0;
        while (!S.bad && j < n) {
            KpRec mine{0, kPNoEntry, 0, 0, 0};
            if (j + (uint32_t)lane < n) mine = rs[j + lane];
            const uint32_t m = n - j < (uint32_t)kWave ? n - j : (uint32_t)kWave;
            for (uint32_t k = 0; k < m && !S.bad; k++) {
                const uint32_t ps = (j + k) * kp_part_bytes(C);
                const uint32_t pe = nb - ps > kp_part_bytes(C) ? ps + kp_part_bytes(C) : nb;
                KpRec r;
                r.out = __shfl(mine.out, (int)k, kWave);
                r.ent = (uint32_t)__shfl((int)mine.ent, (int)k, kWave);
                r.exit = (uint32_t)__shfl((int)mine.exit, (int)k, kWave);
                r.maxd = (uint32_t)__shfl((int)mine.maxd, (int)k, kWave);
                r.fl = (uint32_t)__shfl((int)mine.fl, (int)k, kWave);
                const int cls = kp_class(S, pe, r);
                if (cls == kPPass) continue;
                if (cls == kPWalk) {
                    r = part_walk<C>(stage, bm, b, nb, ps, true, S.e, lim32, limit);
                    walked++;
                } else {
                    joined++;
                }
                kp_take(S, r);
            }
            // the next part the chain can enter: the parts a token spans are not even loaded
            j += m;
            const uint32_t at = S.e / kp_part_bytes(C);
            j = at > j ? at : j;
        }
        const bool ok = kp_end_ok(S, nb);
        if (lane == 0) {
            if (!ok) {
                slow_append(A, s);
            } else {
                A.out_size[s] = S.total;
                if (A.status) A.status[s] = EZ_OK;
            }
        }
    }
    if (lane == 0) {
        if (joined) atomicAdd(&hdr[kHJoined], joined);
        if (walked) atomicAdd(&hdr[kHAgain], walked);
    }
}

// the scratch: [header][part bases: count + 1][records: cap]
size_t recs_at(uint64_t count) { return (((size_t)kHWords + count + 1) * 4 + 15) / 16 * 16; }

template <int C>
hipError_t launch_parts(const DecompressArgs &a, uint8_t *w, uint64_t cap, int probe, hipStream_t st) {
    uint32_t *hdr = (uint32_t *)w;
    uint32_t *base = hdr + kHWords;
    KpRec *recs = (KpRec *)(w + recs_at(a.count));
    const hipError_t e = launch_parts_layout(C, a.in, a.in_off, a.count, a.in_bytes, hdr, base, nullptr, cap, probe, st);
    if (e != hipSuccess) return e;
    // the chip's LDS holds two such blocks per CU; the parts beyond go round the grid
    hipLaunchKernelGGL(kp_first<C>, dim3((unsigned)(cap < 2048 ? cap : 2048)), dim3(64), 0, st, a, hdr, base, recs);
    hipLaunchKernelGGL(kp_order<C>, dim3((unsigned)(a.count < 2048 ? a.count : 2048)), dim3(64), 0, st, a, hdr, base, recs);
    return hipGetLastError();
}

PartsScratch &scratch() {
    static PartsScratch *x = new PartsScratch();
    return *x;
}

}  // namespace

hipError_t launch_parts_layout(int chunk, const uint8_t *in, const uint64_t *in_off, uint64_t count, uint64_t in_bytes, uint32_t *hdr, uint32_t *base,
                               uint32_t *listed, uint64_t cap, int probe, hipStream_t st) {
    const hipError_t e = hipMemsetAsync(hdr, 0, kHWords * 4, st);
    if (e != hipSuccess) return e;
    if (chunk == 1024) hipLaunchKernelGGL(kp_layout<1024>, dim3(1), dim3(kLayoutThreads), 0, st, in, in_off, count, in_bytes, hdr, base, listed, cap, probe);
    else hipLaunchKernelGGL(kp_layout<256>, dim3(1), dim3(kLayoutThreads), 0, st, in, in_off, count, in_bytes, hdr, base, listed, cap, probe);
    return hipGetLastError();
}

DevCache &size_cache() { return scratch().cache; }

static std::atomic<int> g_size_route{0};  // 0: automatic; 'p', 'v'
void select_size_route(int v) { g_size_route = v; }
int selected_size_route() { return g_size_route; }

void size_parts_none() { scratch().none(); }

// bytes of scratch the route needs for a batch (either chunk size; 0: more parts than the route takes):
// a synchronous caller that owns its scratch (a Reader handle) sizes it with this and passes it as
// DecompressArgs.jws / jws_cap
uint64_t size_parts_workspace_bytes(uint64_t count, uint64_t in_bytes) {
    const uint64_t cap = parts_cap(in_bytes, kp_part_bytes(256), count);
    return cap ? recs_at(count) + cap * sizeof(KpRec) : 0;
}

hipError_t launch_size_parts(const DecompressArgs &a, int chunk, bool probe, hipStream_t st, CacheLease &lease, const uint32_t **gate,
                             const uint32_t **base) {
    const uint64_t cap = parts_cap(a.in_bytes, kp_part_bytes((uint32_t)chunk), a.count);
    if (cap == 0) return hipErrorOutOfMemory;
    uint8_t *w = nullptr;
    const hipError_t e = scratch().acquire(a.jws, a.jws_cap, recs_at(a.count) + (size_t)cap * sizeof(KpRec), st, lease, &w);
    if (e != hipSuccess) return e;
    *gate = (const uint32_t *)w + kHGate;
    *base = (const uint32_t *)w + kHWords;
    return chunk == 1024 ? launch_parts<1024>(a, w, cap, probe, st) : launch_parts<256>(a, w, cap, probe, st);
}

// of the last query: parts launched, parts whose record the true chain took, parts walked again
// (zeros where the parts route did not run); the caller has synchronised the query's stream
hipError_t size_parts_last(uint64_t counts[3]) {
    uint32_t h[kHWords];
    const hipError_t e = scratch().last(h);
    counts[0] = h[kHFirst];
    counts[1] = h[kHJoined];
    counts[2] = h[kHAgain];
    return e;
}

}  // namespace ez
