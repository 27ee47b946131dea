// ez_decompress_segs_parts.hip — K2g's parts route: the segment query of long concatenated streams cut
// over many waves, for the few long streams that the wave route (k2g_walk, ez_decompress_segs.hip)
// gives one wave each.
//
// The steps are ez_k2_segs_parts.h's, over K2z's part grid (ez_k2_parts.h).  Kernels on the caller's
// stream, which never wait for it:
//   kp_layout (ez_decompress_parts.hip's, through launch_parts_layout; the steps are ez_k2_layout.h's)
//             checks the caller's in_bytes hint against the real extent and lays the streams' parts
//             out (an exclusive scan of every stream's part count); on a mismatch it leaves the gate
//             closed: the kernels of this file do nothing, and k2g_walk, launched behind them
//             with the gate and the layout in its arguments, walks every stream, else only the
//             streams without parts (empty, 2 GiB or more);
//   ks_first  a wave per part, grid-stride: kz_walk (ez_k2_walk.h) over the part with the warm-up chunk
//             before it, ks_sum per lane, the lanes' sums joined as a tree (ks_append), the record;
//   ks_order  a wave per stream, 64 records per load: follows the true chain through the records
//             (ks_class, ks_take), walks again from the true state the parts whose record starts
//             elsewhere or is marked kSWalk (ks_block: kg_sum and kg_cuts, as kg_stream runs a
//             super-block), leaves every part's entry state and seg_idx[s] = the stream's segments;
//   (k2g_scan and k2g_heads, ez_decompress_segs.hip: the layout, each stream's first segment)
//   ks_fill   a wave per part whose record holds a Reset and whose entry state is live: ks_block
//             from the entry state, which writes the part's cuts in place.  Nothing is walked twice by
//             one wave for a stream of many cuts: the fill is parallel.
// The size query's stage (launch_size_segs) runs kp_layout (which clears a flag per stream), ks_mark (sets
// the flag of every stream of the fast kernels' list), ks_first and ks_order over the listed streams
// that have parts: the order pass then ends as k2g_size does, and there is no fill.
// The scratch ([header][part bases: count + 1][listed: count][records][entry states]) is sized from the hint alone.
// A direct query leases it per (device, HIP stream) from a cache (PartsScratch, ez_cache.h, which also reads
// the header's counters back); the segmented decode carves it out of its own lease and passes it down
// (SegsArgs.pws).  Nothing in it is carried from call to call.
#include <hip/hip_runtime.h>

#include <atomic>

#include "ez_bytes.h"
#include "ez_cache.h"
#include "ez_internal.h"
#include "ez_k2_segs_parts.h"
#include "ez_k2_walk.h"

namespace ez {
namespace {

struct Scratch {
    uint32_t *hdr, *base, *listed;
    KsRec *recs;
    KsEnt *ents;
    size_t bytes;
};
Scratch scratch_at(uint8_t *w, uint64_t count, uint64_t cap) {
    Scratch x;
    size_t o = (((size_t)kHWords + 2 * count + 1) * 4 + 15) / 16 * 16;
    x.hdr = (uint32_t *)w;
    x.base = x.hdr + kHWords;
    x.listed = x.base + count + 1;  // (the size query's stage: the streams of the fast kernels' list)
    x.recs = (KsRec *)(w + o);
    o += (size_t)cap * sizeof(KsRec);
    x.ents = (KsEnt *)(w + o);
    o += (size_t)cap * sizeof(KsEnt);
    x.bytes = o;
    return x;
}

__device__ __forceinline__ KsSum sum_down(const KsSum &r, int d) {
    KsSum o;
    o.out = __shfl_down(r.out, d, kWave);
    o.out0 = __shfl_down(r.out0, d, kWave);
    o.maxd0 = (uint32_t)__shfl_down((int)r.maxd0, d, kWave);
    o.maxdz = (uint32_t)__shfl_down((int)r.maxdz, d, kWave);
    o.nreset = (uint32_t)__shfl_down((int)r.nreset, d, kWave);
    o.nlead = (uint32_t)__shfl_down((int)r.nlead, d, kWave);
    o.bslz = __shfl_down(r.bslz, d, kWave);
    o.fl = (uint32_t)__shfl_down((int)r.fl, d, kWave);
    return o;
}

// The part at ps of the stream b[0 .. nb) by the whole wave: its record for the chain that enters at
// the speculative position (valid in lane 0).
template <int C>
__device__ KsRec part_rec(uint8_t *stage, uint32_t (*bm)[C / 32 + 1], const uint8_t *b, uint32_t nb, uint32_t ps, int32_t lim32, int64_t limit) {
    const int lane = lane_id();
    const uint32_t sbase = kp_stage_base(ps, C);
    const KzWalk k = kz_walk<C>(stage, bm, b, nb, sbase, ps, false, 0);
    if (!k.settled) return ks_rec_unsettled();
    KsSum r = ks_sum<C>(KzWin{stage, sbase}, ps, lane, nb, k.a, k.x, lim32, limit);
    // the lanes in order, as a tree: after the step of width d, lane l (a multiple of 2 d) holds lanes l .. l + 2 d - 1
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const KsSum o = sum_down(r, d);
        if ((lane & (2 * d - 1)) == 0) ks_append(r, o);
    }
    return ks_rec(r, k.a, (uint32_t)__shfl((int)k.x, kWave - 1, kWave));
}

// The part at ps from the true chain's position e in it, with the state (wave-uniform), as kg_stream
// runs a super-block: kg_sum, the in-order prefix, the events in lane order through kg_cuts, which calls
// cut(i, pos, out) on every lane for the stream's cut i.  Returns where the chain leaves the part.
template <int C, class Cut>
__device__ __forceinline__ uint32_t ks_block(uint8_t *stage, uint32_t (*bm)[C / 32 + 1], const uint8_t *b, uint32_t nb, uint32_t ps, uint32_t e,
                                             int32_t lim32, int64_t limit, KgState &st, Cut cut) {
    const int lane = lane_id();
    const uint32_t sbase = kp_stage_base(ps, C);
    const KzWalk k = kz_walk<C>(stage, bm, b, nb, sbase, ps, true, e);
    if (!k.settled) {
        st.stop = true;
        return e;
    }
    const KzWin w{stage, sbase};
    const KgSum r = kg_sum<C>(w, ps, lane, nb, k.a, k.x, lim32, limit);
    const uint64_t io = wscan_add_u64(r.out);
    uint64_t ev = wballot(r.fl != 0);
    uint64_t base = 0;  // the prefix taken into the state so far
    int from = 0;       // the first lane whose distances are not in the state yet
    while (ev) {
        const int j = ffs64(ev);
        ev &= ev - 1;
        const uint64_t ioj = __shfl(io, j, kWave);
        st.total += ioj - base;
        base = ioj;
        st.maxd = max(st.maxd, wmax_u32(lane >= from && lane <= j ? r.maxd : 0u));
        from = j + 1;
        kg_cuts<C>(w, ps, j, nb, (uint32_t)__shfl((int)r.epos, j, kWave), (uint32_t)__shfl((int)k.x, j, kWave), lim32, limit, st, cut);
        if (st.stop) return e;
    }
    st.total += __shfl(io, kWave - 1, kWave) - base;
    st.maxd = max(st.maxd, wmax_u32(lane >= from ? r.maxd : 0u));
    return (uint32_t)__shfl((int)k.x, kWave - 1, kWave);
}

template <int C>
__global__ __launch_bounds__(64) void ks_first(SegsArgs A, uint32_t *hdr, const uint32_t *base, const uint32_t *listed, KsRec *recs) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[kp_stage_bytes(C)];
    __shared__ uint32_t bm[kZLanes][C / 32 + 1];
    if (hdr[kHGate] == 0) return;
    const uint32_t parts = hdr[kHParts];
    const int64_t limit = A.block_size_limit;
    const int32_t lim32 = k2_lim32(limit);
    uint32_t done = 0;
    for (uint32_t g = blockIdx.x; g < parts; g += gridDim.x) {
        const uint64_t s = kp_stream_of(base, A.count, g);
        if (listed && !listed[s]) continue;  // (the size query's stage: only the streams handed over)
        const uint32_t nb = (uint32_t)(A.in_off[s + 1] - A.in_off[s]);  // (below 2^31: the stream has parts)
        const uint32_t ps = (g - base[s]) * kp_part_bytes(C);
        const KsRec r = part_rec<C>(stage, bm, A.in + A.in_off[s], nb, ps, lim32, limit);
        if (lane_id() == 0) recs[g] = r;
        done++;
    }
    if (lane_id() == 0 && done) atomicAdd(&hdr[kHFirst], done);
}

// The size query's stage (launch_size_segs_parts): the fast kernels' list, and where the results go:
// out_size[s] and EZ_OK, or the stream on the second list (ctr: size_segs_counters')
struct KsSize {
    const uint32_t *first;
    uint64_t *out_size;
    int32_t *status;
    uint32_t *ctr;
};
__global__ void ks_mark(KsSize Z, uint64_t count, const uint32_t *hdr, uint32_t *listed) {
    if (hdr[kHGate] == 0) return;
    const uint64_t n = Z.first[0] < count ? Z.first[0] : count;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x) listed[Z.first[1 + k]] = 1;
}

// SIZE: the size query's stage over the listed streams, which ends as k2g_size does and leaves no
// entry states; else the segment query's count
template <int C, bool SIZE>
__global__ __launch_bounds__(64) void ks_order(SegsArgs A, uint32_t *hdr, const uint32_t *base, const KsRec *recs, KsEnt *ents, const uint32_t *listed,
                                               KsSize Z) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[kp_stage_bytes(C)];
    __shared__ uint32_t bm[kZLanes][C / 32 + 1];
    if (hdr[kHGate] == 0) return;
    const int lane = lane_id();
    const int64_t limit = A.block_size_limit;
    const int32_t lim32 = k2_lim32(limit);
    constexpr uint32_t P = kp_part_bytes(C);
    uint32_t joined = 0, again = 0, sized = 0;
    for (uint64_t s = blockIdx.x; s < A.count; s += gridDim.x) {
        const uint32_t n = base[s + 1] - base[s];
        if (n == 0) continue;  // (the wave route's, launched behind this kernel)
        if (SIZE && !listed[s]) continue;
        const uint32_t nb = (uint32_t)(A.in_off[s + 1] - A.in_off[s]);  // (below 2^31: the stream has parts)
        const uint8_t *b = A.in + A.in_off[s];
        const KsRec *rs = recs + base[s];
        KsEnt *es = ents + base[s];
        KsState S = ks_start();
        uint32_t j = 0;  // the next part to look at: every part before it has its entry state
        while (j < n) {
            if (S.st.stop || S.e >= nb) {  // the walk is over: the chain enters no later part
                if (!SIZE)
                    for (uint32_t q = j + (uint32_t)lane; q < n; q += kWave) es[q] = ks_ent(S, false);
                break;
            }
            const uint32_t at = S.e / P;  // the next part the chain enters: the parts a token spans are not even loaded
            if (at > j) {
                const uint32_t to = at < n ? at : n;
                if (!SIZE)
                    for (uint32_t q = j + (uint32_t)lane; q < to; q += kWave) es[q] = ks_ent(S, false);
                j = to;
                continue;
            }
            KsRec mine = ks_rec_unsettled();
            if (j + (uint32_t)lane < n) mine = rs[j + lane];
            const uint32_t m = n - j < (uint32_t)kWave ? n - j : (uint32_t)kWave;
            uint32_t k = 0;
            for (; k < m && !S.st.stop; k++) {
                const uint32_t ps = (j + k) * P;
                const uint32_t pe = nb - ps > P ? ps + P : nb;
                KsRec r;
                r.out = __shfl(mine.out, (int)k, kWave);
                r.out0 = __shfl(mine.out0, (int)k, kWave);
                r.ent = (uint32_t)__shfl((int)mine.ent, (int)k, kWave);
                r.exit = (uint32_t)__shfl((int)mine.exit, (int)k, kWave);
                r.maxd0 = (uint32_t)__shfl((int)mine.maxd0, (int)k, kWave);
                r.maxdz = (uint32_t)__shfl((int)mine.maxdz, (int)k, kWave);
                r.nreset = (uint32_t)__shfl((int)mine.nreset, (int)k, kWave);
                r.nlead = (uint32_t)__shfl((int)mine.nlead, (int)k, kWave);
                r.bslz = __shfl(mine.bslz, (int)k, kWave);
                r.fl = (uint32_t)__shfl((int)mine.fl, (int)k, kWave);
                const int cls = ks_class(S, pe, r);
                if (!SIZE && lane == 0) es[j + k] = ks_ent(S, cls != kSPass);
                if (cls == kSPass) continue;
                if (cls == kSAgain) {
                    const uint32_t x = ks_block<C>(stage, bm, b, nb, ps, S.e, lim32, limit, S.st, [](uint32_t, uint32_t, uint64_t) {});
                    if (!S.st.stop) S.e = x;
                    again++;
                } else {
                    ks_take(S, r);
                    joined++;
                }
            }
            j += k;
        }
        if (!SIZE) {
            if (lane == 0) A.seg_idx[s] = (uint64_t)S.st.ncut + 1;
        } else if (lane == 0) {
            if (kg_end_ok(S.st, S.e, nb)) {
                Z.out_size[s] = S.st.total;
                if (Z.status) Z.status[s] = EZ_OK;
                sized++;
            } else {
                const uint32_t at = atomicAdd(&Z.ctr[2], 1u);
                Z.ctr[3 + at] = (uint32_t)s;
            }
        }
    }
    if (lane == 0) {
        if (SIZE && sized) atomicAdd(&Z.ctr[1], sized);
        if (joined) atomicAdd(&hdr[kHJoined], joined);
        if (again) atomicAdd(&hdr[kHAgain], again);
    }
}

template <int C>
__global__ __launch_bounds__(64) void ks_fill(SegsArgs A, uint32_t *hdr, const uint32_t *base, const KsRec *recs, const KsEnt *ents) {
    __shared__ __attribute__((aligned(16))) uint8_t stage[kp_stage_bytes(C)];
    __shared__ uint32_t bm[kZLanes][C / 32 + 1];
    if (hdr[kHGate] == 0 || A.hdr[0]) return;  // (the one-segment-per-stream layout: no cuts to write)
    const uint32_t parts = hdr[kHParts];
    const int lane = lane_id();
    const int64_t limit = A.block_size_limit;
    const int32_t lim32 = k2_lim32(limit);
    uint32_t filled = 0;
    for (uint32_t g = blockIdx.x; g < parts; g += gridDim.x) {
        const KsRec r = recs[g];
        const KsEnt n = ents[g];
        if (!ks_fills(r, n)) continue;
        const uint64_t s = kp_stream_of(base, A.count, g);
        const uint64_t i0 = A.in_off[s];
        const uint32_t nb = (uint32_t)(A.in_off[s + 1] - i0);
        const uint32_t ps = (g - base[s]) * kp_part_bytes(C);
        const uint64_t g0 = A.seg_idx[s], nseg = A.seg_idx[s + 1] - g0;
        const uint64_t o0 = A.out_off[s], o1 = A.out_off[s + 1];
        auto cut = [&](uint32_t i, uint32_t pos, uint64_t out) {
            if (lane != 0 || (uint64_t)i + 1 >= nseg) return;
            A.seg_in[g0 + 1 + i] = i0 + pos;
            A.seg_out[g0 + 1 + i] = ks_slot(o0, o1, out);
        };
        KsState S = ks_from(n);
        (void)ks_block<C>(stage, bm, A.in + i0, nb, ps, S.e, lim32, limit, S.st, cut);
        if (S.st.ncut != n.ncut) filled++;
    }
    if (lane == 0 && filled) atomicAdd(&hdr[kHFilled], filled);
}

PartsScratch &scratch() {
    static PartsScratch *x = new PartsScratch();
    return *x;
}

std::atomic<int> g_route{0};  // 0: automatic; 'p', 'v'

}  // namespace

DevCache &segs_parts_cache() { return scratch().cache; }

void select_segments_route(int v) { g_route = v; }
int selected_segments_route() { return g_route; }

void segs_parts_none() { scratch().none(); }

// The parts route's chunk for a segment query, 0: the wave route, which takes every batch whose caller
// did not give its input bytes, an empty one, one of more than 2^20 streams, and all of them under
// ez_select_segments_route('v').
// Forced (ez_select_segments_route('p')): at any length, 1,024 where the wave route takes 1,024, else
// 256.  Automatic, only where it measured faster than a wave per stream (tools/segments_bench.py --route
// --forced, profiles/r08_segments_parts.txt; 64 KiB frames of log data, the query alone,
// median ms, wave / parts 256 / parts 1,024):
//   up to 64 streams whose longest is 480 KiB or more, chunk 1,024 (64 x 2.0 MB 25.9 / 6.56 / 4.55;
//     8 x 2.0 MB 25.6 / 5.29 / 1.71; a lone 16.1 MB stream 199 / 33.1 / 1.65; 64 x 0.5 MB 3.96 / 2.14 /
//     1.35; 8 x 0.5 MB 3.95 / 2.04 / 0.92; a lone 0.5 MB stream 3.73 / 1.08 / 0.92: chunk 256 leaves a
//     quarter of the parts to the one wave per stream that walks them again, 2,231 of 7,873 on 64 x 2.0 MB
//     against 35 of 1,984).
// More streams keep a wave each, which fills the chip: the first pass holds two blocks per CU and
// moves about 30 GB/s (1,024 x 0.5 MB 4.45 / 6.75 / 14.9; 4,096 x 126 KB 2.48 / 6.23 / 14.7).  Between
// them 256 x 2.0 MB measured 26.8 / 10.3 / 14.2: left on the wave route until shorter streams are
// measured at that count.
// Without a max_len hint (the segmented decode's query) the batch's mean length stands in, which is
// at most the longest.
int segs_parts_route(uint64_t max_len, uint64_t count, uint64_t in_bytes) {
    const int sel = selected_segments_route();
    if (count == 0 || in_bytes == 0 || count > (1u << 20) || sel == 'v') return 0;
    if (sel == 'p') return size_chunk(max_len) == 1024 ? 1024 : 256;
    if (max_len == 0) max_len = in_bytes / count;
    return count <= 64 && max_len >= (480u << 10) ? 1024 : 0;
}

// bytes of scratch the route needs for a batch (either chunk size; 0: more parts than the route takes)
uint64_t segs_parts_workspace_bytes(uint64_t count, uint64_t in_bytes) {
    const uint64_t cap = parts_cap(in_bytes, kp_part_bytes(256), count);
    return cap ? scratch_at(nullptr, count, cap).bytes : 0;
}

// The passes in front of the wave route's kernels: the layout, a wave per part, a wave per stream.  SIZE:
// the size query's stage, over the streams of the fast kernels' list only (ks_mark)
template <int C, bool SIZE>
static hipError_t launch_front(const SegsArgs &a, const Scratch &x, uint64_t cap, const KsSize &z, hipStream_t st) {
    uint32_t *listed = SIZE ? x.listed : nullptr;
    const hipError_t e = launch_parts_layout(C, a.in, a.in_off, a.count, a.in_bytes, x.hdr, x.base, listed, cap, 0, st);
    if (e != hipSuccess) return e;
    if (SIZE) hipLaunchKernelGGL(ks_mark, dim3((unsigned)((a.count + 255) / 256 < 1024 ? (a.count + 255) / 256 : 1024)), dim3(256), 0, st, z, a.count, x.hdr, listed);
    // the chip's LDS holds two such blocks per CU at chunk 1,024; the parts beyond go round the grid
    hipLaunchKernelGGL(ks_first<C>, dim3((unsigned)(cap < 2048 ? cap : 2048)), dim3(64), 0, st, a, x.hdr, x.base, (const uint32_t *)listed, x.recs);
    hipLaunchKernelGGL((ks_order<C, SIZE>), dim3((unsigned)(a.count < 2048 ? a.count : 2048)), dim3(64), 0, st, a, x.hdr, x.base, x.recs, x.ents,
                       (const uint32_t *)listed, z);
    return hipGetLastError();
}

// a batch's scratch at a chunk size, the caller's own or leased, and the records it holds
// (hipErrorOutOfMemory: not to be had, nothing is launched)
static hipError_t scratch_for(uint64_t in_bytes, int chunk, uint64_t count, void *own, uint64_t own_cap, hipStream_t st, CacheLease &lease, Scratch &x,
                              uint64_t &cap) {
    cap = parts_cap(in_bytes, kp_part_bytes((uint32_t)chunk), count);
    if (cap == 0) return hipErrorOutOfMemory;
    uint8_t *w = nullptr;
    const hipError_t e = scratch().acquire(own, own_cap, scratch_at(nullptr, count, cap).bytes, st, lease, &w);
    if (e == hipSuccess) x = scratch_at(w, count, cap);
    return e;
}

// The size query's stage for the handed-over streams that have parts: the first and order passes in
// place of k2g_size's walk (no fill), over the list the fast kernels wrote (a.slow).  *gate, *base: for
// k2g_size behind it, which then walks only the listed streams without parts (all of them where the
// gate stays closed).  lease: the scratch, held until k2g_size is launched.
hipError_t launch_size_segs_parts(const DecompressArgs &a, int chunk, hipStream_t st, CacheLease &lease, const uint32_t **gate, const uint32_t **base) {
    Scratch x;
    uint64_t cap;
    // (the header's counters are this stage's now: segs_parts_last reports them, with no parts filled)
    const hipError_t e = scratch_for(a.in_bytes, chunk, a.count, nullptr, 0, st, lease, x, cap);
    if (e != hipSuccess) return e;
    SegsArgs q{};
    q.in = a.in;
    q.in_off = a.in_off;
    q.count = a.count;
    q.block_size_limit = a.block_size_limit;
    q.in_bytes = a.in_bytes;
    const KsSize z{a.slow, a.out_size, a.status, size_segs_counters(a.slow, a.count)};
    *gate = x.hdr + kHGate;
    *base = x.base;
    return chunk == 1024 ? launch_front<1024, true>(q, x, cap, z, st) : launch_front<256, true>(q, x, cap, z, st);
}

hipError_t launch_segs_parts(SegsArgs &a, int chunk, hipStream_t st, CacheLease &lease) {
    Scratch x;
    uint64_t cap;
    const hipError_t e = scratch_for(a.in_bytes, chunk, a.count, a.pws, a.pws_cap, st, lease, x, cap);
    if (e != hipSuccess) return e;
    a.parts_gate = x.hdr + kHGate;
    a.parts_base = x.base;
    a.pws = x.hdr;
    a.pws_cap = cap;  // (from here on: the records the scratch holds)
    return chunk == 1024 ? launch_front<1024, false>(a, x, cap, KsSize{}, st) : launch_front<256, false>(a, x, cap, KsSize{}, st);
}

hipError_t launch_segs_parts_fill(const SegsArgs &a, int chunk, hipStream_t st) {
    const uint64_t cap = a.pws_cap;
    const Scratch x = scratch_at((uint8_t *)a.pws, a.count, cap);
    const unsigned grid = (unsigned)(cap < 2048 ? cap : 2048);
    if (chunk == 1024) hipLaunchKernelGGL(ks_fill<1024>, dim3(grid), dim3(64), 0, st, a, x.hdr, x.base, x.recs, x.ents);
    else hipLaunchKernelGGL(ks_fill<256>, dim3(grid), dim3(64), 0, st, a, x.hdr, x.base, x.recs, x.ents);
    return hipGetLastError();
}

// of the last direct query, or of the size query's stage if that ran later: parts walked in the first
// pass, records taken as they stood, parts walked again, parts filled (zeros where the route did not
// run); the caller has synchronised the query's stream
hipError_t segs_parts_last(uint64_t counts[4]) {
    uint32_t h[kHWords];
    const hipError_t e = scratch().last(h);
    counts[0] = h[kHFirst];
    counts[1] = h[kHJoined];
    counts[2] = h[kHAgain];
    counts[3] = h[kHFilled];
    return e;
}

}  // namespace ez
