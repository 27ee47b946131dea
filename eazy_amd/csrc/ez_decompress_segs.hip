// ez_decompress_segs.hip — K2g: where the streams of a batch can be cut at a MetaReset after output
// (ez_stream_segments_batch), the decode over those cuts (ez_decompress_batch_segmented) and the merge
// of its per-segment results (ez_segments_merge_batch).
//
// Reader.reset (reader.go:327-344) zeroes the block and sets r.pos = 0: a stream with k Resets after
// output is k + 1 streams that decode on their own, and every fast decoder hands such a stream over
// whole.  K2g finds the cuts on the device, so that the decoders get one stream per segment.  The
// walk is K2z's (ez_decompress_size.hip: one wave per stream, grid-stride, super-blocks of 64 chunks
// staged in LDS, a chunk per lane, settled by kz_walk, ez_k2_walk.h); in place of kz_sum, the steps of
// ez_k2_segs.h:
//   sum      kg_sum over each lane's true chain up to the chunk's first event (a MetaReset, a form
//            k2_scan hands over);
//   reduce   an in-order prefix over the lanes for the output bytes; a super-block without an event
//            adds its output and longest distance to the stream's state and is done;
//   cuts     else the events in lane order: the state is brought up to the event from the prefix, and
//            every lane runs kg_cuts from there to that chunk's exit (one chain, one state: the walk is
//            wave-uniform), which records the cuts and stops the stream's walk at the first segment
//            that fails K2z's checks.  What follows a stop is the last segment: the decoders see it as
//            they see the whole stream today, so the results are equal by construction.
// Two launches of the walk with a scan between them:
//   count    every stream is walked; seg_idx[s] = its segments, and its first kGKeep cuts are kept;
//   scan     one block: seg_idx becomes the exclusive scan; more segments than seg_cap: the
//            one-segment-per-stream layout instead;
//   heads    a thread per stream: each stream's first segment, the kept cuts, the arrays' ends;
//   fill     the walk again, only for streams with more than kGKeep cuts, which writes them in place.
// A stream without a Reset after output is walked once.
// With the caller's in_bytes hint, few long streams take the parts route instead
// (ez_decompress_segs_parts.hip: its passes go before the count pass and behind the fill pass, and the
// walk here then skips the streams that have parts).
// The size query (ez_decompressed_size_batch) runs the same walk in one more kernel, k2g_size, over the
// streams its fast kernels handed over: the walk's total is a concatenated stream's decoded length.
#include <hip/hip_runtime.h>

#include <atomic>
#include <mutex>

#include "ez_bytes.h"
#include "ez_cache.h"
#include "ez_internal.h"
#include "ez_k2_segs.h"
#include "ez_k2_walk.h"

namespace ez {
namespace {

constexpr uint32_t kGKeep = 15;  // cuts the count pass keeps per stream (streams of up to 16 segments are walked once)

// One stream b[0 .. nb) by the whole wave: super-blocks through kz_walk, kg_sum, the in-order prefix and
// the events in lane order through kg_cuts, which calls cut(i, pos, out) on every lane for cut i.
// Returns the stream's state and where its chain ended (both wave-uniform).
struct KgEnd {
    KgState st;
    uint32_t end;
};
template <int C, class Cut>
__device__ __forceinline__ KgEnd kg_stream(uint8_t *stage, uint32_t (*bm)[C / 32 + 1], const uint8_t *b, uint32_t nb, int32_t lim32,
                                           int64_t limit, Cut cut) {
    const int lane = lane_id();
    KgState st = kg_start();
    uint32_t sb = 0;
    while (!st.stop && sb < nb) {
        const KzWalk k = kz_walk<C>(stage, bm, b, nb, sb, sb, true, sb);
        if (!k.settled) {
            st.stop = true;
            break;
        }
        const KzWin w{stage, sb};
        const KgSum r = kg_sum<C>(w, sb, lane, nb, k.a, k.x, lim32, limit);
        const uint64_t io = wscan_add_u64(r.out);
        uint64_t ev = wballot(r.fl != 0);
        uint64_t base = 0;  // the prefix taken into the state so far
        int from = 0;       // the first lane whose distances are not in the state yet
        while (ev) {
            const int j = ffs64(ev);
            ev &= ev - 1;
            // the lanes before j, and lane j's tokens before its event
            const uint64_t ioj = __shfl(io, j, kWave);
            st.total += ioj - base;
            base = ioj;
            st.maxd = max(st.maxd, wmax_u32(lane >= from && lane <= j ? r.maxd : 0u));
            from = j + 1;
            kg_cuts<C>(w, sb, j, nb, (uint32_t)__shfl((int)r.epos, j, kWave), (uint32_t)__shfl((int)k.x, j, kWave), lim32, limit, st, cut);
            if (st.stop) break;
        }
        if (st.stop) break;
        st.total += __shfl(io, kWave - 1, kWave) - base;
        st.maxd = max(st.maxd, wmax_u32(lane >= from ? r.maxd : 0u));
        sb = __shfl(k.x, kWave - 1, kWave);
    }
    return KgEnd{st, sb};
}

template <int C, bool FILL>
__global__ __launch_bounds__(64) void k2g_walk(SegsArgs A) {
    constexpr int W = C / 32;
    __shared__ __attribute__((aligned(16))) uint8_t stage[kz_stage_bytes(C)];
    __shared__ uint32_t bm[kZLanes][W + 1];  // (+1: the lanes' rows on distinct banks)
    if (FILL && A.hdr[0]) return;            // (the one-segment-per-stream layout: no cuts to write)
    const int lane = lane_id();
    const int64_t limit = A.block_size_limit;
    const int32_t lim32 = k2_lim32(limit);
    const bool parted = A.parts_gate && *A.parts_gate;  // (the parts route walks the streams that have parts)
    for (uint64_t s = blockIdx.x; s < A.count; s += gridDim.x) {
        if (parted && A.parts_base[s] != A.parts_base[s + 1]) continue;
        uint64_t g0 = 0, nseg = 0;
        if (FILL) {
            g0 = A.seg_idx[s];
            nseg = A.seg_idx[s + 1] - g0;
            if (nseg <= kGKeep + 1) continue;  // (the heads wrote its kept cuts)
        }
        const uint64_t i0 = A.in_off[s], nb64 = A.in_off[s + 1] - i0;
        const uint8_t *b = A.in + i0;
        const uint32_t nb = nb64 >= (1ull << 31) ? 0u : (uint32_t)nb64;  // (2 GiB or more: no cuts)
        const uint64_t o0 = FILL ? A.out_off[s] : 0, o1 = FILL ? A.out_off[s + 1] : 0;
        auto cut = [&](uint32_t i, uint32_t pos, uint64_t out) {
            if (lane != 0) return;
            if (!FILL) {
                if (i < kGKeep) {
                    A.keep[(s * kGKeep + i) * 2] = pos;
                    A.keep[(s * kGKeep + i) * 2 + 1] = out;
                }
            } else if ((uint64_t)i + 1 < nseg) {
                A.seg_in[g0 + 1 + i] = i0 + pos;
                A.seg_out[g0 + 1 + i] = out < o1 - o0 ? o0 + out : o1;
            }
        };
        const KgEnd r = kg_stream<C>(stage, bm, b, nb, lim32, limit, cut);
        if (!FILL && lane == 0) A.seg_idx[s] = (uint64_t)r.st.ncut + 1;
    }
}

// The size query's stage behind K2z (launch_decompress_size): a wave per entry of the list K2z's kernels
// and the parts route wrote (first: [0] = its length, read here, on the device), grid-stride.  The walk
// is k2g_walk's with a cut that stores nothing, and kg_end_ok decides at the stream's end: the wave
// writes out_size[s] = the total and EZ_OK, or appends the stream to the second list for the exact
// decoder run dry (a stop, an unsettled super-block, 2 GiB or more, a failed end check).  The first
// list is only read.  ctr: {entries taken, streams sized, the second list: [0] = its length, which is
// the streams handed on}, zeroed by the launcher.
template <int C>
__global__ __launch_bounds__(64) void k2g_size(DecompressArgs A, const uint32_t *first, uint32_t *ctr, const uint32_t *gate, const uint32_t *base) {
    constexpr int W = C / 32;
    __shared__ __attribute__((aligned(16))) uint8_t stage[kz_stage_bytes(C)];
    __shared__ uint32_t bm[kZLanes][W + 1];  // (+1: the lanes' rows on distinct banks)
    const uint64_t n = first[0] < A.count ? first[0] : A.count;  // (a list is never longer than the batch: the second one has room for that)
    const int lane = lane_id();
    const int64_t limit = A.block_size_limit;
    const int32_t lim32 = k2_lim32(limit);
    const bool parted = gate && *gate;  // (the parts route's stage sized the listed streams that have parts)
    uint32_t sized = 0;
    for (uint64_t k = blockIdx.x; k < n; k += gridDim.x) {
        const uint64_t s = first[1 + k];
        if (parted && base[s] != base[s + 1]) continue;
        const uint64_t nb64 = A.in_off[s + 1] - A.in_off[s];
        bool ok = nb64 < (1ull << 31);
        uint64_t total = 0;
        if (ok) {
            const uint32_t nb = (uint32_t)nb64;
            const KgEnd r = kg_stream<C>(stage, bm, A.in + A.in_off[s], nb, lim32, limit, [](uint32_t, uint32_t, uint64_t) {});
            ok = kg_end_ok(r.st, r.end, nb);
            total = r.st.total;
        }
        if (lane == 0) {
            if (ok) {
                A.out_size[s] = total;
                if (A.status) A.status[s] = EZ_OK;
                sized++;
            } else {
                const uint32_t at = atomicAdd(&ctr[2], 1u);
                ctr[3 + at] = (uint32_t)s;
            }
        }
    }
    if (lane == 0) {
        if (blockIdx.x == 0) ctr[0] = (uint32_t)n;
        if (sized) atomicAdd(&ctr[1], sized);
    }
}

// seg_idx[0 .. count) holds every stream's segments: one block turns it into the exclusive scan
// (seg_idx[count] = the segments found), or, where those exceed seg_cap, into 0, 1, .. count
constexpr int kScanThreads = 1024;
__global__ __launch_bounds__(kScanThreads) void k2g_scan(SegsArgs A) {
    __shared__ uint64_t part[kScanThreads];
    const uint64_t per = (A.count + kScanThreads - 1) / kScanThreads;
    const uint64_t lo = (uint64_t)threadIdx.x * per < A.count ? (uint64_t)threadIdx.x * per : A.count;
    const uint64_t hi = lo + per < A.count ? lo + per : A.count;
    uint64_t sum = 0;
    for (uint64_t s = lo; s < hi; s++) sum += A.seg_idx[s];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int d = 1; d < kScanThreads; d <<= 1) {
        const uint64_t v = (int)threadIdx.x >= d ? part[threadIdx.x - d] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    const uint64_t found = part[kScanThreads - 1];
    const bool over = found > A.seg_cap;
    uint64_t run = part[threadIdx.x] - sum;
    for (uint64_t s = lo; s < hi; s++) {
        const uint64_t n = A.seg_idx[s];
        A.seg_idx[s] = over ? s : run;
        run += n;
    }
    if (threadIdx.x == 0) {
        A.seg_idx[A.count] = over ? A.count : found;
        A.seg_total[0] = over ? A.count : found;
        A.seg_total[1] = found;
        A.hdr[0] = over ? 1u : 0u;
    }
}

__global__ void k2g_heads(SegsArgs A) {
    const bool over = A.hdr[0] != 0;
    const bool parted = A.parts_gate && *A.parts_gate;
    for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s <= A.count; s += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t g = A.seg_idx[s];
        A.seg_in[g] = A.in_off[s];  // (s == count: the arrays' ends)
        A.seg_out[g] = A.out_off[s];
        if (s == A.count || over) continue;
        if (parted && A.parts_base[s] != A.parts_base[s + 1]) continue;  // (the parts route's fill writes its cuts)
        const uint64_t n = A.seg_idx[s + 1] - g;
        if (n > kGKeep + 1) continue;  // (the fill pass walks it again)
        const uint64_t o0 = A.out_off[s], o1 = A.out_off[s + 1];
        for (uint64_t i = 0; i + 1 < n; i++) {
            const uint64_t out = A.keep[(s * kGKeep + i) * 2 + 1];
            A.seg_in[g + 1 + i] = A.in_off[s] + A.keep[(s * kGKeep + i) * 2];
            A.seg_out[g + 1 + i] = out < o1 - o0 ? o0 + out : o1;
        }
    }
}

// per stream, its first segment whose status is not EZ_OK, else its last
__global__ void k2g_merge(const uint64_t *out_off, uint64_t *out_size, int32_t *status, uint64_t count, const uint64_t *seg_idx,
                          const uint64_t *seg_out, const uint64_t *seg_size, const int32_t *seg_status, const uint32_t *slow,
                          uint64_t *handed) {
    for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < count; s += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t g = seg_idx[s];
        const uint64_t ge = seg_idx[s + 1];
        while (g + 1 < ge && seg_status[g] == EZ_OK) g++;
        out_size[s] = seg_out[g] - out_off[s] + seg_size[g];
        if (status) status[s] = seg_status[g];
    }
    if (handed && blockIdx.x == 0 && threadIdx.x == 0) *handed = slow[0];
}

// the segmented decode's hints: h[2] = the largest segment slot, h[3] and h[4] = the batch's extents
// (h[0], h[1]: seg_total)
__global__ void k2g_hints(const uint64_t *in_off, const uint64_t *out_off, uint64_t count, const uint64_t *seg_out, uint64_t *h) {
    const uint64_t nseg = h[0];
    uint64_t m = 0;
    for (uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; g < nseg; g += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t d = seg_out[g + 1] - seg_out[g];
        m = d > m ? d : m;
    }
    if (m) atomicMax((unsigned long long *)&h[2], (unsigned long long)m);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        h[3] = in_off[count] - in_off[0];
        h[4] = out_off[count] - out_off[0];
    }
}

unsigned grid_for(uint64_t n, unsigned threads, unsigned most) {
    const uint64_t blocks = (n + threads - 1) / threads;
    return (unsigned)(blocks < 1 ? 1 : (blocks < most ? blocks : most));
}

}  // namespace

// [header: 16 words, word 0 = the one-segment-per-stream layout was taken][kept cuts: count x kGKeep x (input position, output bytes)]
uint64_t segments_workspace_bytes(uint64_t count) { return 64 + count * kGKeep * 16; }

hipError_t launch_segments(const SegsArgs &a0, uint64_t max_len, void *workspace, hipStream_t st) {
    SegsArgs a = a0;
    a.hdr = (uint32_t *)workspace;
    a.keep = (uint64_t *)((uint8_t *)workspace + 64);
    const int chunk = size_chunk(max_len);
    // every wave of the chip busy at most (32 per CU); the streams beyond go round the grid
    const unsigned grid = (unsigned)(a.count < 8192 ? a.count : 8192);
    hipError_t e;
    // The parts route (ez_decompress_segs_parts.hip) needs the batch's extent to size its records
    // without a read-back: only with the caller's in_bytes hint, and where segs_parts_route picks it or
    // it is forced.  Without its scratch the batch takes the wave route.
    a.parts_gate = a.parts_base = nullptr;
    int pchunk = segs_parts_route(max_len, a.count, a.in_bytes);
    CacheLease please;  // (its scratch, until the last launch)
    if (pchunk) {
        e = launch_segs_parts(a, pchunk, st, please);
        if (e == hipErrorOutOfMemory) {
            pchunk = 0;
            a.parts_gate = a.parts_base = nullptr;
        } else if (e != hipSuccess) {
            return e;
        }
    }
    if (!pchunk) segs_parts_none();
    if (a.count != 0) {
        if (chunk == 64) hipLaunchKernelGGL((k2g_walk<64, false>), dim3(grid), dim3(64), 0, st, a);
        else if (chunk == 1024) hipLaunchKernelGGL((k2g_walk<1024, false>), dim3(grid), dim3(64), 0, st, a);
        else hipLaunchKernelGGL((k2g_walk<256, false>), dim3(grid), dim3(64), 0, st, a);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k2g_scan, dim3(1), dim3(kScanThreads), 0, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k2g_heads, dim3(grid_for(a.count + 1, 256, 1024)), dim3(256), 0, st, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (a.count != 0) {
        if (chunk == 64) hipLaunchKernelGGL((k2g_walk<64, true>), dim3(grid), dim3(64), 0, st, a);
        else if (chunk == 1024) hipLaunchKernelGGL((k2g_walk<1024, true>), dim3(grid), dim3(64), 0, st, a);
        else hipLaunchKernelGGL((k2g_walk<256, true>), dim3(grid), dim3(64), 0, st, a);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (pchunk && (e = launch_segs_parts_fill(a, pchunk, st)) != hipSuccess) return e;
    return hipSuccess;
}

// The size query's slow area, 2 * count + 32 words: [the first list: count + 1][taken, sized][the second
// list: 1 + count] ... [word 2 * count + 31: largest_slot's].
uint32_t *size_segs_counters(uint32_t *slow, uint64_t count) { return slow + count + 1; }

hipError_t launch_size_segs(const DecompressArgs &a, uint64_t max_len, hipStream_t st, bool parts) {
    uint32_t *ctr = size_segs_counters(a.slow, a.count);
    const int chunk = size_chunk(max_len);
    // The parts route's stage for the listed streams that have parts, where the caller gave in_bytes
    // (the same hint and gate as ez_stream_segments_batch's; not for a caller with its own scratch, a
    // Reader handle).  Without its scratch k2g_size walks the whole list.
    const uint32_t *gate = nullptr, *base = nullptr;
    CacheLease please;
    const int pchunk = parts ? segs_parts_route(max_len, a.count, a.in_bytes) : 0;
    if (pchunk) {
        const hipError_t e = launch_size_segs_parts(a, pchunk, st, please, &gate, &base);
        if (e == hipErrorOutOfMemory) gate = base = nullptr;
        else if (e != hipSuccess) return e;
    }
    if (!gate) segs_parts_none();
    // (a block per listed stream; the list's length is on the device: the blocks past it leave at once)
    const unsigned grid = (unsigned)(a.count < 8192 ? a.count : 8192);
    if (chunk == 64) hipLaunchKernelGGL(k2g_size<64>, dim3(grid), dim3(64), 0, st, a, a.slow, ctr, gate, base);
    else if (chunk == 1024) hipLaunchKernelGGL(k2g_size<1024>, dim3(grid), dim3(64), 0, st, a, a.slow, ctr, gate, base);
    else hipLaunchKernelGGL(k2g_size<256>, dim3(grid), dim3(64), 0, st, a, a.slow, ctr, gate, base);
    return hipGetLastError();
}

hipError_t launch_segments_merge(const uint64_t *out_off, uint64_t *out_size, int32_t *status, uint64_t count, const uint64_t *seg_idx,
                                 const uint64_t *seg_out, const uint64_t *seg_size, const int32_t *seg_status, const uint32_t *slow,
                                 uint64_t *handed, hipStream_t st) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(k2g_merge, dim3(grid_for(count, 256, 1024)), dim3(256), 0, st, out_off, out_size, status, count, seg_idx, seg_out,
                       seg_size, seg_status, slow, handed);
    return hipGetLastError();
}

DevCache &segs_cache() {
    static DevCache *c = new DevCache();  // (never destroyed: no hipFree after the runtime's teardown)
    return *c;
}

namespace {
// the last segmented decode (ez_segments_last)
std::mutex g_last_mu;
struct {
    bool any = false;
    int dev = 0;
    void *stream = nullptr;
    uint64_t segments = 0, retries = 0;
} g_last;

// the scratch of a segmented decode of count streams in at most cap segments
struct SegScratch {
    uint64_t *hints, *seg_idx, *seg_in, *seg_out, *seg_size;
    void *qws, *pws;
    uint32_t *dws;
    int32_t *seg_status;
    size_t bytes;
};
constexpr size_t kHintBytes = 64;  // {written, found, largest slot, in bytes, out bytes, handed over}
SegScratch seg_scratch(uint8_t *p, uint64_t count, uint64_t cap, uint64_t pbytes) {
    SegScratch x;
    size_t o = 0;
    auto take = [&](size_t n) {
        uint8_t *q = (uint8_t *)((uintptr_t)p + o);  // (p == nullptr: the sizes only)
        o += (n + 15) & ~(size_t)15;
        return q;
    };
    x.hints = (uint64_t *)take(kHintBytes);
    x.seg_idx = (uint64_t *)take((count + 1) * 8);
    x.seg_in = (uint64_t *)take((cap + 1) * 8);
    x.seg_out = (uint64_t *)take((cap + 1) * 8);
    x.seg_size = (uint64_t *)take(cap * 8);
    x.qws = take(segments_workspace_bytes(count));
    x.pws = take(pbytes);  // (the query's parts route, carved out of this lease)
    x.dws = (uint32_t *)take(decompress_workspace_words(cap) * 4);
    x.seg_status = (int32_t *)take(cap * 4);
    x.bytes = o;
    return x;
}
}  // namespace

hipError_t launch_decompress_segmented(const DecompressArgs &a, hipStream_t st) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    uint64_t segments = 0, retries = 0;
    if (a.count != 0) {
        CacheLease lease = segs_cache().acquire(dev, (void *)st);
        // room for a segment per stream and some more, or for what the scratch held last time
        uint64_t cap = a.count + a.count / 2 + 1024;
        // the query's parts route, where the caller's in_bytes hint lets it run
        const uint64_t pbytes = segs_parts_route(0, a.count, a.in_bytes) ? segs_parts_workspace_bytes(a.count, a.in_bytes) : 0;
        for (uint64_t step = 1ull << 36; step; step >>= 1)
            if (seg_scratch(nullptr, a.count, cap + step, pbytes).bytes <= lease->cap) cap += step;
        uint64_t h[5] = {0, 0, 0, 0, 0};
        SegScratch x;
        for (;;) {
            x = seg_scratch(nullptr, a.count, cap, pbytes);
            if (!lease->ensure(x.bytes)) return hipErrorOutOfMemory;
            x = seg_scratch((uint8_t *)lease->p, a.count, cap, pbytes);
            if ((e = hipMemsetAsync(x.hints, 0, kHintBytes, st)) != hipSuccess) return e;
            SegsArgs q{};
            q.in = a.in;
            q.in_off = a.in_off;
            q.out_off = a.out_off;
            q.count = a.count;
            q.block_size_limit = a.block_size_limit;
            q.seg_idx = x.seg_idx;
            q.seg_in = x.seg_in;
            q.seg_out = x.seg_out;
            q.seg_cap = cap;
            q.seg_total = x.hints;
            q.in_bytes = pbytes ? a.in_bytes : 0;
            q.pws = pbytes ? x.pws : nullptr;
            q.pws_cap = pbytes;
            if ((e = launch_segments(q, 0, x.qws, st)) != hipSuccess) return e;
            hipLaunchKernelGGL(k2g_hints, dim3(grid_for(cap, 256, 1024)), dim3(256), 0, st, a.in_off, a.out_off, a.count, x.seg_out, x.hints);
            if ((e = hipGetLastError()) != hipSuccess) return e;
            if ((e = hipMemcpyAsync(h, x.hints, sizeof h, hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
            if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
            if (h[1] <= h[0] || retries != 0) break;
            cap = h[1];  // (more segments than there was room for: once more, with room)
            retries++;
        }
        segments = h[0];
        DecompressArgs d{};
        d.in = a.in;
        d.in_off = x.seg_in;
        d.out = a.out;
        d.out_off = x.seg_out;
        d.out_size = x.seg_size;
        d.status = x.seg_status;
        d.count = segments;
        d.block_size_limit = a.block_size_limit;
        d.slow = x.dws;
        d.max_out = h[2];
        d.in_bytes = h[3];
        d.out_bytes = h[4];
        if ((e = launch_decompress(d, st)) != hipSuccess) return e;
        if ((e = launch_segments_merge(a.out_off, a.out_size, a.status, a.count, x.seg_idx, x.seg_out, x.seg_size, x.seg_status, x.dws,
                                       x.hints + 5, st)) != hipSuccess)
            return e;
    }
    std::lock_guard<std::mutex> g(g_last_mu);
    g_last.any = a.count != 0;
    g_last.dev = dev;
    g_last.stream = (void *)st;
    g_last.segments = segments;
    g_last.retries = retries;
    return hipSuccess;
}

hipError_t segments_last(uint64_t counts[3]) {
    std::lock_guard<std::mutex> g(g_last_mu);
    counts[0] = g_last.segments;
    counts[1] = 0;
    counts[2] = g_last.retries;
    if (!g_last.any) return hipSuccess;
    CacheLease lease = segs_cache().acquire(g_last.dev, g_last.stream);
    if (!lease->p || lease->cap < kHintBytes) return hipSuccess;  // (the scratch was released: the count went with it)
    return hipMemcpy(&counts[1], (uint8_t *)lease->p + 5 * 8, 8, hipMemcpyDeviceToHost);
}

}  // namespace ez
